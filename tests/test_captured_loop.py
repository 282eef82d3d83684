"""clipbert_amd.captured: the task loops replayed from captured step graphs.

GPU part (marked `gpu`): a replayed step against the eager tasks.train_step from the same state, per step, over two alternating
signatures -- held to the bounds tests/test_bench_step.py uses for eager against replay (gradients 2e-6 x tensor scale, first-writer
encoder weight gradients bit-equal, parameters 1e-6 x max |p|, gradient norm 1e-5 relative); eviction; fresh dropout masks and fresh
hyper-parameters per replay; every fallback; a capture that raises; ``pad_text_to`` against the CPU oracle's own padded-vs-unpadded
difference in its bf16-storage modes; retrieval inference.  The models are bench_step.build(videos=2, n_clips=2, frames=1, size=128,
txt_len=8, repeat=2) and the small configuration of tests/test_model_small.py.

CPU part (host emulator, ``capture="dry"``: signatures and staging without graphs): signature ingredients, LRU order, the contents of
the static buffers, and start_training(capture=...) against capture=False."""
import copy
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import parity_bounds as PB
from clipbert_amd import captured as CAP
from clipbert_amd import data as D
from clipbert_amd import optim, tasks
from clipbert_amd import synthetic as S
from clipbert_amd._lib import HP_LR
from oracle import clipbert_oracle as O
from test_model_small import build as build_small

NO_DROP = dict(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
RET = dict(num_labels=2, loss_type="ce", margin=0.1, **NO_DROP)


# ---- shared helpers ----------------------------------------------------------------------------------------------------------
def _snapshot(model, opt):
    bank = model.rt.bank
    return dict(master=bank.master.clone(), m=bank.exp_avg.clone(), v=bank.exp_avg_sq.clone(), w16=None if bank.w16 is None else bank.w16.clone(),
                step=opt.step_count, seed=model.rt.seed_dev.clone(), fwd=model.rt.forward_count)


def _restore(model, opt, snap):
    bank = model.rt.bank
    bank.master.copy_(snap["master"]); bank.exp_avg.copy_(snap["m"]); bank.exp_avg_sq.copy_(snap["v"])
    if bank.w16 is not None:
        bank.w16.copy_(snap["w16"])
    opt.step_count = snap["step"]
    model.rt.seed_dev.copy_(snap["seed"])
    model.rt.forward_count = snap["fwd"]


def _result(model, opt, loss):
    if loss.is_cuda:
        torch.cuda.synchronize()
    bank = model.rt.bank
    return SimpleNamespace(grad=bank.grad.clone(), master=bank.master.clone(), norm=float(opt.grad_norm()), loss=float(loss))


def _both(model, opt, run_captured, run_eager):
    """the same step twice from the same state: through the object under test, then eagerly; the eager result is what is kept"""
    snap = _snapshot(model, opt)
    got = _result(model, opt, run_captured())
    _restore(model, opt, snap)
    want = _result(model, opt, run_eager())
    return got, want


def _assert_same_step(model, got, want, what):
    """the bounds of tests/test_bench_step.py for eager against replay"""
    bank = model.rt.bank
    for name, p in bank._trainable:
        off = bank.offset[id(p)]
        sl = slice(off, off + p.numel())
        a, b = want.grad[sl], got.grad[sl]
        scale = float(a.abs().max())
        err = float((a - b).abs().max())
        assert err <= 2e-6 * scale + 1e-12, (what, name, err, scale)
        if "encoder.layer" in name and name.endswith("dense.weight") or name.endswith(("query.weight", "key.weight", "value.weight")):
            if bank.compute_dtype == torch.bfloat16:
                assert torch.equal(a, b), (what, name, "first-writer weight gradients: bit-equal")
    assert abs(want.norm - got.norm) <= 1e-5 * want.norm, (what, want.norm, got.norm)
    assert float((want.master - got.master).abs().max()) <= 1e-6 * float(want.master.abs().max()), what
    assert abs(want.loss - got.loss) <= 1e-6 * max(1.0, abs(want.loss)), (what, want.loss, got.loss)


def _text_batch(frames, per_video, txt_len, seed, vocab=None, dev=None):
    n = frames.shape[0] * per_video
    ids, mask = S.synthetic_text(n, txt_len, seed) if vocab is None else S.synthetic_text(n, txt_len, seed, vocab)
    if vocab is not None:
        ids = ids.clamp(max=vocab - 1)
    labels = torch.tensor(([1] + [0] * (per_video - 1)) * frames.shape[0], dtype=torch.long)
    b = dict(visual_inputs=frames, text_input_ids=ids, text_input_mask=mask, labels=labels, n_examples_list=[per_video] * frames.shape[0])
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}


# ================================================================================================================================
# GPU
# ================================================================================================================================
@pytest.fixture(scope="module")
def full():
    """the metric model at its smallest: 2 videos x 2 clips x 1 frame of 128 px, dropout off; signatures A (2 texts / video, 8 tokens)
    and B (1 text / video, 12 tokens)"""
    from clipbert_amd.bench import step as bench_step
    st = bench_step.build(videos=2, n_clips=2, frames=1, size=128, txt_len=8, repeat=2, dropout=False)
    fr = st.batch["visual_inputs"]
    st.A = [_text_batch(S.synthetic_frames(2, 2, 128, 42 + i).to(st.dev), 2, 8, 42 + i) for i in range(3)]
    st.B = [_text_batch(S.synthetic_frames(2, 2, 128, 52 + i).to(st.dev), 1, 12, 52 + i) for i in range(3)]
    st.A = [{k: (v.to(st.dev) if torch.is_tensor(v) else v) for k, v in b.items()} for b in st.A]
    st.B = [{k: (v.to(st.dev) if torch.is_tensor(v) else v) for k, v in b.items()} for b in st.B]
    st.init = _snapshot(st.model, st.opt)
    assert fr.shape == st.A[0]["visual_inputs"].shape
    return st


def _abab(st):
    return [st.A[0], st.B[0], st.A[1], st.B[1], st.A[2], st.B[2]]


def _run_sequence(st, stepper, batches, first_step=0):
    model, opt = st.model, st.opt
    live = []
    for k, b in enumerate(batches, first_step):
        got, want = _both(model, opt, lambda: stepper.step(b, k), lambda: tasks.train_step(model, opt, b, st.tcfg, k))
        _assert_same_step(model, got, want, f"step {k}")
        live.append(len(stepper.graphs))
    return live


@pytest.mark.gpu
def test_replay_equals_eager_per_step_over_two_signatures(full):
    st = full
    _restore(st.model, st.opt, st.init)
    stepper = CAP.CapturedStep(st.model, st.opt, st.tcfg)
    _run_sequence(st, stepper, _abab(st))
    assert stepper.log == ["eager"] * 4 + ["replay"] * 2, stepper.log            # sights 1 and 2 of A and B eager, sights 3 replays
    assert len(stepper.graphs) == 2 and stepper.stats["captures"] == 2 and stepper.stats["fallbacks"] == 0, stepper.stats
    _run_sequence(st, stepper, _abab(st)[:4], first_step=6)                      # and they stay replays
    assert stepper.log[6:] == ["replay"] * 4 and stepper.stats["captures"] == 2, (stepper.log, stepper.stats)


@pytest.mark.gpu
def test_eviction_recaptures_and_keeps_one_live_graph(full):
    st = full
    _restore(st.model, st.opt, st.init)
    stepper = CAP.CapturedStep(st.model, st.opt, st.tcfg, max_graphs=1)
    live = _run_sequence(st, stepper, _abab(st))
    assert max(live) == 1 and stepper.stats["max_live"] == 1, (live, stepper.stats)
    assert stepper.stats["captures"] > 2 and stepper.stats["evictions"] == stepper.stats["captures"] - 1, stepper.stats
    # the survivor replays: the signature captured last is B
    live += _run_sequence(st, stepper, [st.B[0], st.B[1]], first_step=6)
    assert stepper.log[-2:] == ["replay"] * 2 and max(live) == 1


@pytest.mark.gpu
def test_replays_get_the_learning_rate_of_their_step(full):
    """the device hyper-parameter array after replay k holds get_lr_sched(k + 1, ...) for every group (both schedules are the same here)"""
    st = full
    _restore(st.model, st.opt, st.init)
    stepper = CAP.CapturedStep(st.model, st.opt, st.tcfg)
    seen = []
    for k in (0, 1, 2, 4999, 10000, 60000):
        stepper.step(st.A[0], k)
        want = optim.get_lr_sched(k + 1, "linear", st.tcfg.learning_rate, st.tcfg.num_train_steps, warmup_ratio=st.tcfg.warmup_ratio)
        got = st.opt._hp_dev[:, HP_LR].cpu()
        assert torch.equal(got, torch.full((8,), want, dtype=torch.float32)), (k, got, want)
        seen.append(want)
    assert stepper.log == ["eager"] * 2 + ["replay"] * 4 and len(set(seen)) == len(seen)
    assert st.opt.step_count == st.init["step"] + 6


@pytest.mark.gpu
def test_replays_draw_fresh_dropout_masks():
    from clipbert_amd.bench import step as bench_step
    st = bench_step.build(videos=2, n_clips=2, frames=1, size=128, txt_len=8, repeat=2, dropout=True)
    model, opt, rt = st.model, st.opt, st.model.rt
    stepper = CAP.CapturedStep(model, opt, st.tcfg)
    stepper.step(st.batch, 0); stepper.step(st.batch, 1)
    snap = _snapshot(model, opt)
    seed0 = int(rt.seed_dev.item())
    grads = []
    for i in range(2):
        _restore(model, opt, dict(snap, seed=rt.seed_dev.clone()))             # the same weights and moments; the seed word keeps counting
        loss = stepper.step(st.batch, 2)
        torch.cuda.synchronize()
        assert int(rt.seed_dev.item()) == seed0 + i + 1
        grads.append(model.rt.bank.grad.clone())
        assert torch.isfinite(loss)
    assert stepper.log == ["eager"] * 2 + ["replay"] * 2
    diff = float((grads[0] - grads[1]).abs().max())
    assert diff > 1e-3 * float(grads[0].abs().max()), diff                      # other masks, other gradients


@pytest.fixture(scope="module")
def small_gpu():
    dev = torch.device("cuda", 0)
    out = {}
    for head, extra in (("retrieval", RET), ("pretraining", NO_DROP)):
        cfg, _sd, model = build_small(head, extra, torch.bfloat16, dev)
        model.train(True)
        opt = optim.FusedAdamW(model.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=5.0)
        out[head] = SimpleNamespace(cfg=cfg, model=model, opt=opt, dev=dev)
    return out


def _tcfg(**over):
    base = dict(train_n_clips=2, num_frm=1, score_agg_func="lse", task=None, num_labels=2, gradient_accumulation_steps=1, learning_rate=1e-3,
                cnn_learning_rate=1e-3, decay="linear", cnn_lr_decay="linear", num_train_steps=100, warmup_ratio=0.1)
    return SimpleNamespace(**dict(base, **over))


def _small_frames(seed, size=64, dev=None):
    return S.synthetic_frames(2, 2, size, seed).contiguous().to(dev)             # uint8 (2 videos, 2 clips x 1 frame, 3, size, size)


def _one_warning(caught, reason):
    mine = [w for w in caught if issubclass(w.category, RuntimeWarning) and "runs eagerly" in str(w.message)]
    assert len(mine) == 1 and reason in str(mine[0].message), [str(w.message) for w in caught]


def _expect_fallback(s, tcfg, batches, reason, loss_fn=None, before=None):
    """every step through a fresh CapturedStep and through train_step from the same state: same result, eager, ONE warning"""
    stepper = CAP.CapturedStep(s.model, s.opt, tcfg, loss_fn=loss_fn)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for k, b in enumerate(batches):
            def eager():
                before and before()
                return tasks.train_step(s.model, s.opt, b, tcfg, k, loss_fn=loss_fn)

            def cap():
                before and before()
                return stepper.step(b, k)

            got, want = _both(s.model, s.opt, cap, eager)
            _assert_same_step(s.model, got, want, f"{reason} step {k}")
    _one_warning(caught, reason)
    assert stepper.log == ["eager"] * len(batches) and stepper.stats["fallbacks"] == len(batches) and not stepper.graphs, stepper.stats
    return stepper


@pytest.mark.gpu
def test_fallbacks_run_eagerly_and_warn_once(small_gpu):
    s = small_gpu["retrieval"]
    vocab = s.cfg["vocab_size"]
    plain = [_text_batch(_small_frames(60 + i, dev=s.dev), 2, 6, 60 + i, vocab, s.dev) for i in range(3)]
    # gradient accumulation: the same four micro-steps (two optimizer steps) through the object and through train_step, compared at the end
    acc = _tcfg(gradient_accumulation_steps=2)
    micro = [plain[0], plain[1], plain[2], plain[0]]
    stepper = CAP.CapturedStep(s.model, s.opt, acc)

    def group(step_fn):
        for ms, b in enumerate(micro):
            loss = step_fn(b, ms // 2, ms)
        return loss

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, want = _both(s.model, s.opt, lambda: group(lambda b, k, ms: stepper.step(b, k, micro_step=ms)),
                          lambda: group(lambda b, k, ms: tasks.train_step(s.model, s.opt, b, acc, k, micro_step=ms)))
    _assert_same_step(s.model, got, want, "accumulation groups")
    _one_warning(caught, "gradient_accumulation_steps")
    assert stepper.log == ["eager"] * 4 and stepper.stats["fallbacks"] == 4 and not stepper.graphs and s.opt.step_count >= 2, stepper.stats
    # a tensor the loader left on the host is a reason to stay eager (a graph would run it elsewhere than the eager step does)
    reason = CAP.CapturedStep(s.model, s.opt, _tcfg())._why_eager(dict(plain[0], text_input_mask=plain[0]["text_input_mask"].cpu()))
    assert reason is not None and "text_input_mask is on cpu" in reason, reason
    # RawFrames: native-resolution uint8 frames, resized on the device from a host table
    raw = []
    for i in range(3):
        vids = [torch.randint(0, 256, (2, 40 + 8 * v, 56, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(70 + i + v)) for v in range(2)]
        raw.append(dict(plain[i], visual_inputs=D.collate_raw_frames(vids, 64).to(s.dev)))
    _expect_fallback(s, _tcfg(), raw, "RawFrames")
    # pixel sub-sampling drawn by numpy per forward (both runs of a step start from the same numpy state)
    big = [_text_batch(_small_frames(80 + i, size=128, dev=s.dev), 2, 6, 80 + i, vocab, s.dev) for i in range(3)]
    s.model.config.pixel_random_sampling_size = 2
    try:
        _expect_fallback(s, _tcfg(), big, "pixel_random_sampling_size", before=lambda: np.random.seed(11))
    finally:
        s.model.config.pixel_random_sampling_size = 0


def _pretrain_batches(s, n):
    out = []
    for i in range(n):
        b = _text_batch(_small_frames(90 + i, dev=s.dev), 1, 6, 90 + i, s.cfg["vocab_size"], s.dev)
        del b["labels"]
        g = torch.Generator().manual_seed(90 + i)
        mlm = torch.full((2, 6), -100, dtype=torch.long)
        mlm[0, 1 + i % 3] = int(torch.randint(1, s.cfg["vocab_size"], (1,), generator=g))
        mlm[1, 2] = int(torch.randint(1, s.cfg["vocab_size"], (1,), generator=g))
        out.append(dict(b, mlm_labels=mlm.to(s.dev), itm_labels=torch.tensor([1, 0]).to(s.dev)))
    return out


@pytest.mark.gpu
def test_pretraining_falls_back_without_capacity_and_is_captured_with_it(small_gpu):
    s = small_gpu["pretraining"]
    batches = _pretrain_batches(s, 4)
    _expect_fallback(s, _tcfg(train_n_clips=1, num_frm=2, mlm_rows="labelled", mlm_capacity=None), batches[:3], "mlm_capacity", loss_fn=tasks.pretrain_loss)
    tcfg = _tcfg(train_n_clips=1, num_frm=2, mlm_rows="labelled", mlm_capacity=64)
    stepper = CAP.CapturedStep(s.model, s.opt, tcfg, loss_fn=tasks.pretrain_loss)
    for k, b in enumerate(batches):
        got, want = _both(s.model, s.opt, lambda: stepper.step(b, k), lambda: tasks.train_step(s.model, s.opt, b, tcfg, k, loss_fn=tasks.pretrain_loss))
        _assert_same_step(s.model, got, want, f"pretraining step {k}")
    assert stepper.log == ["eager"] * 2 + ["replay"] * 2 and stepper.stats["captures"] == 1 and stepper.stats["fallbacks"] == 0, stepper.stats


@pytest.mark.gpu
def test_a_failed_capture_leaves_no_trace(full):
    """a HOST exception from the loss function on its first call inside a capture"""
    st = full
    model, opt = st.model, st.opt
    _restore(model, opt, st.init)
    calls = dict(capturing=0)

    def base(m, b, cfg):
        stack = tasks.forward_clips_stack(m, b, cfg.train_n_clips, cfg.num_frm, cfg=cfg)
        return tasks.training_loss(m, stack, b["labels"], b["n_examples_list"], cfg.score_agg_func)

    def flaky(m, b, cfg):
        if torch.cuda.is_current_stream_capturing():
            calls["capturing"] += 1
            if calls["capturing"] == 1:
                raise RuntimeError("loss function refuses to be captured")
        return base(m, b, cfg)

    stepper = CAP.CapturedStep(model, opt, st.tcfg, loss_fn=flaky)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for k in range(4):
            b = st.A[k % 3]
            got, want = _both(model, opt, lambda: stepper.step(b, k), lambda: tasks.train_step(model, opt, b, st.tcfg, k, loss_fn=base))
            _assert_same_step(model, got, want, f"step {k}")
            assert not torch.cuda.is_current_stream_capturing()
    assert calls["capturing"] == 1 and stepper.stats["failed_captures"] == 1 and stepper.stats["captures"] == 0 and not stepper.graphs, stepper.stats
    assert stepper.log == ["eager"] * 4 and len(stepper.uncapturable) == 1
    assert sum("capture failed" in str(w.message) for w in caught) == 1
    # the model is usable afterwards: a fresh object captures and replays this very signature
    again = CAP.CapturedStep(model, opt, st.tcfg)
    _run_sequence(st, again, [st.A[0], st.A[1], st.A[2]], first_step=4)
    assert again.log == ["eager"] * 2 + ["replay"]


@pytest.mark.gpu
def test_pad_text_to_differs_by_attention_rounding_only(full):
    """Logits of the captured step on the batch padded from 8 to 12 text columns against the eager step on the un-padded batch.

    The bound is drawn on this batch by the CPU oracle itself: its own padded-vs-unpadded difference of the same logits in its two
    bf16-storage modes; the product is held to PB.FACTOR x the larger one (tests/parity_bounds.py), as the other bf16 tests are."""
    st = full
    model, opt = st.model, st.opt
    _restore(model, opt, st.init)
    held = {}

    def loss_fn(m, b, cfg):
        stack = tasks.forward_clips_stack(m, b, cfg.train_n_clips, cfg.num_frm, cfg=cfg)
        held["captured" if torch.cuda.is_current_stream_capturing() else "eager"] = stack
        return tasks.training_loss(m, stack, b["labels"], b["n_examples_list"], cfg.score_agg_func)

    b = st.A[0]
    stepper = CAP.CapturedStep(model, opt, st.tcfg, loss_fn=loss_fn, pad_text_to=12)
    snap = _snapshot(model, opt)
    for k in range(3):
        _restore(model, opt, snap)
        stepper.step(b, 0)
    torch.cuda.synchronize()
    assert stepper.log == ["eager", "eager", "replay"]
    assert stepper.graphs and next(iter(stepper.graphs.values())).bufs["text_input_ids"].shape == (4, 12)
    padded = held["captured"].detach().float().cpu().clone()        # the graph's own logits tensor, as the replay left it
    assert padded.shape == (2, 4, 2) and bool(torch.isfinite(padded).all())
    _restore(model, opt, snap)
    tasks.train_step(model, opt, b, st.tcfg, 0, loss_fn=loss_fn)
    plain = held["eager"].detach().float().cpu().clone()
    got = float((padded - plain).abs().max())

    frames, ids, mask = b["visual_inputs"].cpu(), b["text_input_ids"].cpu(), b["text_input_mask"].cpu()
    pad = (0, 4)
    ids_p, mask_p = torch.nn.functional.pad(ids, pad, value=0), torch.nn.functional.pad(mask, pad, value=0)

    def oracle_logits(mode, ids, mask):
        with torch.no_grad(), O.precision(mode):
            vis = O.image_norm(frames, S.PIXEL_MEAN, S.PIXEL_STD).view(2, 2, 1, 3, 128, 128)
            return torch.stack([O.clipbert_forward(st.state_dict, dict(visual_inputs=vis[:, c], text_input_ids=ids, text_input_mask=mask,
                                                                       n_examples_list=[2, 2]), st.cfg, "retrieval")["logits"].float() for c in range(2)])

    yard = {m: float((oracle_logits(m, ids_p, mask_p) - oracle_logits(m, ids, mask)).abs().max()) for m in PB.MODES}
    rec = dict(product_padded_vs_unpadded=got, oracle_padded_vs_unpadded=yard, logits_scale=float(plain.abs().max()), bound=PB.FACTOR * max(yard.values()))
    print("[pad_text_to]", rec)
    assert got <= PB.FACTOR * max(yard.values()), rec


@pytest.mark.gpu
def test_inference_retrieval_video_replays_its_encoder_passes(full):
    """3 clips x 5 captions at inference_batch_size 2: one full (2 captions) and one remainder (1 caption) signature; scores bit-equal"""
    st = full
    model = st.model
    _restore(model, st.opt, st.init)
    cfg = copy.copy(st.tcfg)
    cfg.inference_n_clips, cfg.num_frm, cfg.inference_batch_size = 3, 1, 2
    model.eval()
    try:
        for i in range(3):
            vis = S.synthetic_frames(1, 3, 128, 7 + i).to(st.dev)
            ids, mask = (t.to(st.dev) for t in S.synthetic_text(5, 8, 7 + i))
            want = tasks.inference_retrieval_video(model, vis, ids, mask, cfg)
            got = tasks.inference_retrieval_video(model, vis, ids, mask, cfg, capture=True)
            assert got == want and len(got) == 5, (i, got, want)
        cf = model._captured_forward
        assert cf.stats["captures"] == 2 and len(cf.graphs) == 2 and cf.log[-3:] == ["replay"] * 3, (cf.stats, cf.log)
        assert cf.log == ["eager"] * 3 + ["replay", "replay", "eager"] + ["replay"] * 3, cf.log
        # the raw logits of a replay against the eager pass, not only the rounded scores
        with torch.no_grad():
            grid = model.grid_features(vis.view(3, 1, 3, 128, 128))
            a = cf.logits(grid, ids[:2].repeat(3, 1), mask[:2].repeat(3, 1), [2] * 3)
            b = model.forward_from_grid(dict(visual_inputs=grid, text_input_ids=ids[:2].repeat(3, 1), text_input_mask=mask[:2].repeat(3, 1), labels=None,
                                             n_examples_list=[2] * 3))["logits"]
        assert cf.log[-1] == "replay" and torch.equal(a, b)
        with pytest.raises(ValueError):
            tasks.inference_retrieval_video(model, vis, ids, mask, cfg, cache_cnn=False, capture=True)
    finally:
        model.train(True)
        model._captured_forward = None


# ================================================================================================================================
# host emulator: capture="dry"
# ================================================================================================================================
@pytest.fixture()
def small_cpu(emul):
    cfg, _sd, model = build_small("retrieval", RET, torch.float32, torch.device("cpu"))
    model.train(True)
    opt = optim.FusedAdamW(model.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=5.0)
    return SimpleNamespace(cfg=cfg, model=model, opt=opt, dev=torch.device("cpu"))


def test_signature_changes_with_every_ingredient(small_cpu):
    s = small_cpu
    vocab = s.cfg["vocab_size"]
    b = _text_batch(_small_frames(1), 2, 6, 1, vocab)
    mk = lambda tcfg=None, **kw: CAP.CapturedStep(s.model, s.opt, tcfg or _tcfg(), mode="dry", **kw)       # noqa: E731
    base = mk().signature(b)
    assert base == mk().signature(_text_batch(_small_frames(2), 2, 6, 2, vocab))                          # other values, same signature
    assert hash(base) is not None
    other = [
        mk().signature(dict(b, text_input_ids=b["text_input_ids"].to(torch.int32))),                       # dtype
        mk().signature(_text_batch(_small_frames(1), 2, 7, 1, vocab)),                                     # shape (text length)
        mk().signature(dict(b, visual_inputs=b["visual_inputs"].to("meta"))),                              # device
        mk().signature(dict(b, n_examples_list=[3, 1])),                                                   # n_examples_list
        mk(_tcfg(train_n_clips=1, num_frm=2)).signature(b), mk(_tcfg(num_frm=2)).signature(b),             # train_n_clips, num_frm
        mk(_tcfg(score_agg_func="mean")).signature(b), mk(_tcfg(task="action")).signature(b), mk(_tcfg(num_labels=5)).signature(b),
        mk(_tcfg(mlm_rows="all")).signature(b), mk(_tcfg(mlm_capacity=64)).signature(b),                    # pretraining
        mk().signature(dict(b, itm_labels=torch.tensor([1, 0]))), mk().signature({k: v for k, v in b.items() if k != "labels"}),    # optional keys
        mk().signature(dict(b, labels=None)), mk(fold_clips=False).signature(b),
    ]
    s.model.train(False)
    other.append(mk().signature(b))                                                                        # model.training
    s.model.train(True)
    assert all(o != base for o in other) and len(set(other)) == len(other)
    # pad_text_to folds the text lengths into one signature
    padder = mk(pad_text_to=9)
    sigs = {padder.signature(padder._pad(_text_batch(_small_frames(1), 2, lt, 1, vocab))) for lt in (5, 6, 9)}
    assert len(sigs) == 1
    padded = padder._pad(b)
    assert padded["text_input_ids"].shape == (4, 9) and torch.equal(padded["text_input_ids"][:, :6], b["text_input_ids"])
    assert not padded["text_input_ids"][:, 6:].any() and not padded["text_input_mask"][:, 6:].any()
    with pytest.raises(ValueError):
        padder._pad(_text_batch(_small_frames(1), 2, 10, 1, vocab))


def test_lru_order_and_static_buffers_hold_exactly_the_batch(small_cpu, monkeypatch):
    """bookkeeping only: the eager step is replaced by a recorder of the batch it was handed"""
    s = small_cpu
    vocab = s.cfg["vocab_size"]
    handed = []
    monkeypatch.setattr(tasks, "train_step", lambda model, opt, batch, *a, **kw: handed.append(batch) or torch.zeros(()))
    stepper = CAP.CapturedStep(s.model, s.opt, _tcfg(), mode="dry", max_graphs=2)
    mkb = lambda lt, seed: _text_batch(_small_frames(seed), 2, lt, seed, vocab)      # noqa: E731
    sig = lambda lt: stepper.signature(mkb(lt, 0))                                    # noqa: E731
    step = 0
    for lt in (5, 5, 6, 6):                     # two signatures seen twice: both hold a (dry) graph, 5 is the older one
        stepper.step(mkb(lt, lt), step); step += 1
    assert list(stepper.graphs) == [sig(5), sig(6)] and stepper.log == ["eager"] * 4
    stepper.step(mkb(5, 9), step); step += 1    # a replay makes 5 the most recently used
    assert list(stepper.graphs) == [sig(6), sig(5)] and stepper.log[-1] == "replay"
    for lt in (7, 7):                           # a third signature evicts the least recently used: 6
        stepper.step(mkb(lt, lt), step); step += 1
    assert list(stepper.graphs) == [sig(5), sig(7)] and stepper.stats["evictions"] == 1 and stepper.stats["max_live"] == 2
    stepper.step(mkb(6, 3), step); step += 1    # 6 was seen before: captured again at its next sight, 5 goes
    assert list(stepper.graphs) == [sig(7), sig(6)] and stepper.stats["captures"] == 4 and stepper.log[-1] == "eager"

    # the static buffers after a replay are the batch, bit for bit -- also when a batch of small values follows one of large values
    entry = stepper.graphs[sig(7)]
    large = mkb(7, 21)
    large["visual_inputs"] = torch.full_like(large["visual_inputs"], 255)
    large["text_input_ids"] = torch.full_like(large["text_input_ids"], vocab - 1)
    small = mkb(7, 22)
    small["visual_inputs"] = torch.zeros_like(small["visual_inputs"])
    small["text_input_ids"] = torch.ones_like(small["text_input_ids"])
    small["text_input_mask"] = torch.zeros_like(small["text_input_mask"]); small["text_input_mask"][:, 0] = 1
    for b in (large, small, mkb(7, 23)):
        stepper.step(b, step); step += 1
        assert stepper.log[-1] == "replay" and stepper.graphs[sig(7)] is entry and handed[-1] is entry.static       # the step ran on the static buffers
        assert set(entry.bufs) == {k for k, v in b.items() if torch.is_tensor(v)}
        for k, buf in entry.bufs.items():
            assert buf.data_ptr() != b[k].data_ptr() and buf.dtype == b[k].dtype and torch.equal(buf, b[k]), k
        assert entry.static["n_examples_list"] == b["n_examples_list"]


def test_start_training_with_capture_reaches_the_same_parameters(hw):
    """six optimizer steps over a loader of two signatures: captured (dry on the emulator, hipGraphs on the GPU) against capture=False"""
    vocab = None
    finals, objs = [], []
    for capture in (False, "dry" if hw.name == "emul" else True):
        cfg, _sd, model = build_small("retrieval", RET, torch.float32 if hw.name == "emul" else torch.bfloat16, hw.dev)
        vocab = cfg["vocab_size"]
        opt = optim.FusedAdamW(model.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=5.0)
        tcfg = _tcfg(train_n_clips=1, num_train_steps=6, warmup_ratio=0.5, train_batch_size=1, valid_steps=0)
        one_video = lambda seed: S.synthetic_frames(1, 1, 64, seed).contiguous().to(hw.dev)      # noqa: E731  (one image per step keeps the emulator run short)
        loader = [_text_batch(one_video(31), 2, 6, 31, vocab, hw.dev), _text_batch(one_video(32), 1, 9, 32, vocab, hw.dev)]
        if capture:
            capture = CAP.CapturedStep(model, opt, tcfg, mode="dry" if capture == "dry" else "graph")
            objs.append(capture)
        assert tasks.start_training(model, opt, loader, tcfg, capture=capture) == 6 and opt.step_count == 6
        finals.append(model.rt.bank.master.clone())
    assert objs[0].log == ["eager"] * 4 + ["replay"] * 2 and objs[0].stats["captures"] == 2
    assert float((finals[0] - finals[1]).abs().max()) <= 1e-6 * float(finals[0].abs().max())


def test_start_training_builds_the_stepper_itself(small_cpu, monkeypatch):
    """capture="dry" / True construct the CapturedStep with the loop's own arguments; capture=False never touches the module"""
    s = small_cpu
    built = []

    class Spy(CAP.CapturedStep):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            built.append(self)

    monkeypatch.setattr(CAP, "CapturedStep", Spy)
    monkeypatch.setattr(tasks, "train_step", lambda model, opt, batch, *a, **kw: torch.zeros(()))
    loader = [_text_batch(_small_frames(1), 2, 6, 1, s.cfg["vocab_size"])]
    tcfg = _tcfg(num_train_steps=3)
    fn = lambda m, b, c: None      # noqa: E731
    assert tasks.start_training(s.model, s.opt, loader, tcfg, capture=False) == 3 and not built
    assert tasks.start_training(s.model, s.opt, loader, tcfg, capture="dry", loss_fn=fn, fold_clips=False) == 3
    assert len(built) == 1 and built[0].mode == "dry" and built[0].loss_fn is fn and built[0].fold_clips is False and built[0].log == ["eager", "eager", "replay"]
    mine = CAP.CapturedStep(s.model, s.opt, tcfg, mode="dry", max_graphs=3)
    assert tasks.start_training(s.model, s.opt, loader, tcfg, capture=mine) == 3 and len(built) == 2 and mine.log == ["eager", "eager", "replay"]
    # an object built on other arguments than the loop's is refused, not silently preferred
    for kw in (dict(loss_fn=fn), dict(fold_clips=False), dict(sync=SimpleNamespace(active=False, grad_scale=1.0))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            tasks.start_training(s.model, s.opt, loader, tcfg, capture=mine, **kw)


def test_dry_inference_matches_eager(small_cpu):
    s = small_cpu
    s.model.eval()
    cfg = _tcfg(inference_n_clips=2, num_frm=1, inference_batch_size=2)
    for i in range(3):
        vis = S.synthetic_frames(1, 2, 64, 7 + i).contiguous()
        ids, mask = S.synthetic_text(3, 6, 7 + i, s.cfg["vocab_size"])
        ids = ids.clamp(max=s.cfg["vocab_size"] - 1)
        assert tasks.inference_retrieval_video(s.model, vis, ids, mask, cfg, capture="dry") == tasks.inference_retrieval_video(s.model, vis, ids, mask, cfg)
    cf = s.model._captured_forward
    assert cf.mode == "dry" and cf.stats["captures"] == 2 and cf.log[-2:] == ["replay"] * 2, (cf.stats, cf.log)
