"""Pixel sub-sampling drawn on the device: cb_pixel_sample / ops.pixel_sample against its NumPy restatement (exact), its argument
checks, the uniformity of the selections a replayed graph would draw, the model in ``pixel_sampling="device"`` mode against the CPU
oracle on the restated index, the host logic around it (config, CapturedStep._why_eager, signature), and -- on the GPU -- a captured
pretraining loop with sub-sampling on: replays against eager steps, selections against the restatement, fresh selections per replay."""
import itertools
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dropout_restatement as DR
import pixel_sample_restatement as PR
from clipbert_amd import captured as CAP
from clipbert_amd import config as CFG
from clipbert_amd import ops, optim, tasks
from clipbert_amd.modeling import runtime as RT
from oracle import clipbert_oracle as O
from test_captured_loop import NO_DROP, _assert_same_step, _both, _restore, _small_frames, _snapshot, _tcfg, _text_batch
from test_captured_loop import build_small
from test_model_small import make_batch, to_dev

SENTINEL = -7
SHAPES = [(2, 1), (4, 2), (12, 5), (64, 63), (65, 1), (144, 100), (256, 255), (257, 129), (1025, 100), (10000, 100), (10000, 9999),
          (65536, 3), (7, 7)]
# (host seed, device word or None): no seed_ptr; the model's site at forward 3 under word 5; the wrap-around of the 64-bit sum
SEEDS = [(0, None), (RT._seed(RT._SITE_PIXEL, 0, 3), 5), ((1 << 64) - 1, 5)]


def _draw(hw, lv, n, seed, word):
    """-> (the n + 8 long output buffer after the launch, the restated selection)"""
    buf = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device=hw.dev)
    ptr = None if word is None else torch.tensor([word], dtype=torch.int64, device=hw.dev)
    got = ops.pixel_sample(lv, n, seed, ptr, out=buf)
    assert got.data_ptr() == buf.data_ptr() and got.shape == (n,)
    return buf.cpu().numpy(), PR.sample(DR.effective_seed(seed, word or 0), lv, n)


# ---- the kernel against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lv,n", SHAPES)
def test_kernel_equals_the_restatement(hw, lv, n):
    for seed, word in SEEDS:
        got, want = _draw(hw, lv, n, seed, word)
        sel, tail = got[:n], got[n:]
        assert (tail == SENTINEL).all(), (seed, word, tail)
        assert sel.min() >= 0 and sel.max() < lv and (np.diff(sel) > 0).all(), (seed, word)
        assert np.array_equal(sel, want), (seed, word, sel[:8], want[:8])
        if n == lv:
            assert np.array_equal(sel, np.arange(lv))


def test_allocates_its_output_next_to_the_seed_word(hw):
    word = torch.tensor([9], dtype=torch.int64, device=hw.dev)
    got = ops.pixel_sample(12, 5, 3, word)
    assert got.dtype == torch.int32 and got.shape == (5,) and got.device == word.device
    assert np.array_equal(got.cpu().numpy(), PR.sample(12, 12, 5))
    assert np.array_equal(ops.pixel_sample(12, 5, 12, device=hw.dev).cpu().numpy(), PR.sample(12, 12, 5))
    with pytest.raises(ValueError):
        ops.pixel_sample(12, 5, 3)


@pytest.mark.parametrize("lv,n", [(12, 0), (12, 13), (65537, 5)])
def test_argument_errors_launch_nothing(hw, lv, n):
    buf = torch.full((32,), SENTINEL, dtype=torch.int32, device=hw.dev)
    with pytest.raises(RuntimeError, match="cb_pixel_sample"):
        ops.pixel_sample(lv, n, 1, out=buf)
    if buf.is_cuda:
        torch.cuda.synchronize()
    assert (buf.cpu() == SENTINEL).all()


def test_null_output_is_refused(hw):
    from clipbert_amd import _lib
    assert _lib.get().cb_pixel_sample(None, 12, 5, 0, None, None) != 0
    assert b"cb_pixel_sample" in _lib.get().cb_last_error()
    assert _lib.get().cb_version() >= 15 and "cb_pixel_sample" in _lib.EXPORTED_SYMBOLS


# ---- uniformity ---------------------------------------------------------------------------------------------------------------------------
def test_selections_are_uniform_over_the_seed_words_of_replays(hw):
    """Lv = 12, n = 5, the model's seed at forward 0, device words 0..1999 (what 2000 replays of one graph hash with).  The bounds are
    binomial: 5 sigma around the expectation of a uniformly random 5-subset, for every index and every pair; the restatement itself
    sits at 1.65 and 3.12 sigma on exactly these inputs and draws 741 of the 792 possible sets."""
    lv, n, T = 12, 5, 2000
    seed = RT._seed(RT._SITE_PIXEL, 0, 0)
    word = torch.zeros(1, dtype=torch.int64, device=hw.dev)
    buf = torch.full((T, n), SENTINEL, dtype=torch.int32, device=hw.dev)
    for t in range(T):
        ops.pixel_sample(lv, n, seed, word, out=buf[t])
        ops.counter_add(word)
    got = buf.cpu().numpy()                                                    # the one read-back
    assert int(word.item()) == T
    want = np.stack([PR.sample(DR.effective_seed(seed, t), lv, n) for t in range(T)])
    assert np.array_equal(got, want)
    member = np.zeros((T, lv), dtype=np.int64)
    np.put_along_axis(member, got.astype(np.int64), 1, axis=1)
    assert (member.sum(1) == n).all()
    p1 = n / lv
    dev1 = np.abs(member.sum(0) - T * p1) / np.sqrt(T * p1 * (1 - p1))
    p2 = n * (n - 1) / (lv * (lv - 1))
    pairs = member.T @ member
    dev2 = np.array([abs(pairs[i, j] - T * p2) for i, j in itertools.combinations(range(lv), 2)]) / np.sqrt(T * p2 * (1 - p2))
    distinct = len({tuple(r) for r in got})
    print(f"[pixel_sample uniformity] worst index {dev1.max():.2f} sigma, worst pair {dev2.max():.2f} sigma, {distinct} distinct sets of 792")
    assert dev1.max() <= 5.0, dev1
    assert dev2.max() <= 5.0, dev2.max()
    assert distinct >= 700, distinct


# ---- the model in device mode ---------------------------------------------------------------------------------------------------------
class _Spy:
    """records every ops.pixel_sample call of the model: (lv, n, the returned tensor)"""

    def __init__(self, monkeypatch):
        self.calls, real = [], ops.pixel_sample

        def spy(lv, n, *a, **kw):
            out = real(lv, n, *a, **kw)
            self.calls.append((lv, n, out))
            return out

        monkeypatch.setattr(ops, "pixel_sample", spy)


def _pretraining_case(hw, extra):
    from test_model_small import build
    from clipbert_amd import synthetic as S
    cfg, sd, model = build("pretraining", dict(extra, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), torch.float32, hw.dev)
    batch = make_batch(cfg, "pretraining", 2, 1, 6)
    mlm = batch["text_input_ids"].clone()
    mlm[:, ::2] = -100
    batch["mlm_labels"] = mlm
    batch["itm_labels"] = S.synthetic_labels(2, 2, 5)
    return cfg, sd, model, batch


def test_pretraining_device_sampling_train_mode(hw, monkeypatch):
    """the twin of test_model_small.test_pretraining_pixel_random_sampling_train_mode: the index is restated from the runtime's seed
    state instead of drawn from numpy; forward AND gradients against the oracle under that test's tolerances"""
    cfg, sd, model, batch = _pretraining_case(hw, dict(pixel_random_sampling_size=1, pixel_sampling="device"))
    model.train()
    rt = model.rt
    sdr = {k: v.clone().requires_grad_(v.is_floating_point() and "norm" not in k) for k, v in sd.items()}
    sdr["transformer.cls.predictions.decoder.weight"] = sdr["transformer.bert.embeddings.word_embeddings.weight"]
    sdr["transformer.cls.predictions.decoder.bias"] = sdr["transformer.cls.predictions.bias"]
    grid = O.grid_feat_backbone(sdr, batch["visual_inputs"], "cnn.")
    lv = grid.shape[2] * grid.shape[3]
    assert lv == 2
    # a seed word under which this forward and the next one keep different pixels (a condition on the inputs, from the restatement)
    fwd0 = rt.forward_count
    word = next(w for w in range(64) if not np.array_equal(PR.site_sample(fwd0, w, lv, 1), PR.site_sample(fwd0 + 1, w, lv, 1)))
    rt.seed_dev.fill_(word)
    assert int(rt.seed_dev.item()) == word
    idx = torch.from_numpy(PR.site_sample(fwd0, word, lv, 1)).long()
    ref = O.pretraining_forward(sdr, batch["text_input_ids"], grid, batch["text_input_mask"], cfg, batch["mlm_labels"], batch["itm_labels"],
                                sample_idx=idx)
    (ref["mlm_loss"].mean() + ref["itm_loss"].mean()).backward()
    spy = _Spy(monkeypatch)
    np.random.seed(7)
    state = np.random.get_state()
    model.rt.bank.zero_grad()
    gb = lambda: to_dev(dict(batch, n_examples_list=[1, 1]), hw.dev)      # noqa: E731  (forward() consumes its batch dict)
    out = model(gb())
    assert rt.forward_count == fwd0 + 1                                     # (dropout is off: the selection alone advances the counter)
    assert len(spy.calls) == 1 and spy.calls[0][:2] == (lv, 1) and torch.equal(spy.calls[0][2].cpu().long(), idx)
    tol = dict(rtol=1e-3, atol=1e-4) if hw.name == "emul" else dict(rtol=2e-3, atol=1e-3)
    torch.testing.assert_close(out["itm_scores"].cpu(), ref["itm_scores"].detach(), **tol)
    torch.testing.assert_close(out["mlm_loss"].cpu(), ref["mlm_loss"].detach(), **tol)
    (out["mlm_loss"].mean() + out["itm_loss"].mean()).backward()
    for name in ("transformer.bert.visual_embeddings.row_position_embeddings.weight", "cnn.grid_encoder.0.weight",
                 "transformer.bert.encoder.layer.0.attention.self.query.weight"):
        p = dict(model.named_parameters())[name]
        g_ref = sdr[name].grad
        diff = (p.grad.cpu() - g_ref).norm() / max(g_ref.norm().item(), 1e-8)
        assert diff < (2e-3 if hw.name == "emul" else 5e-3), (name, float(diff))
    # the second forward: the restatement at fwd_i + 1 -- the other pixel
    with torch.no_grad():
        idx2 = torch.from_numpy(PR.site_sample(fwd0 + 1, word, lv, 1)).long()
        assert not torch.equal(idx, idx2)
        ref2 = O.pretraining_forward(sd, batch["text_input_ids"], grid.detach(), batch["text_input_mask"], cfg, batch["mlm_labels"],
                                     batch["itm_labels"], sample_idx=idx2)
        out2 = model(gb())
    assert rt.forward_count == fwd0 + 2 and len(spy.calls) == 2 and torch.equal(spy.calls[1][2].cpu().long(), idx2)
    torch.testing.assert_close(out2["itm_scores"].cpu(), ref2["itm_scores"], **tol)
    # evaluation: nothing drawn, nothing advanced, every token used
    model.eval()
    with torch.no_grad():
        ref3 = O.pretraining_forward(sd, batch["text_input_ids"], grid.detach(), batch["text_input_mask"], cfg, batch["mlm_labels"],
                                     batch["itm_labels"], sample_idx=None)
        out3 = model(gb())
    assert rt.forward_count == fwd0 + 2 and len(spy.calls) == 2
    torch.testing.assert_close(out3["itm_scores"].cpu(), ref3["itm_scores"], **tol)
    assert int(rt.seed_dev.item()) == word                                  # (only a captured step advances the word)
    # numpy's global generator was neither read nor advanced by any of it
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    # an unknown mode is refused, in training and in evaluation alike
    model.config.pixel_sampling = "gpu"
    for training in (False, True):
        model.train(training)
        with pytest.raises(ValueError, match="pixel_sampling"):
            model(gb())


def test_host_mode_is_the_default_and_leaves_the_counter_alone(hw, monkeypatch):
    """without the key the selection comes from numpy as before: no device draw, no counter advance with dropout off"""
    cfg, sd, model, batch = _pretraining_case(hw, dict(pixel_random_sampling_size=1))
    model.train()
    spy = _Spy(monkeypatch)
    np.random.seed(7)
    want = np.sort(np.random.choice(2, size=1, replace=False))
    after = np.random.get_state()
    np.random.seed(7)
    fwd0 = model.rt.forward_count
    with torch.no_grad():
        model(to_dev(dict(batch, n_examples_list=[1, 1]), hw.dev))
    now = np.random.get_state()
    assert not spy.calls and model.rt.forward_count == fwd0 and want.shape == (1,)
    assert np.array_equal(now[1], after[1]) and now[2] == after[2]          # numpy advanced exactly as one choice() does


# ---- host logic ---------------------------------------------------------------------------------------------------------------------------
def _stub_model(**enc):
    cfg = SimpleNamespace(**enc)
    return SimpleNamespace(training=True, config=cfg, transformer=SimpleNamespace(bert=SimpleNamespace(config=cfg)),
                           rt=SimpleNamespace(bank=SimpleNamespace(device=torch.device("cpu"))))


def test_why_eager_and_signature_follow_the_mode():
    batch = dict(visual_inputs=torch.zeros(1, 2, 3, 8, 8, dtype=torch.uint8), text_input_ids=torch.zeros(1, 4, dtype=torch.long),
                 text_input_mask=torch.ones(1, 4, dtype=torch.long), n_examples_list=[1])
    mk = lambda **enc: CAP.CapturedStep(_stub_model(**enc), None, _tcfg(), mode="dry")      # noqa: E731
    host, dev = mk(pixel_random_sampling_size=100, pixel_sampling="host"), mk(pixel_random_sampling_size=100, pixel_sampling="device")
    unset = mk(pixel_random_sampling_size=100)
    assert dev._why_eager(batch) is None
    for s in (host, unset):
        assert "pixel_random_sampling_size" in s._why_eager(batch)
    assert host.signature(batch) != dev.signature(batch) and host.signature(batch) == unset.signature(batch)
    assert dev.signature(batch) != mk(pixel_random_sampling_size=50, pixel_sampling="device").signature(batch)
    assert mk(pixel_random_sampling_size=0)._why_eager(batch) is None
    dev.model.training = False                                               # evaluation never samples
    host.model.training = False
    assert host._why_eager(batch) is None and dev._why_eager(batch) is None


def test_config_carries_the_mode_into_the_model_config():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_configs")
    path = os.path.join(root, "src", "configs", "pretrain_image_text_base_resnet50_mlm_itm.json")
    cfg = CFG.load_task_config(path, task="pretraining")
    assert cfg.pixel_sampling == "host" and cfg.pixel_random_sampling_size == 100
    mc = CFG.build_model_config(cfg, config_root=root)
    assert mc.pixel_sampling == "host" and mc.pixel_random_sampling_size == 100
    cfg = CFG.load_task_config(path, task="pretraining", pixel_sampling="device")
    mc = CFG.build_model_config(cfg, config_root=root)
    assert mc.pixel_sampling == "device" and mc.pixel_random_sampling_size == 100
    assert "pixel_sampling" not in CFG.load_task_config(os.path.join(root, "src", "configs", "msrvtt_ret_base_resnet50.json"))


# ---- captured pretraining with sub-sampling on ------------------------------------------------------------------------------------------
def _pretrain_batches_128(s, n):
    """test_captured_loop._pretrain_batches on 128 px frames (a 2 x 2 grid)"""
    out = []
    for i in range(n):
        b = _text_batch(_small_frames(90 + i, size=128, dev=s.dev), 1, 6, 90 + i, s.cfg["vocab_size"], s.dev)
        del b["labels"]
        g = torch.Generator().manual_seed(90 + i)
        mlm = torch.full((2, 6), -100, dtype=torch.long)
        mlm[0, 1 + i % 3] = int(torch.randint(1, s.cfg["vocab_size"], (1,), generator=g))
        mlm[1, 2] = int(torch.randint(1, s.cfg["vocab_size"], (1,), generator=g))
        out.append(dict(b, mlm_labels=mlm.to(s.dev), itm_labels=torch.tensor([1, 0]).to(s.dev)))
    return out


@pytest.mark.gpu
def test_pretraining_with_device_sampling_is_captured_and_draws_fresh_selections(monkeypatch):
    dev = torch.device("cuda", 0)
    cfg, _sd, model = build_small("pretraining", dict(NO_DROP, pixel_random_sampling_size=2, pixel_sampling="device"), torch.bfloat16, dev)
    model.train(True)
    opt = optim.FusedAdamW(model.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=5.0)
    s = SimpleNamespace(cfg=cfg, model=model, opt=opt, dev=dev)
    rt = model.rt
    batches = _pretrain_batches_128(s, 5)
    tcfg = _tcfg(train_n_clips=1, num_frm=2, mlm_rows="labelled", mlm_capacity=64)
    loss_fn = tasks.pretrain_loss
    lv, n = 4, 2
    # eager steps leave the seed word alone, every replay adds one: the three replays hash with fwd_cap and w0, w0 + 1, w0 + 2.  fwd_cap is
    # the counter the capture (second sight) sees: one eager forward after now.  w0: the first word under which replays 1 and 2 differ.
    fwd_cap = rt.forward_count + 1
    w0 = next(w for w in range(64) if not np.array_equal(PR.site_sample(fwd_cap, w, lv, n), PR.site_sample(fwd_cap, w + 1, lv, n)))
    rt.seed_dev.fill_(w0)
    spy = _Spy(monkeypatch)
    stepper = CAP.CapturedStep(model, opt, tcfg, loss_fn=loss_fn)
    state = {}

    def run_captured(b, k):
        state["capturing_at"] = len(spy.calls)
        loss = stepper.step(b, k)
        torch.cuda.synchronize()
        state["word"] = int(rt.seed_dev.item())
        if k == 1:                                                           # the capture's own call comes first: its output tensor is the graph's
            state["graph_sel"] = spy.calls[state["capturing_at"]][2]
        if k >= 2:                                                           # (a replay calls nothing)
            assert len(spy.calls) == state["capturing_at"]
            state["sel"] = state["graph_sel"].cpu().numpy().copy()
        return loss

    def run_eager(b, k, replay):
        if replay:                                                           # the graph's host half of the seed is frozen at the capture's count
            rt.forward_count = fwd_cap
        return tasks.train_step(model, opt, b, tcfg, k, loss_fn=loss_fn)

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for k, b in enumerate(batches):
            replay = k >= 2
            fwd_before, word_before = rt.forward_count, int(rt.seed_dev.item())
            got, want = _both(model, opt, lambda: run_captured(b, k), lambda: run_eager(b, k, replay))
            _assert_same_step(model, got, want, f"device-sampled pretraining step {k}")
            if k == 1:
                assert fwd_before == fwd_cap
            if replay:
                assert state["word"] == word_before + 1 and word_before == w0 + (k - 2)
                assert np.array_equal(state["sel"], PR.site_sample(fwd_cap, word_before, lv, n)), (k, state["sel"])
                rt.forward_count = fwd_before                                # (the twin counted from fwd_cap)
                rt.seed_dev.fill_(state["word"])                             # and the word goes on from where the replay left it
    assert not [w for w in caught if "runs eagerly" in str(w.message)], [str(w.message) for w in caught]
    assert stepper.log == ["eager", "eager", "replay", "replay", "replay"], stepper.log
    assert stepper.stats["fallbacks"] == 0 and stepper.stats["captures"] == 1, stepper.stats
    assert spy.calls and all(c[:2] == (lv, n) for c in spy.calls), [c[:2] for c in spy.calls]      # the grid has 4 cells, 2 are kept

    # from identical weights, replays under w0 and w0 + 1: the graph's own selection buffer against the restatement, and other gradients
    snap = _snapshot(model, opt)
    graph_sel = state["graph_sel"]
    rt.seed_dev.fill_(w0)
    grads, sels = [], []
    for i in range(2):
        _restore(model, opt, dict(snap, seed=rt.seed_dev.clone()))          # the same weights and moments; the seed word keeps counting
        loss = stepper.step(batches[0], 5)
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and int(rt.seed_dev.item()) == w0 + i + 1
        grads.append(rt.bank.grad.clone())
        sels.append(graph_sel.cpu().numpy().copy())
        assert np.array_equal(sels[-1], PR.site_sample(fwd_cap, w0 + i, lv, n)), (i, sels[-1])
    assert stepper.log[-2:] == ["replay"] * 2 and not np.array_equal(sels[0], sels[1])
    diff = float((grads[0] - grads[1]).abs().max())
    assert diff > 1e-3 * float(grads[0].abs().max()), diff                  # other pixels, other gradients
