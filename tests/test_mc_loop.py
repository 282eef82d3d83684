"""The MSRVTT multiple-choice test (src/tasks/run_msrvtt_mc.py): tasks.inference_retrieval_mc against the reference's own loop executed
from its source, tasks.mc_accuracy against its evaluate_qa_accuracy, the feature-cached clip loop against the reference's order of
evaluation on a small model, the captured encoder passes against the eager ones, and the collate / gather helpers."""
import functools
import os
import time
from types import SimpleNamespace

import pytest
import torch

import mc_restatement as R
from clipbert_amd import data as D
from clipbert_amd import ops, tasks
from clipbert_amd import synthetic as S
from oracle import clipbert_oracle as O
from oracle import ref_functions, ref_shim
from test_model_small import build, to_dev

live = pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")
MC_RUNNER = os.path.join("src", "tasks", "run_msrvtt_mc.py")
RETRIEVAL_DATASET = os.path.join("src", "datasets", "dataset_video_retrieval.py")
N_OPTIONS = 5
MODES = {"mean": ops.AGG_MEAN, "max": ops.AGG_MAX, "lse": ops.AGG_LSE}


# ---- the reference loop, executed from its source ---------------------------------------------------------------------------------
def _reference_loop():
    quiet = SimpleNamespace(info=lambda *a, **k: None, disabled=False)
    ns = dict(hvd=SimpleNamespace(rank=lambda: 0, size=lambda: 1, local_rank=lambda: 0), LOGGER=quiet, all_gather_list=lambda x: [x],
              tqdm=lambda *a, **k: SimpleNamespace(update=lambda n: None), join=os.path.join, F=torch.nn.functional, time=time)
    fns = ref_functions.load(MC_RUNNER, ["forward_step", "inference_retrieval_mc"], extra_ns=ns)
    return fns["inference_retrieval_mc"]


def _reference_accuracy():
    return ref_functions.load_method(RETRIEVAL_DATASET, "ClipBertMSRVTTMCEvalDataset", "evaluate_qa_accuracy")


class _Replay(torch.nn.Module):
    """a model that replays canned per-clip logits, one (B*n_options, C) tensor per call, and checks what it is called with"""

    def __init__(self, canned, num_frm):
        super().__init__()
        self.canned, self.num_frm, self.calls = canned, num_frm, 0

    def forward(self, batch):
        logits = self.canned[self.calls]
        self.calls += 1
        bsz = logits.shape[0] // N_OPTIONS
        assert list(batch["n_examples_list"]) == [N_OPTIONS] * bsz
        assert tuple(batch["visual_inputs"].shape[:2]) == (bsz, self.num_frm) and batch["text_input_ids"].shape[0] == bsz * N_OPTIONS
        return dict(logits=logits.clone())


class _Loader:
    """fresh copies per pass: the reference's loop deletes and rewrites entries of the batch it is given"""

    def __init__(self, batches, dataset=None):
        self.batches, self.dataset = batches, dataset

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for b in self.batches:
            yield {k: (list(v) if isinstance(v, list) else v) for k, v in b.items()}


def _canned_batches(c, n_clips, num_frm, seed):
    """two batches (2 videos + 1 video = three question ids) and their canned (n_clips, B*5, C) logits"""
    g = torch.Generator().manual_seed(seed)
    batches, stacks = [], []
    for qids in (["q7", "q3"], ["q11"]):
        bsz = len(qids)
        stacks.append(torch.randn(n_clips, bsz * N_OPTIONS, c, generator=g) * 1.5)
        batches.append(D.collate_mc(torch.zeros(bsz, n_clips * num_frm, 3, 4, 4), torch.ones(bsz, N_OPTIONS, 6, dtype=torch.long),
                                    torch.ones(bsz, N_OPTIONS, 6, dtype=torch.long), qids))
    return batches, stacks


@live
@pytest.mark.parametrize("pool", list(MODES))
@pytest.mark.parametrize("c", [2, 1])
def test_loop_matches_the_reference_loop_run_from_source(emul, tmp_path, c, pool):
    n_clips, num_frm = 3, 2
    batches, stacks = _canned_batches(c, n_clips, num_frm, seed=17 + c)
    for st in stacks:                                        # a decided answer for every question: margin > 2x the kernel's bound
        margin = float(R.top2_margin(R.mc_scores(st, N_OPTIONS, pool)[0], N_OPTIONS).min())
        assert margin > 2 * R.score_bound(st), (margin, R.score_bound(st))
    canned = [clip for st in stacks for clip in st.unbind(0)]
    cfg = SimpleNamespace(score_agg_func=pool, inference_n_clips=n_clips, num_frm=num_frm, output_dir=str(tmp_path))
    ref_model = _Replay(canned, num_frm)
    # the reference decides what is right: its predictions with one of them flipped are the ground truth (accuracy 2 of 3)
    probe = _Loader(batches, SimpleNamespace(evaluate_qa_accuracy=lambda pred, force_same=True: None))
    with torch.no_grad():
        ref_pred, _ = _reference_loop()(ref_model, probe, "probe.json", cfg, n_options=N_OPTIONS)
    id2answer = dict(ref_pred)
    id2answer["q3"] = (id2answer["q3"] + 1) % N_OPTIONS
    acc = _reference_accuracy()
    dataset = SimpleNamespace(id2answer=id2answer)
    dataset.evaluate_qa_accuracy = lambda pred, force_same=True: acc(dataset, pred, force_same=force_same)
    ref_model = _Replay(canned, num_frm)
    with torch.no_grad():
        want_pred, want_metrics = _reference_loop()(ref_model, _Loader(batches, dataset), "val.json", cfg, n_options=N_OPTIONS)
    assert ref_model.calls == len(canned) and want_metrics == dict(mc_accuracy="66.67")
    for was_training in (True, False):
        model = _Replay(canned, num_frm).train(was_training)
        got_pred, got_metrics = tasks.inference_retrieval_mc(model, _Loader(batches), cfg, n_options=N_OPTIONS, cache_cnn=False,
                                                             id2answer=id2answer)
        assert model.calls == len(canned) and model.training is was_training
        assert got_pred == want_pred and list(got_pred) == ["q7", "q3", "q11"] and all(type(v) is int for v in got_pred.values())
        assert got_metrics == want_metrics
    assert tasks.inference_retrieval_mc(_Replay(canned, num_frm), _Loader(batches), cfg, cache_cnn=False)[1] is None
    with pytest.raises(ValueError):
        tasks.inference_retrieval_mc(_Replay(canned, num_frm), _Loader(batches), cfg, cache_cnn=False, capture=True)
    with pytest.raises(ValueError, match="score_agg_func"):
        tasks.inference_retrieval_mc(_Replay(canned, num_frm), _Loader(batches), SimpleNamespace(**dict(vars(cfg), score_agg_func="median")),
                                     cache_cnn=False)


@live
def test_mc_accuracy_matches_evaluate_qa_accuracy():
    acc = _reference_accuracy()
    id2answer = {"a": 0, "b": 4, "c": 2, "d": 2, 5: 1, 6: 3, 7: 0}
    dataset = SimpleNamespace(id2answer=id2answer)
    for wrong in ((), ("b",), ("a", "c", 5), tuple(id2answer)):
        pred = {k: (v + 1) % N_OPTIONS if k in wrong else v for k, v in id2answer.items()}
        assert tasks.mc_accuracy(pred, id2answer) == acc(dataset, pred) == dict(mc_accuracy=f"{100 * (7 - len(wrong)) / 7:.2f}")
    part = {"c": 2, "a": 1, 6: 3}                           # fewer predictions than questions
    assert tasks.mc_accuracy(part, id2answer, force_same=False) == acc(dataset, part, force_same=False) == dict(mc_accuracy="66.67")
    for fn in (lambda: tasks.mc_accuracy(part, id2answer), lambda: acc(dataset, part, force_same=True),
               lambda: tasks.mc_accuracy(dict(part, zz=0), id2answer, force_same=True)):
        with pytest.raises(AssertionError):
            fn()


# ---- the small model --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small(c, dtype, dev):
    """(cfg, state dict, model in eval mode) per (num_labels, dtype, device): built once, only ever run forward"""
    cfg, sd, model = build("retrieval", dict(num_labels=c, loss_type="ce", margin=0.1), dtype, torch.device(dev))
    model.eval()
    return cfg, sd, model


def _mc_batch(cfg, bsz, n_frames, lt, seed, wide=True):
    f = S.synthetic_frames(bsz, n_frames, 64, seed)                                                          # (B, n, 3, 64, 64)
    if wide:
        f = f[..., :64, :].repeat(1, 1, 1, 1, 2).contiguous()                                                # (B, n, 3, 64, 128)
    ids, mask = S.synthetic_text(bsz * N_OPTIONS, lt, seed, cfg["vocab_size"])
    return D.collate_mc(O.image_norm(f, S.PIXEL_MEAN, S.PIXEL_STD), ids.clamp(max=cfg["vocab_size"] - 1), mask,
                        [f"q{seed}_{i}" for i in range(bsz)])


@pytest.mark.parametrize("c,pool", [(2, "lse"), (1, "mean")])
def test_cached_clip_loop_equals_the_reference_order(hw, c, pool):
    """3 videos x 2 clips x 2 frames, 5 options, fp32: the stack of cache_cnn=True -- 6 (clip, video) blocks in encoder passes of 2
    (max_pairs_per_pass=10) and of 4 + a remainder of 2 (20: a pass that runs across the clip boundary) -- gives the scores of the
    reference's order of evaluation within 1.01e-4 (the bound tests/test_tasks.py holds the retrieval loop's same comparison to) and the
    same predictions.  The synthetic model barely separates the options; the oracle's float64 top-2 margins (printed) are asserted to be
    at least 1e-5."""
    cfg, sd, model = _small(c, torch.float32, str(hw.dev))
    icfg = SimpleNamespace(inference_n_clips=2, num_frm=2, score_agg_func=pool)
    batch = _mc_batch(cfg, 3, 4, 6, seed=11)
    vis = batch["visual_inputs"].view(3, 2, 2, *batch["visual_inputs"].shape[2:])
    with torch.no_grad():
        oracle = torch.stack([O.clipbert_forward(sd, dict(visual_inputs=vis[:, k], text_input_ids=batch["text_input_ids"],
                                                          text_input_mask=batch["text_input_mask"], n_examples_list=[N_OPTIONS] * 3),
                                                 cfg, "retrieval")["logits"].float() for k in range(2)])
    o_scores, o_pred = R.mc_scores(oracle, N_OPTIONS, pool)
    margins = R.top2_margin(o_scores, N_OPTIONS)
    print(f"oracle top-2 margins: {[f'{m:.2e}' for m in margins.tolist()]}")
    assert float(margins.min()) >= 1e-5
    dev_batch = to_dev(batch, hw.dev)
    slow = tasks.mc_clip_logits(model, dict(dev_batch), icfg, cache_cnn=False)
    assert tuple(slow.shape) == (2, 15, c) and slow.dtype == torch.float32
    s_scores, s_pred = ops.mc_predict(slow, N_OPTIONS, MODES[pool])
    fast = tasks.mc_clip_logits(model, dict(dev_batch), icfg, cache_cnn=True, max_pairs_per_pass=10)
    assert tuple(fast.shape) == (2, 15, c) and fast.dtype == torch.float32
    f_scores, f_pred = ops.mc_predict(fast, N_OPTIONS, MODES[pool])
    b_pred, b_scores = tasks.mc_predict_batch(model, dict(dev_batch), icfg, max_pairs_per_pass=20)       # (every (CNN) pass costs the emulator seconds)
    assert b_pred.device == slow.device and b_scores.device == slow.device
    for pairs, scores, pred in ((10, f_scores, f_pred), (20, b_scores, b_pred)):
        diff = float((scores - s_scores).abs().max())
        print(f"max_pairs_per_pass {pairs}: max |score(cached) - score(per clip)| = {diff:.3e}")
        assert diff <= 1.01e-4
        assert torch.equal(pred, s_pred)
    print(f"predictions: oracle {o_pred.tolist()}, model {s_pred.cpu().tolist()}")
    with pytest.raises(ValueError):
        tasks.mc_clip_logits(model, dict(dev_batch, n_examples_list=[1, 2, 1]), icfg)


@pytest.mark.gpu
@pytest.mark.parametrize("c,pool", [(2, "lse"), (1, "max"), (2, "mean")])
def test_bf16_stack_meets_the_kernel_bound(c, pool):
    """bf16 model: the options' margins lie below bf16 resolution, so nothing is asserted across paths; the model's own fp32 stack goes
    through the kernel and through the restatement"""
    dev = torch.device("cuda", 0)
    cfg, sd, model = _small(c, torch.bfloat16, str(dev))
    icfg = SimpleNamespace(inference_n_clips=2, num_frm=2, score_agg_func=pool)
    stack = tasks.mc_clip_logits(model, to_dev(_mc_batch(cfg, 3, 4, 6, seed=11), dev), icfg, max_pairs_per_pass=10)
    assert tuple(stack.shape) == (2, 15, c) and stack.dtype == torch.float32
    scores, pred = ops.mc_predict(stack, N_OPTIONS, MODES[pool])
    ref_scores, _ = R.mc_scores(stack, N_OPTIONS, pool)
    err = float((scores.cpu().double() - ref_scores).abs().max())
    print(f"bf16 stack, C {c}, {pool}: max |score - float64| = {err:.3e}, bound {R.score_bound(stack):.3e}")
    assert err <= R.score_bound(stack)
    assert torch.equal(pred.cpu().long(), scores.cpu().view(-1, N_OPTIONS).max(1)[1])


def test_captured_encoder_passes_equal_eager(hw):
    """batches of one signature, one encoder pass over all blocks but one + a remainder of 1 (two signatures of the CapturedForward): on the emulator
    capture="dry" -- the bookkeeping without graphs --, on the GPU hipGraph replays; the stack is bit-equal to the eager one on every
    batch, replays included, and the whole loop returns the eager loop's predictions"""
    gpu = hw.name == "gpu"
    cfg, sd, model = _small(2, torch.bfloat16 if gpu else torch.float32, str(hw.dev))
    capture = True if gpu else "dry"
    n_batches, bsz = (4, 3) if gpu else (3, 2)
    icfg = SimpleNamespace(inference_n_clips=2, num_frm=1, score_agg_func="lse")
    batches = [to_dev(_mc_batch(cfg, bsz, 2, 6, seed=50 + i, wide=gpu), hw.dev) for i in range(n_batches)]
    pairs = (2 * bsz - 1) * N_OPTIONS                       # all (clip, video) blocks but one in the full pass
    assert getattr(model, "_captured_forward", None) is None
    try:
        for b in batches:
            want = tasks.mc_clip_logits(model, dict(b), icfg, max_pairs_per_pass=pairs)
            got = tasks.mc_clip_logits(model, dict(b), icfg, max_pairs_per_pass=pairs, capture=capture)
            assert torch.equal(got, want)
        cf = model._captured_forward
        assert cf.mode == ("graph" if gpu else "dry") and cf.stats["captures"] == 2 and cf.stats["failed_captures"] == 0, cf.stats
        assert cf.log == ["eager"] * 4 + ["replay"] * (2 * n_batches - 4), cf.log
        loop = batches if gpu else batches[:2]               # (every pass costs the emulator seconds)
        want_pred, _ = tasks.inference_retrieval_mc(model, loop, icfg)
        got_pred, _ = tasks.inference_retrieval_mc(model, loop, icfg, capture=capture)
        assert got_pred == want_pred and len(got_pred) == len(loop) * bsz
        # (the loop's default of 256 pairs: one pass per batch, a third signature -- seen twice, then replayed)
        assert cf.stats["captures"] == 3 and cf.log[-len(loop):] == ["eager"] * 2 + ["replay"] * (len(loop) - 2), cf.log
        with pytest.raises(ValueError):
            tasks.mc_clip_logits(model, dict(batches[0]), icfg, cache_cnn=False, capture=capture)
    finally:
        model._captured_forward = None


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def test_gather_mc_predictions_single_process():
    pred = {"q1": 3, 7: 0}
    assert tasks.gather_mc_predictions(pred) is pred


def test_collate_mc():
    videos = [torch.full((4, 3, 8, 8), float(i)) for i in range(3)]
    ids = [torch.arange(N_OPTIONS * 6).view(N_OPTIONS, 6) + 100 * i for i in range(3)]
    mask = [torch.ones(N_OPTIONS, 6, dtype=torch.long) for _ in range(3)]
    b = D.collate_mc(videos, ids, mask, ["a", "b", "c"])
    assert set(b) == {"visual_inputs", "text_input_ids", "text_input_mask", "question_ids", "labels", "n_examples_list"}
    assert tuple(b["visual_inputs"].shape) == (3, 4, 3, 8, 8) and tuple(b["text_input_ids"].shape) == tuple(b["text_input_mask"].shape) == (15, 6)
    assert b["n_examples_list"] == [1, 1, 1] and b["question_ids"] == ["a", "b", "c"] and b["labels"] is None
    assert torch.equal(b["text_input_ids"][5:10], ids[1]) and float(b["visual_inputs"][2].max()) == 2.0      # video v's options: rows 5v ..
    b2 = D.collate_mc(torch.stack(videos), torch.stack(ids), torch.stack(mask).view(15, 6), ["a", "b", "c"], answers=[4, 0, 2])
    assert torch.equal(b2["text_input_ids"], b["text_input_ids"]) and b2["answers"] == [4, 0, 2]
    assert dict(zip(b2["question_ids"], b2["answers"])) == {"a": 4, "b": 0, "c": 2}
    with pytest.raises(ValueError):
        D.collate_mc(videos, ids, mask, ["a", "b"])
    with pytest.raises(ValueError):
        D.collate_mc(videos, ids, mask, ["a", "b", "c"], answers=[1])
