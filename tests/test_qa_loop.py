"""The video-QA validation loop (src/tasks/run_video_qa.py:216-362): tasks.validate_video_qa against the reference's validate +
forward_step and evaluate_tgif_qa executed from their source over the oracle model, the feature-cached clip loop against the reference's
order of evaluation, the captured encoder passes against the eager ones, the additive counters, and the collate helper."""
import functools
import os
import time
from types import SimpleNamespace

import pytest
import torch

import qa_restatement as R
from clipbert_amd import data as D
from clipbert_amd import ops, tasks
from clipbert_amd import synthetic as S
from oracle import clipbert_oracle as O
from oracle import ref_functions, ref_shim
from test_model_small import build, to_dev

live = pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")
QA_RUNNER = os.path.join("src", "tasks", "run_video_qa.py")
QA_DATASET = os.path.join("src", "datasets", "dataset_video_qa.py")
MODES = {"mean": ops.AGG_MEAN, "max": ops.AGG_MAX, "lse": ops.AGG_LSE}
N_CLIPS, NUM_FRM, LT = 2, 2, 6
# task -> (head, its config, classes of the stack, text rows per video)
TASKS = dict(action=("multiple_choice", dict(num_labels=5, loss_type="ce"), 5, 5),
             frameqa=("sequence_classification", dict(num_labels=24, loss_type="ce"), 24, 1),
             count=("regression", dict(num_labels=1, loss_type="mse", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), 1, 1))
# (question ids, seed) per batch.  count: two videos in every batch -- the reference's preds.data.squeeze().tolist() (:279) turns the answer
# of a one-question batch into a bare int that its zip() cannot walk
_QIDS = {False: ((["q7", "q3"], 31), (["q11"], 32)), True: ((["q7", "q3"], 31), (["q11", "q5"], 32))}
FRAMEQA_TYPES = ["object", "color", "number"]               # of the three questions; no "location" question: an empty answer type


def _qcfg(task, pool="mean", **kw):
    return SimpleNamespace(task=task, score_agg_func=pool, inference_n_clips=N_CLIPS, num_frm=NUM_FRM, num_labels=TASKS[task][1]["num_labels"],
                           debug=False, **kw)


# ---- the reference, executed from its source ----------------------------------------------------------------------------------------
def _reference_validate(val_log):
    """validate of the reference with its forward_step; what it hands to TB_LOGGER lands in ``val_log``"""
    quiet = SimpleNamespace(info=lambda *a, **k: None, disabled=False)
    helper = ref_functions.load(ref_functions.BASIC_UTILS, ["get_rounded_percentage"])
    ns = dict(LOGGER=quiet, TB_LOGGER=SimpleNamespace(log_scalar_dict=val_log.update), all_gather_list=lambda x: [x], time=time,
              tqdm=lambda *a, **k: SimpleNamespace(update=lambda n: None), **helper)
    return ref_functions.load(QA_RUNNER, ["forward_step", "validate"], extra_ns=ns)["validate"]


def _reference_dataset(task, qid2data, label2ans):
    ev = ref_functions.load_method(QA_DATASET, "ClipBertVideoQADataset", "evaluate_tgif_qa")
    ds = SimpleNamespace(task_type=task, open_ended_qa_names=["frameqa", "msrvtt_qa"], label2ans=label2ans, qid2data=qid2data)
    ds.evaluate_tgif_qa = lambda results: ev(ds, results)
    return ds


class _Loader:
    """fresh copies per pass: the reference's loop deletes and rewrites entries of the batch it is given"""

    def __init__(self, batches, dataset=None):
        self.batches, self.dataset = batches, dataset

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for b in self.batches:
            yield {k: (list(v) if isinstance(v, list) else v) for k, v in b.items()}


class _OracleModel(torch.nn.Module):
    """the CPU oracle behind the reference's model(batch) call"""

    def __init__(self, sd, cfg, head, seen):
        super().__init__()
        self.sd, self.cfg, self.head, self.seen = sd, cfg, head, seen

    def forward(self, batch):
        out = O.clipbert_forward(self.sd, {k: v for k, v in batch.items() if not (k == "labels" and v is None)}, self.cfg, self.head)
        self.seen.append(float(out["logits"].abs().max()))   # (the size of the logits: what the kernel's loss bound scales with)
        return out


class _Replay(torch.nn.Module):
    """a model that replays canned per-clip logits, one (B, C) tensor per call, starting over after the last (every validation consumes
    all of them); with labels it returns the head's per-example loss"""

    def __init__(self, canned, task):
        super().__init__()
        self.canned, self.task, self.calls = canned, task, 0

    def forward(self, batch):
        logits = self.canned[self.calls % len(self.canned)].clone()
        self.calls += 1
        rows = TASKS[self.task][3]
        assert list(batch["n_examples_list"]) == [rows] * logits.shape[0] and batch["text_input_ids"].shape[0] == rows * logits.shape[0]
        loss, labels = 0, batch.get("labels")
        if labels is not None:
            loss = ((logits.view(-1) - labels.float()) ** 2 if self.task == "count"
                    else torch.nn.functional.cross_entropy(logits, labels.long(), reduction="none"))
        return dict(logits=logits, loss=loss)


# ---- the small models and their batches ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small(task, dtype, dev):
    """(cfg, state dict, model in eval mode) per (task, dtype, device): built once, only ever run forward"""
    head, extra, _, _ = TASKS[task]
    cfg, sd, model = build(head, extra, dtype, torch.device(dev))
    model.eval()
    return cfg, sd, model


def _qa_batch(task, vocab, qids, seed, labels=None, wide=True, n_frames=N_CLIPS * NUM_FRM):
    bsz, rows = len(qids), TASKS[task][3]
    f = S.synthetic_frames(bsz, n_frames, 64, seed)                                                          # (B, n, 3, 64, 64)
    if wide:
        f = f[..., :64, :].repeat(1, 1, 1, 1, 2).contiguous()                                                # (B, n, 3, 64, 128)
    ids, mask = S.synthetic_text(bsz * rows, LT, seed, vocab)
    return D.collate_qa(O.image_norm(f, S.PIXEL_MEAN, S.PIXEL_STD), ids.clamp(max=vocab - 1), mask, qids, labels=labels, n_options=rows)


def _with_labels(batches, qid2label):
    return [dict(b, labels=torch.tensor([qid2label[q] for q in b["question_ids"]])) for b in batches]


def _ground_truth(task, probe_results):
    """the reference decides what is right: its answers with the second one changed are the ground truth (2 of 3 right; count: 3 of 4)
    -> (qid2label for the batches, qid2data, label2ans)"""
    n_labels = TASKS[task][2]
    qid2label = {r["question_id"]: int(r["answer"]) for r in probe_results}
    flip = probe_results[1]["question_id"]
    qid2label[flip] = (qid2label[flip] % 10) + 1 if task == "count" else (qid2label[flip] + 1) % n_labels
    label2ans = {i: f"ans{i}" for i in range(n_labels)} if task == "frameqa" else None
    qid2data = {}
    for i, (q, lab) in enumerate(qid2label.items()):
        qid2data[q] = dict(question_id=q, answer=label2ans[lab] if label2ans else lab)
        if task == "frameqa":
            qid2data[q]["answer_type"] = FRAMEQA_TYPES[i]
    return qid2label, qid2data, label2ans


def _compare_with_reference(task, pool, ref_model_fn, model, batches, loss_tol_fn, full=True, **loop_kw):
    """probe with the reference (eval_score=False), build the ground truth, run both validations -> nothing; asserts.  full=False (a
    model whose every pass costs seconds): one validation of the product, started in training mode"""
    cfg = _qcfg(task, pool)
    log0 = {}
    probe_ds = _reference_dataset(task, {q: None for b in batches for q in b["question_ids"]}, None)
    probe, zero = _reference_validate(log0)(ref_model_fn(), _Loader(batches, probe_ds), cfg, 0, eval_score=False)
    assert zero == 0 and log0 == {"valid/loss": 0.0}        # (no labels: the reference's loss is 0)
    if full:
        got_probe, got_zero = tasks.validate_video_qa(model, _Loader(batches), cfg, eval_score=False, val_log=(glog0 := {}), **loop_kw)
        assert got_zero == 0 and glog0 == {"valid/loss": 0.0}
        assert [(r["question_id"], r["answer"]) for r in got_probe] == [(r["question_id"], r["answer"]) for r in probe]
    qid2label, qid2data, label2ans = _ground_truth(task, probe)
    labelled = _with_labels(batches, qid2label)
    want_log = {}
    want_results, want_scores = _reference_validate(want_log)(ref_model_fn(), _Loader(labelled, _reference_dataset(task, qid2data, label2ans)),
                                                              cfg, 0, eval_score=True)
    for was_training in (True, False) if full else (True,):
        model.train(was_training)
        got_log = {}
        got_results, got_scores = tasks.validate_video_qa(model, _Loader(labelled), cfg, qid2data=qid2data, label2ans=label2ans,
                                                          val_log=got_log, **loop_kw)
        assert model.training is was_training
        assert got_results == want_results and all(type(r["answer"]) is int for r in got_results)
        assert got_scores == want_scores, (got_scores, want_scores)
        assert set(got_log) == set(want_log) and all(got_log[k] == want_log[k] for k in want_log if k != "valid/loss")
        err, tol = abs(got_log["valid/loss"] - want_log["valid/loss"]), loss_tol_fn(want_log["valid/loss"])
        print(f"{task} {pool}: valid/loss {got_log['valid/loss']:.6f} (reference {want_log['valid/loss']:.6f}): |difference| {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol
    model.eval()
    assert want_scores["overall_acc"] == (0.75 if task == "count" else 66.67)
    if task == "frameqa":                                   # an empty answer type: accuracy 0, ratio [0.0, 0]
        assert want_scores["location_acc"] == 0 and want_scores["ratios"]["location_ratio"] == [0.0, 0]
        assert want_scores["ratios"]["object_ratio"] == [33.33, 1]
    if not full:
        return
    # the labels in the batches alone (no qid2data) give the same scores
    types = {b["question_ids"][0]: [qid2data[q].get("answer_type") for q in b["question_ids"]] for b in labelled}
    typed = [dict(b, answer_types=types[b["question_ids"][0]]) if task == "frameqa" else b for b in labelled]
    assert tasks.validate_video_qa(model, _Loader(typed), cfg, **loop_kw)[1] == want_scores
    # the old path (tasks.qa_predict) and the new one agree on the answers
    for i, b in enumerate(labelled):
        model.calls = i * N_CLIPS                           # (a _Replay: both paths read this batch's canned clips)
        old = tasks.qa_predict(model, {k: v for k, v in b.items() if k != "question_ids"}, cfg)
        model.calls = i * N_CLIPS
        pred, loss = tasks.qa_predict_batch(model, dict(b), cfg, **loop_kw)
        assert old == pred.tolist() and tuple(loss.shape) == (len(old),)


@live
@pytest.mark.parametrize("task", list(TASKS))
def test_validate_matches_the_reference_over_the_oracle_model(emul, task):
    """3 videos in batches of 2 + 1 (count: 4 in 2 + 2), 2 clips x 2 frames at 64x128, text length 6: the reference's validate over the CPU oracle against
    validate_video_qa over the product model (feature cache on).  Answers and every score identical; valid/loss within the kernel's loss
    bound plus the tolerance tests/test_tasks.py holds a loss of the emulator run to (rtol 2e-3, atol 2e-4)."""
    cfg, sd, model = _small(task, torch.float32, "cpu")
    head, c = TASKS[task][0], TASKS[task][2]
    batches = [_qa_batch(task, cfg["vocab_size"], qids, seed) for qids, seed in _QIDS[task == "count"]]
    # the kernel's bound for logits up to 10 in size and, count, labels in 1..10 (the oracle's logits are asserted to stay below 9)
    kernel = 4.0 * R.EPS * (N_CLIPS + 3) * 20.0 ** 2 if task == "count" else R.loss_bound(torch.full((N_CLIPS, 1, c), 10.0))
    seen = []
    _compare_with_reference(task, "mean", lambda: _OracleModel(sd, cfg, head, seen), model, batches,
                            lambda ref: kernel + 2e-3 * abs(ref) + 2e-4, full=False)
    assert len(seen) == 2 * 2 * N_CLIPS and max(seen) <= 9.0


@live
@pytest.mark.parametrize("pool", list(MODES))
@pytest.mark.parametrize("task", list(TASKS))
def test_validate_matches_the_reference_on_canned_logits(emul, task, pool):
    """the loop's host logic with the model taken out: both loops replay the same per-clip logits (cache_cnn=False, the reference's order),
    so answers and scores are identical and valid/loss differs by the kernel's loss bound plus the reference's own fp32 loss rounding"""
    c = TASKS[task][2]
    g = torch.Generator().manual_seed(5 + c)
    batches, stacks = [], []
    for qids, _ in _QIDS[task == "count"]:
        rows = TASKS[task][3]
        st = torch.randn(N_CLIPS, len(qids), c, generator=g) * 1.5 + (4.0 if task == "count" else 0.0)
        stacks.append(st)
        batches.append(D.collate_qa(torch.zeros(len(qids), N_CLIPS * NUM_FRM, 3, 4, 4), torch.ones(len(qids) * rows, LT, dtype=torch.long),
                                    torch.ones(len(qids) * rows, LT, dtype=torch.long), qids, n_options=rows))
    for st in stacks:                                       # a decided answer for every question
        pooled = R.pool(st, pool)
        assert float((R.round_distance(pooled) if task == "count" else R.top2_margin(pooled)).min()) > 2 * R.pooled_bound(st)
    canned = [clip for st in stacks for clip in st.unbind(0)]
    big = torch.cat([st.reshape(N_CLIPS, -1) for st in stacks], dim=1).unsqueeze(-1) if task == "count" else torch.cat(stacks, dim=1)
    # count: labels lie in 1..10 and logits around 4: |x - label| <= 16 (asserted through the stack's range)
    assert task != "count" or float(big.abs().max()) <= 10.0
    kernel = 4.0 * R.EPS * (N_CLIPS + 3) * 20.0 ** 2 if task == "count" else R.loss_bound(big)

    _compare_with_reference(task, pool, lambda: _Replay(canned, task), _Replay(canned, task), batches, lambda ref: kernel + 8 * R.EPS * max(1.0, abs(ref)) * N_CLIPS,
                            cache_cnn=False)


# ---- the clip loop -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,pairs", [("action", 20), ("frameqa", 4)])
def test_cached_clip_loop_equals_the_reference_order(hw, task, pairs):
    """3 videos x 2 clips: 6 (clip, video) blocks in encoder passes of 4 + a remainder of 2 (a pass that runs across the clip boundary)
    give the stack of the reference's order of evaluation within 1.01e-4 (the bound tests/test_tasks.py holds the retrieval loop's same
    comparison to) and the same answers"""
    cfg, sd, model = _small(task, torch.float32, str(hw.dev))
    c = TASKS[task][2]
    qcfg = _qcfg(task, "lse")
    batch = to_dev(_qa_batch(task, cfg["vocab_size"], ["a", "b", "c"], 11, labels=[1, 0, 3]), hw.dev)
    slow = tasks.qa_clip_logits(model, dict(batch), qcfg, cache_cnn=False)
    fast = tasks.qa_clip_logits(model, dict(batch), qcfg, cache_cnn=True, max_pairs_per_pass=pairs)
    assert tuple(slow.shape) == tuple(fast.shape) == (N_CLIPS, 3, c) and slow.dtype == fast.dtype == torch.float32
    diff = float((fast - slow).abs().max())
    margins = R.top2_margin(R.pool(slow, "lse"))
    print(f"{task}: max |stack(cached) - stack(per clip)| = {diff:.3e}; float64 top-2 margins of the pooled logits {[f'{m:.2e}' for m in margins.tolist()]}")
    assert diff <= 1.01e-4
    s_pred, s_loss, _ = ops.qa_predict(slow, MODES["lse"], labels=batch["labels"].to(torch.int32))
    b_pred, b_loss, _ = ops.qa_predict(fast, MODES["lse"], labels=batch["labels"].to(torch.int32))
    assert torch.equal(b_pred, s_pred)
    assert float((b_loss - s_loss).abs().max()) <= 2 * 1.01e-4 + 2 * R.loss_bound(slow)      # (each logit moves by <= 1.01e-4: lse and x[label] both)
    with pytest.raises(ValueError):
        tasks.qa_clip_logits(model, dict(batch, n_examples_list=[1, 2, 1]), qcfg)
    with pytest.raises(ValueError, match="score_agg_func"):
        tasks.qa_predict_batch(model, dict(batch), _qcfg(task, "median"))


def test_captured_encoder_passes_equal_eager(hw):
    """frameqa batches of one signature, one encoder pass over all (clip, video) blocks but one + a remainder of 1: on the emulator
    capture="dry" -- the bookkeeping without graphs --, on the GPU hipGraph replays; the stack is bit-equal to the eager one on every
    batch, replays included, and the whole loop returns the eager loop's answers"""
    gpu = hw.name == "gpu"
    cfg, sd, model = _small("frameqa", torch.bfloat16 if gpu else torch.float32, str(hw.dev))
    capture = True if gpu else "dry"
    n_batches, bsz = (4, 3) if gpu else (3, 2)
    qcfg = SimpleNamespace(**dict(vars(_qcfg("frameqa", "max")), num_frm=1))
    batches = [to_dev(_qa_batch("frameqa", cfg["vocab_size"], [f"q{i}_{j}" for j in range(bsz)], 50 + i, labels=[i] * bsz, wide=gpu, n_frames=N_CLIPS),
                      hw.dev) for i in range(n_batches)]
    pairs = N_CLIPS * bsz - 1
    assert getattr(model, "_captured_forward", None) is None
    try:
        for b in batches:
            want = tasks.qa_clip_logits(model, dict(b), qcfg, max_pairs_per_pass=pairs)
            got = tasks.qa_clip_logits(model, dict(b), qcfg, max_pairs_per_pass=pairs, capture=capture)
            assert torch.equal(got, want)
        cf = model._captured_forward
        assert cf.mode == ("graph" if gpu else "dry") and cf.stats["captures"] == 2 and cf.stats["failed_captures"] == 0, cf.stats
        assert cf.log == ["eager"] * 4 + ["replay"] * (2 * n_batches - 4), cf.log
        loop = batches if gpu else batches[:1]               # (every pass costs the emulator seconds)
        want_rows, want_scores = tasks.validate_video_qa(model, loop, qcfg)
        got_rows, got_scores = tasks.validate_video_qa(model, loop, qcfg, capture=capture)
        assert got_rows == want_rows and len(got_rows) == len(loop) * bsz and got_scores == want_scores
        with pytest.raises(ValueError):
            tasks.qa_clip_logits(model, dict(batches[0]), qcfg, cache_cnn=False, capture=capture)
    finally:
        model._captured_forward = None


# ---- scores and counters --------------------------------------------------------------------------------------------------------------
@live
@pytest.mark.parametrize("task", ["frameqa", "msrvtt_qa", "action", "count"])
def test_video_qa_scores_match_evaluate_tgif_qa(task):
    g = torch.Generator().manual_seed(3)
    n = 23
    gt = torch.randint(1, 9, (n,), generator=g)
    pred = torch.where(torch.rand(n, generator=g) < 0.6, gt, torch.randint(1, 9, (n,), generator=g))
    names = tasks.QA_ANSWER_TYPES.get(task)
    types = [names[int(i)] for i in torch.randint(0, len(names) - 1, (n,), generator=g)] if names else None      # (the last type stays empty)
    label2ans = {i: f"ans{i}" for i in range(10)} if names else None
    qid2data = {q: dict(answer=label2ans[int(a)] if names else int(a), **(dict(answer_type=types[q]) if names else {})) for q, a in enumerate(gt)}
    want = _reference_dataset(task, qid2data, label2ans).evaluate_tgif_qa([dict(question_id=q, answer=int(a)) for q, a in enumerate(pred)])
    got = tasks.video_qa_scores(pred.numpy(), gt.numpy(), types, task)
    assert got == want and ("ratios" in got) == bool(names)
    if names:
        assert got[f"{names[-1]}_acc"] == 0 and got["ratios"][f"{names[-1]}_ratio"] == [0.0, 0]
        with pytest.raises(KeyError):
            tasks.video_qa_scores(pred.numpy(), gt.numpy(), ["nothing"] * n, task)


@pytest.mark.parametrize("task", ["frameqa", "count"])
def test_counters_of_two_halves_merge_to_the_whole(task):
    g = torch.Generator().manual_seed(9)
    n, cut = 37, 15
    gt = torch.randint(1, 11, (n,), generator=g).numpy()
    pred = torch.where(torch.rand(n, generator=g) < 0.5, torch.as_tensor(gt), torch.randint(1, 11, (n,), generator=g)).numpy()
    names = tasks.QA_ANSWER_TYPES.get(task)
    types = [names[int(i)] for i in torch.randint(0, len(names), (n,), generator=g)] if names else None
    loss = torch.rand(n, generator=g).double().numpy()
    whole = tasks.video_qa_counters(pred, gt, types, task, float(loss.sum()))
    halves = [tasks.video_qa_counters(pred[s], gt[s], types[s] if types else None, task, float(loss[s].sum())) for s in (slice(0, cut), slice(cut, n))]
    merged = tasks.merge_video_qa_counters(halves)
    assert {k: v for k, v in merged.items() if k != "loss_sum"} == {k: v for k, v in whole.items() if k != "loss_sum"}
    assert merged["loss_sum"] == pytest.approx(whole["loss_sum"], rel=1e-14)
    assert whole["n"] == n and whole["abs_err"] == int(abs(pred - gt).sum()) and whole["hits"] == int((pred == gt).sum())
    assert tasks.video_qa_metrics(merged, task) == tasks.video_qa_metrics(whole, task)
    shown = tasks.video_qa_metrics(whole, task)
    assert shown["overall_acc"] == (round(whole["hits"] / n * 100, 2) if names else round(whole["hits"] / n, 2))
    if names:
        assert sum(v[1] for v in shown["ratios"].values()) == n
    assert tasks._all_gather_scalar(whole) == [whole]       # a single process: the merge sees one rank


def test_collate_qa():
    videos = [torch.full((4, 3, 8, 8), float(i)) for i in range(3)]
    ids = [torch.arange(5 * 6).view(5, 6) + 100 * i for i in range(3)]
    mask = [torch.ones(5, 6, dtype=torch.long) for _ in range(3)]
    b = D.collate_qa(videos, ids, mask, ["a", "b", "c"], labels=[4, 0, 2], n_options=5)
    assert set(b) == {"visual_inputs", "text_input_ids", "text_input_mask", "question_ids", "labels", "n_examples_list"}
    assert tuple(b["visual_inputs"].shape) == (3, 4, 3, 8, 8) and tuple(b["text_input_ids"].shape) == tuple(b["text_input_mask"].shape) == (15, 6)
    assert b["n_examples_list"] == [1, 1, 1] and b["question_ids"] == ["a", "b", "c"]
    assert b["labels"].dtype == torch.int64 and b["labels"].tolist() == [4, 0, 2]
    assert torch.equal(b["text_input_ids"][5:10], ids[1]) and float(b["visual_inputs"][2].max()) == 2.0      # video v's rows: 5v ..
    one = D.collate_qa(torch.stack(videos), [i[0] for i in ids], [m[0] for m in mask], [1, 2, 3])
    assert tuple(one["text_input_ids"].shape) == (3, 6) and one["labels"] is None and torch.equal(one["text_input_ids"][2], ids[2][0])
    with pytest.raises(ValueError):
        D.collate_qa(videos, ids, mask, ["a", "b", "c"])     # 15 text rows for n_options = 1
    with pytest.raises(ValueError):
        D.collate_qa(videos, ids, mask, ["a", "b"], n_options=5)
    with pytest.raises(ValueError):
        D.collate_qa(videos, ids, mask, ["a", "b", "c"], labels=[1], n_options=5)
