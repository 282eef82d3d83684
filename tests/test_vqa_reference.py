"""The host pieces of the image-VQA task against the REFERENCE's own code, executed from its source (oracle/ref_functions.py): the sparse
answer tables against ClipBertVQADataset._get_vqa_targets, the metric arithmetic of tasks.validate_vqa against ClipBertVQADataset.
evaluate_vqa (src/datasets/dataset_vqa.py:57-112), and tasks.vqa_loss on the reference's dense batch format against the oracle's
loss.mean() * num_labels (src/tasks/run_vqa.py:355-356).  CPU only; the live tests are skipped where the reference checkout (oracle/ref_shim.py) is absent."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from clipbert_amd import tasks
from clipbert_amd.data import vqa_dense_targets, vqa_sparse_targets
from oracle import clipbert_oracle as O
from oracle import ref_shim

live = pytest.mark.skipif(not ref_shim.available(), reason="needs the reference checkout")
DATASET_VQA = os.path.join("src", "datasets", "dataset_vqa.py")
SCORES = (0.3, 0.6, 0.9, 1.0)


def _answers(rng, ans2label, n):
    names = list(ans2label)
    picked = rng.permutation(len(names))[:n]
    return {names[int(i)]: float(SCORES[int(rng.integers(0, 4))]) for i in picked}


@live
def test_sparse_tables_scatter_to_the_reference_targets():
    from oracle import ref_functions as RF
    get_targets = RF.load_method(DATASET_VQA, "ClipBertVQADataset", "_get_vqa_targets")
    rng = np.random.default_rng(3)
    ans2label = {f"answer {i}": int(l) for i, l in enumerate(rng.permutation(40))}
    ds = SimpleNamespace(num_labels=len(ans2label), ans2label=ans2label)
    questions = [_answers(rng, ans2label, n) for n in (0, 1, 3, 10, 3)]
    ids, scores = vqa_sparse_targets(questions, ans2label)
    assert ids.dtype == torch.int32 and scores.dtype == torch.float32 and ids.shape == scores.shape == (5, 10)
    for q, row_ids, row_scores in zip(questions, ids, scores):
        n = len(q)
        assert row_ids[:n].tolist() == [ans2label[a] for a in q] and (row_ids[n:] == -1).all()             # the dict's order, then padding
        assert (row_scores[n:] == 0).all()
    want = torch.stack([get_targets(ds, q) for q in questions])
    assert torch.equal(vqa_dense_targets(ids, scores, ds.num_labels), want)
    assert vqa_sparse_targets(questions[:3], ans2label, max_answers=3)[0].shape == (3, 3)
    with pytest.raises(KeyError):
        vqa_sparse_targets([{"not an answer": 1.0}], ans2label)
    with pytest.raises(KeyError):
        get_targets(ds, {"not an answer": 1.0})
    with pytest.raises(ValueError, match="max_answers"):
        vqa_sparse_targets([questions[3]], ans2label, max_answers=9)


@live
def test_metric_arithmetic_equals_the_reference_evaluate_vqa():
    """40 questions (20 yes/no, 10 number, 10 other), scores from {0.3, 0.6, 0.9, 1.0}: every exact percentage is a multiple of 0.25, so no
    value sits on a boundary of the two-decimal rounding"""
    from oracle import ref_functions as RF
    evaluate = RF.load_method(DATASET_VQA, "ClipBertVQADataset", "evaluate_vqa")
    rng = np.random.default_rng(11)
    ans2label = {f"answer {i}": i for i in range(30)}
    label2ans = {v: k for k, v in ans2label.items()}
    types = ["yes/no"] * 20 + ["number"] * 10 + ["other"] * 10
    order = rng.permutation(40)
    types = [types[int(i)] for i in order]
    questions = [_answers(rng, ans2label, int(rng.integers(1, 11))) for _ in range(40)]
    pred = []
    for i, q in enumerate(questions):                                          # two predictions in three are one of the answers
        pred.append(ans2label[list(q)[int(rng.integers(0, len(q)))]] if i % 3 else int(rng.integers(0, 30)))
    qid2data = {1000 + i: dict(labels=q, answer_type=t, question_id=1000 + i) for i, (q, t) in enumerate(zip(questions, types))}
    ref = evaluate(SimpleNamespace(qid2data=qid2data), [dict(question_id=1000 + i, answer=label2ans[p]) for i, p in enumerate(pred)])
    ids, scores = vqa_sparse_targets(questions, ans2label)
    ours = tasks.evaluate_vqa(pred, types, ids, scores)
    want = {k: round(100 * v, 2) for k, v in ref.items() if k != "ratios"}
    assert set(want) == {"overall_acc", "yes/no_acc", "number_acc", "other_acc"} and ours == want, (ours, want)
    assert 0 < want["overall_acc"] < 100
    # the same through per-batch sums, as validate_vqa accumulates them
    total = {}
    for lo, hi in ((0, 13), (13, 40)):
        part = tasks.vqa_score_sums(tasks.vqa_pred_scores(pred[lo:hi], ids[lo:hi], scores[lo:hi]), types[lo:hi])
        for k, (s, n) in part.items():
            total[k] = [total.get(k, [0.0, 0])[0] + s, total.get(k, [0.0, 0])[1] + n]
    assert tasks.vqa_metrics(total) == want and [total[k][1] for k in ("overall", "yes/no", "number", "other")] == [40, 20, 10, 10]
    assert tasks.evaluate_vqa(pred, None, ids, scores) == {"overall_acc": want["overall_acc"]}
    with pytest.raises(KeyError):
        tasks.evaluate_vqa(pred[:2], ["yes/no", "colour"], ids[:2], scores[:2])


def test_vqa_loss_on_dense_labels_is_the_runners_loss(emul):
    """the reference's batch format: tasks.vqa_loss = loss.mean() * num_labels (run_vqa.py:355-356) of the oracle's (pairs, C) loss; the
    sparse batch gives the same number"""
    from test_model_small import build, make_batch
    cfg, sd, model = build("sequence_classification", dict(num_labels=6, loss_type="bce"), torch.float32, torch.device("cpu"))
    batch = make_batch(cfg, "sequence_classification", 1, 2, 5)
    ids = torch.tensor([[4, 1, -1], [-1, -1, -1]], dtype=torch.int32)
    scores = torch.tensor([[1.0, 0.3, 0.0], [0.0, 0.0, 0.0]])
    dense = vqa_dense_targets(ids, scores, 6)
    with torch.no_grad():
        ref = O.clipbert_forward(sd, dict(batch, labels=dense), cfg, "sequence_classification")
        want = float(ref["loss"].mean() * cfg["num_labels"])
        got_dense = float(tasks.vqa_loss(model, dict(batch, labels=dense, question_ids=[7, 8]), cfg))
        got_sparse = float(tasks.vqa_loss(model, dict(batch, answer_ids=ids, answer_scores=scores, question_ids=[7, 8], answer_types=["other"] * 2), cfg))
    assert got_dense == pytest.approx(want, rel=1e-3) and got_sparse == pytest.approx(want, rel=1e-3), (got_dense, got_sparse, want)
    assert got_sparse == pytest.approx(got_dense, rel=1e-5)
    with pytest.raises(ValueError, match="neither"):
        tasks.vqa_loss(model, dict(batch, question_ids=[7, 8]), cfg)
