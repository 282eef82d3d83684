"""cb_qa_predict through ops.qa_predict -- pooling, answer and loss of the video-QA validation in one launch -- against the float64
restatement of src/tasks/run_video_qa.py:250-279 (qa_restatement.py, which derives the bounds), on the host emulator and on the GPU.

The arg-max is exact on every question: the float64 top-2 margin of the pooled logits of every random question is asserted to exceed
twice the pooled bound (no question is excluded), and the constructed questions have their answer by construction.  Likewise the count
answer: the float64 distance of pooled + 0.5 to the nearest integer is asserted to exceed the pooled bound for every random row."""
import functools
import math

import pytest
import torch

import qa_restatement as R
from clipbert_amd import ops

# (n_clips, n_q, C): smallest; one question; several questions per workgroup; questions straddling a workgroup; the wave / workgroup switch
# at C = 64 | 65; 256 -+ 1 lanes; frameqa at the retrieval config's 16 clips
CLASSIFY = [(1, 1, 1), (1, 1, 5), (3, 7, 5), (2, 53, 5), (4, 3, 64), (4, 3, 65), (2, 2, 255), (2, 2, 257), (16, 3, 1540)]
COUNT = [(5, 9, 1), (16, 40, 1)]
MODES = {"mean": ops.AGG_MEAN, "max": ops.AGG_MAX, "lse": ops.AGG_LSE}


def _ids(case):
    return "x".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def _classify_case(case):
    """the case's stack, labels and, per pooling method, the float64 (pooled, pred, loss): computed once, never written to"""
    n_clips, n_q, c = case
    g = torch.Generator().manual_seed(7 + n_q + n_clips + c)
    stack = torch.randn(n_clips, n_q, c, generator=g) * 1.5
    labels = torch.randint(0, c, (n_q,), generator=g, dtype=torch.int32)
    return stack, labels, {pool: R.classify(stack, pool, labels) for pool in MODES}


@functools.lru_cache(maxsize=None)
def _count_case(case):
    n_clips, n_q, c = case
    g = torch.Generator().manual_seed(11 + n_q + n_clips)
    stack = torch.randn(n_clips, n_q, 1, generator=g) * 1.5 + torch.linspace(-8, 16, n_q).view(1, n_q, 1)     # answers below 1, inside, above 10
    labels = torch.randint(1, 11, (n_q,), generator=g).float()
    return stack, labels, {pool: R.count(stack, pool, labels) for pool in MODES}


def _run(hw, stack, pool, kind=ops.QA_CLASSIFY, labels=None, **kw):
    pred, loss, pooled = ops.qa_predict(hw(stack), MODES[pool], kind=kind, labels=hw(labels), want_pooled=True, **kw)
    n_clips, n_q, c = stack.shape
    assert pred.dtype == torch.int32 and tuple(pred.shape) == (n_q,)
    assert pooled.dtype == torch.float32 and tuple(pooled.shape) == (n_q, c)
    assert (loss is None) == (labels is None)
    if loss is not None:
        assert loss.dtype == torch.float32 and tuple(loss.shape) == (n_q,)
        loss = loss.cpu()
    return pred.cpu().long(), loss, pooled.cpu()


@pytest.mark.parametrize("pool", list(MODES))
@pytest.mark.parametrize("case", CLASSIFY, ids=_ids)
def test_classify_matches_the_restatement(hw, case, pool):
    stack, labels, refs = _classify_case(case)
    ref_pooled, ref_pred, ref_loss = refs[pool]
    pb, lb = R.pooled_bound(stack), R.loss_bound(stack)
    margin = float(R.top2_margin(ref_pooled).min())
    print(f"{case} {pool}: pooled bound {pb:.3e}, loss bound {lb:.3e}, smallest float64 top-2 margin {margin:.3e}")
    assert margin > 2 * pb                                  # precondition of an exact arg-max, for EVERY question
    pred, loss, pooled = _run(hw, stack, pool, labels=labels)
    perr = float((pooled.double() - ref_pooled).abs().max())
    lerr = float((loss.double() - ref_loss).abs().max())
    print(f"{case} {pool}: max |pooled - float64| = {perr:.3e}, max |loss - float64| = {lerr:.3e}")
    assert perr <= pb
    assert lerr <= lb
    assert torch.equal(pred, ref_pred)


@pytest.mark.parametrize("pool", list(MODES))
@pytest.mark.parametrize("case", COUNT, ids=_ids)
def test_count_matches_the_restatement(hw, case, pool):
    stack, labels, refs = _count_case(case)
    ref_pooled, ref_pred, ref_loss = refs[pool]
    pb, lb = R.pooled_bound(stack), R.count_loss_bound(stack, labels)
    dist = float(R.round_distance(ref_pooled).min())
    print(f"{case} {pool}: pooled bound {pb:.3e}, loss bound {lb:.3e}, smallest distance of pooled + 0.5 to an integer {dist:.3e}")
    assert dist > pb                                        # precondition of an exact answer, for EVERY row
    assert int(ref_pred.min()) == 1 and int(ref_pred.max()) == 10 and len(set(ref_pred.tolist())) > 2       # both clamps and the middle
    pred, loss, pooled = _run(hw, stack, pool, kind=ops.QA_COUNT, labels=labels)
    perr = float((pooled.double() - ref_pooled).abs().max())
    lerr = float((loss.double() - ref_loss).abs().max())
    print(f"{case} {pool}: max |pooled - float64| = {perr:.3e}, max |loss - float64| = {lerr:.3e}")
    assert perr <= pb
    assert lerr <= lb
    assert torch.equal(pred, ref_pred)


@pytest.mark.parametrize("pool", list(MODES))
@pytest.mark.parametrize("n_clips", [1, 5])
def test_constructed_count_rows(hw, n_clips, pool):
    """every clip of a row holds the same value: mean and max pool to it exactly, the log-sum-exp adds ln(n_clips) (1.61 for 5 clips)"""
    values = [3.5, -0.7, 0.49, 10.6, 1e6, -1e6]
    want = [4, 1, 1, 10, 10, 1]
    if pool == "lse" and n_clips == 5:                      # 3.5 + 1.61 + 0.5 = 5.61 -> 5; -0.7 + 1.61 + 0.5 = 1.41 -> 1; 0.49 + 2.11 = 2.60 -> 2
        want = [5, 1, 2, 10, 10, 1]
    stack = torch.tensor(values).view(1, -1, 1).repeat(n_clips, 1, 1).contiguous()
    labels = torch.tensor([4.0, 1.0, 1.0, 10.0, 10.0, 1.0])
    ref_pooled, ref_pred, ref_loss = R.count(stack, pool, labels)
    assert ref_pred.tolist() == want                        # (the restatement agrees with the construction)
    pred, loss, pooled = _run(hw, stack, pool, kind=ops.QA_COUNT, labels=labels)
    assert pred.tolist() == want
    assert float((loss.double() - ref_loss).abs()[:4].max()) <= R.count_loss_bound(stack[:, :4], labels[:4])  # (rows 0-3: their own bound)
    rel = ((loss.double() - ref_loss).abs() / ref_loss)[4:]
    assert float(rel.max()) <= 4 * R.EPS * (n_clips + 3)    # the 1e6 rows: the same bound, relative to D^2


def test_count_nan_gives_an_answer_in_range(hw):
    stack = torch.tensor([[[float("nan")], [2.2]], [[1.0], [float("nan")]]])
    pred, _, _ = _run(hw, stack, "mean", kind=ops.QA_COUNT)
    assert all(1 <= p <= 10 for p in pred.tolist())


def _constructed(case):
    """the random stack of the case followed by constructed questions -> (stack, labels, {question: expected answer})"""
    n_clips, n_q, c = case
    stack, labels, _ = _classify_case(case)
    g = torch.Generator().manual_seed(1000 + n_q + n_clips + c)
    extra, extra_labels, expect = [], [], {}

    def add(rows, label, answer):
        expect[n_q + len(extra)] = answer
        extra.append(rows)
        extra_labels.append(label)

    lo, hi = (c - 1) // 3, c - 1
    if c >= 2:                                              # two bit-equal maxima: the lower index wins
        tie = torch.randn(n_clips, c, generator=g) * 1.5
        tie[:, lo] = 12.0
        tie[:, hi] = 12.0
        add(tie, hi, lo)
    add(torch.full((n_clips, c), 80.0), hi, 0)              # all logits equal: answer 0, loss ln C
    add(torch.full((n_clips, c), -80.0), lo, 0)
    if c >= 2:                                              # one class at +80 against -80: loss exactly 0 at the label, 160 at any other
        one = torch.full((n_clips, c), -80.0)
        one[:, hi] = 80.0
        add(one, hi, hi)
        add(one.clone(), lo, hi)
    stack = torch.cat([stack] + [e.unsqueeze(1) for e in extra], dim=1).contiguous()
    return stack, torch.cat([labels, torch.tensor(extra_labels, dtype=torch.int32)]), expect


@pytest.mark.parametrize("pool", list(MODES))
@pytest.mark.parametrize("case", CLASSIFY, ids=_ids)
def test_constructed_questions(hw, case, pool):
    n_clips, n_q, c = case
    stack, labels, expect = _constructed(case)
    ref_pooled, ref_pred, ref_loss = R.classify(stack, pool, labels)
    pred, loss, pooled = _run(hw, stack, pool, labels=labels)
    for q, want in expect.items():
        assert int(ref_pred[q]) == want                     # (the restatement agrees with the construction)
        assert int(pred[q]) == want, (q, int(pred[q]), want)
    base = n_q
    if c >= 2:                                              # the tie really is one: equal bits, above every other class
        lo, hi = (c - 1) // 3, c - 1
        row = pooled[base]
        assert row[lo] == row[hi] and int((row >= row[lo]).sum()) == 2
        base += 1
    lb = R.loss_bound(stack)
    print(f"{case} {pool}: loss bound with |x| = 80: {lb:.3e}; saturated losses {loss[base:].tolist()}")
    for q in (base, base + 1):                              # all +80 / all -80
        assert abs(float(loss[q]) - math.log(c)) <= lb
    if c >= 2:
        assert float(loss[base + 2]) == 0.0 and float(loss[base + 3]) == 160.0
    random_stack, _, refs = _classify_case(case)
    assert float((loss.double() - ref_loss).abs()[:n_q].max()) <= R.loss_bound(random_stack)     # the random questions: their own (tighter) bound
    assert float((loss.double() - ref_loss).abs().max()) <= lb
    assert float((pooled.double() - ref_pooled).abs().max()) <= R.pooled_bound(stack)
    assert torch.equal(pred[:n_q], refs[pool][1])


def test_nan_counts_as_the_largest_logit(hw):
    """torch.max: a NaN beats every number, the first NaN wins -- in one wave (C = 6) and across the waves of a workgroup (C = 300)"""
    nan = float("nan")
    small = torch.tensor([[[0.5, nan, 3.0, nan, 1.0, 2.0], [9.0, 1.0, 2.0, 3.0, 4.0, nan]]])
    pred, _, _ = _run(hw, small, "mean")
    assert pred.tolist() == R.classify(small, "mean")[1].tolist() == [1, 5]
    big = torch.randn(2, 2, 300, generator=torch.Generator().manual_seed(3))
    big[0, 0, 299] = nan
    big[1, 0, 70] = nan                                     # (wave 1 of the workgroup; 299 sits in wave 0's second stride)
    big[1, 1, 255] = nan
    for pool in MODES:
        pred, _, _ = _run(hw, big, pool)
        assert pred.tolist() == R.classify(big, pool)[1].tolist() == [70, 255]


@pytest.mark.parametrize("pool", list(MODES))
@pytest.mark.parametrize("case,kind,pad,offset", [((3, 7, 5), "classify", 3, 1), ((2, 53, 5), "classify", 2, 2), ((4, 3, 65), "classify", 5, 1),
                                                  ((2, 2, 257), "classify", 1, 3), ((5, 9, 1), "count", 4, 1)],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else str(v))
def test_padded_and_misaligned_stack(hw, case, kind, pad, offset, pool):
    """a view with dim-0 stride n_q*C + pad whose base sits ``offset`` floats into its buffer, NaN in the padding: the same bits as the
    contiguous stack"""
    n_clips, n_q, c = case
    stack, labels, _ = (_classify_case if kind == "classify" else _count_case)(case)
    k = ops.QA_CLASSIFY if kind == "classify" else ops.QA_COUNT
    stride = n_q * c + pad
    buf = torch.full((offset + n_clips * stride,), float("nan"))           # (a read of the padding would poison the results)
    buf[offset:].as_strided((n_clips, n_q, c), (stride, c, 1)).copy_(stack)
    dev_view = hw(buf)[offset:].as_strided((n_clips, n_q, c), (stride, c, 1))
    assert dev_view.stride(0) == stride
    want = ops.qa_predict(hw(stack), MODES[pool], kind=k, labels=hw(labels), want_pooled=True)
    for kw in ({}, dict(clip_stride=stride)):               # (the stride handed over explicitly means the same)
        got = ops.qa_predict(dev_view, MODES[pool], kind=k, labels=hw(labels), want_pooled=True, **kw)
        for a, b in zip(got, want):
            assert not bool(torch.isnan(a.float()).any()) and torch.equal(a.cpu(), b.cpu())


def test_no_labels_no_loss(hw):
    stack, labels, refs = _classify_case((3, 7, 5))
    pred, loss, pooled = ops.qa_predict(hw(stack), ops.AGG_MEAN)
    assert loss is None and pooled is None and torch.equal(pred.cpu().long(), refs["mean"][1])
    big, _, big_refs = _classify_case((2, 2, 257))
    pred, loss, pooled = ops.qa_predict(hw(big), ops.AGG_LSE)
    assert loss is None and pooled is None and torch.equal(pred.cpu().long(), big_refs["lse"][1])
    # without a loss the workgroup kernel keeps nothing per clip: any number of clips
    many = torch.randn(300, 1, 70, generator=torch.Generator().manual_seed(5))
    pred, _, _ = ops.qa_predict(hw(many), ops.AGG_MAX)
    assert pred.cpu().long().tolist() == R.classify(many, "max")[1].tolist()


def test_label_outside_the_classes_gives_nan(hw):
    """nothing is read for such a label; the other questions are untouched"""
    for case in ((3, 7, 5), (2, 2, 257)):
        stack, labels, refs = _classify_case(case)
        bad = labels.clone()
        bad[0] = case[2]
        bad[-1] = -100
        _, loss, _ = _run(hw, stack, "mean", labels=bad)
        assert bool(torch.isnan(loss[0])) and bool(torch.isnan(loss[-1]))
        if case[1] > 2:
            assert float((loss[1:-1].double() - refs["mean"][2][1:-1]).abs().max()) <= R.loss_bound(stack)


def test_error_paths(hw):
    ok = hw(torch.zeros(2, 10, 5))
    with pytest.raises(RuntimeError, match="cb_qa_predict: unknown mode 7"):
        ops.qa_predict(ok, 7)
    with pytest.raises(RuntimeError, match="cb_qa_predict: unknown kind 3"):
        ops.qa_predict(ok, ops.AGG_MEAN, kind=3)
    with pytest.raises(RuntimeError, match="cb_qa_predict: kind count needs C == 1 \\(got 5\\)"):
        ops.qa_predict(ok, ops.AGG_MEAN, kind=ops.QA_COUNT)
    with pytest.raises(RuntimeError, match="cb_qa_predict: clip_stride 49 is smaller than n_q \\* C = 50"):
        ops.qa_predict(ok, ops.AGG_MEAN, clip_stride=49)
    with pytest.raises(RuntimeError, match="cb_qa_predict: bad counts \\(n_clips 2, n_q 0, C 5"):
        ops.qa_predict(hw(torch.zeros(2, 0, 5)), ops.AGG_MEAN)
    with pytest.raises(RuntimeError, match="takes at most 256 clips \\(got 257\\)"):
        ops.qa_predict(hw(torch.zeros(257, 1, 65)), ops.AGG_MEAN, labels=hw(torch.zeros(1, dtype=torch.int32)))
    with pytest.raises(ValueError, match="fp32"):
        ops.qa_predict(ok.double(), ops.AGG_MEAN)
    with pytest.raises(ValueError, match="fp32"):
        ops.qa_predict(ok[0], ops.AGG_MEAN)
    with pytest.raises(ValueError, match="contiguous"):
        ops.qa_predict(hw(torch.zeros(2, 5, 10)).transpose(1, 2), ops.AGG_MEAN)
    with pytest.raises(ValueError, match="labels"):
        ops.qa_predict(ok, ops.AGG_MEAN, labels=hw(torch.zeros(10, dtype=torch.int64)))
    with pytest.raises(ValueError, match="labels"):
        ops.qa_predict(ok, ops.AGG_MEAN, labels=hw(torch.zeros(9, dtype=torch.int32)))
    with pytest.raises(ValueError, match="labels"):
        ops.qa_predict(hw(torch.zeros(2, 10, 1)), ops.AGG_MEAN, kind=ops.QA_COUNT, labels=hw(torch.zeros(10, dtype=torch.int32)))


def test_null_pointers_are_refused(hw):
    from clipbert_amd import _lib
    pred = hw(torch.zeros(4, dtype=torch.int32))
    rc = _lib.get().cb_qa_predict(None, 20, 2, 4, 5, 0, 0, None, pred.data_ptr(), None, None, None)
    assert rc != 0 and "cb_qa_predict: null pointer" in _lib.get().cb_last_error().decode()


def test_refuses_cpu_tensors_on_the_product_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.qa_predict(torch.zeros(1, 5, 2), ops.AGG_MEAN)


def test_abi_entry():
    from clipbert_amd import _lib
    assert _lib.get().cb_version() >= 18 and "cb_qa_predict" in _lib.EXPORTED_SYMBOLS
    assert (ops.QA_CLASSIFY, ops.QA_COUNT) == (0, 1)
