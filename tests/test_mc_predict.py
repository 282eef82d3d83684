"""cb_mc_predict through ops.mc_predict -- the scoring of the MSRVTT multiple-choice test in one launch -- against the float64
restatement of src/tasks/run_msrvtt_mc.py:178-195 (mc_restatement.py), on the host emulator and on the GPU.

Score bound (mc_restatement.score_bound): |score - float64| <= 2 eps (n_clips + 2) max(1, max|x|) + 16 eps, eps = 2^-24.  A pooled logit
carries at most (n_clips + 2) eps max|x| (the additions and the division of the mean; the shift, exponentials, additions, logarithm and
final addition of the max-shifted log-sum-exp); the difference of two pooled logits doubles that; the sigmoid has a slope of at most 1/4
and costs a few ulps of its own; a 4x margin on top.  The arg-max is exact on every group: the float64 top-2 margin of every random group
is asserted to exceed twice the bound (no group is excluded), and the constructed groups -- an exact tie, saturated scores -- have their
answer by construction."""
import functools

import pytest
import torch

import mc_restatement as R
from clipbert_amd import ops

# (n_clips, n_q, n_options, C): one row; one group; several groups in one workgroup; 265, 258 and 600 rows -- groups straddling a
# 256-thread boundary --; more options than a wave / a workgroup has lanes; the retrieval config's 16 clips x 5 options
CASES = [(1, 1, 1, 1), (1, 1, 5, 2), (3, 7, 5, 2), (2, 53, 5, 1), (16, 86, 3, 2), (4, 3, 256, 1), (16, 64, 5, 2), (5, 2, 300, 2)]
MODES = {"mean": ops.AGG_MEAN, "max": ops.AGG_MAX, "lse": ops.AGG_LSE}


def _ids(case):
    return "x".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def _random_case(case):
    """the case's stack and, per pooling method, its float64 scores and arg-max: computed once, never written to"""
    n_clips, n_q, n_options, c = case
    g = torch.Generator().manual_seed(n_q + n_clips)
    stack = torch.randn(n_clips, n_q * n_options, c, generator=g) * 1.5
    return stack, {pool: R.mc_scores(stack, n_options, pool) for pool in MODES}


def _run(hw, stack, n_options, pool, **kw):
    scores, pred = ops.mc_predict(hw(stack), n_options, MODES[pool], **kw)
    assert scores.dtype == torch.float32 and pred.dtype == torch.int32
    assert tuple(scores.shape) == (stack.shape[1],) and tuple(pred.shape) == (stack.shape[1] // n_options,)
    return scores.cpu(), pred.cpu().long()


@pytest.mark.parametrize("pool", list(MODES))
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_scores_and_argmax_match_the_restatement(hw, case, pool):
    n_clips, n_q, n_options, c = case
    stack, refs = _random_case(case)
    ref_scores, ref_pred = refs[pool]
    bound = R.score_bound(stack)
    margin = float(R.top2_margin(ref_scores, n_options).min())
    print(f"{case} {pool}: bound {bound:.3e}, smallest float64 top-2 margin {margin:.3e}")
    assert margin > 2 * bound                              # precondition of an exact arg-max, for EVERY group
    scores, pred = _run(hw, stack, n_options, pool)
    err = float((scores.double() - ref_scores).abs().max())
    print(f"{case} {pool}: max |score - float64| = {err:.3e}")
    assert err <= bound
    assert torch.equal(pred, ref_pred)


def _constructed(case):
    """the random stack of the case followed by constructed groups -> (stack, {group index: expected answer}, rows of the random part)"""
    n_clips, n_q, n_options, c = case
    stack, _ = _random_case(case)
    g = torch.Generator().manual_seed(1000 + n_q + n_clips)

    def const_group(v0, v1):
        grp = torch.empty(n_clips, n_options, c)
        grp[..., 0] = v0
        grp[..., c - 1] = v1                               # (C == 1: v1 is the value)
        return grp

    groups, expect = [], {}
    if n_options >= 2:                                      # two bit-identical rows holding the group's maximum: the lower index wins
        tie = torch.randn(n_clips, n_options, c, generator=g) * 1.5
        lo, hi = (n_options - 1) // 3, n_options - 1
        top = torch.tensor([-6.0, 6.0]) if c == 2 else torch.tensor([12.0])
        tie[:, lo] = top
        tie[:, hi] = top
        expect[n_q + len(groups)] = lo
        groups.append(tie)
    for v0, v1 in ((80.0, 80.0), (-80.0, -80.0)) + (((-80.0, 80.0), (80.0, -80.0)) if c == 2 else ()):
        expect[n_q + len(groups)] = 0                       # every score of the group is the same number
        groups.append(const_group(v0, v1))
    return torch.cat([stack] + groups, dim=1).contiguous(), expect, n_q * n_options


@pytest.mark.parametrize("pool", list(MODES))
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_constructed_groups(hw, case, pool):
    """ties, saturation at 1.0 and at 0 on top of the random rows: all logits +80 / -80 (C == 1: every score is exactly 1.0 / 1.8e-35;
    C == 2: the two classes cancel, every score is exactly 0.5), and for C == 2 also class 1 at +80 / -80 against class 0 at -80 / +80
    (every score exactly 1.0 / 0.0).  The answer of such a group is option 0."""
    n_clips, n_q, n_options, c = case
    stack, expect, n_random = _constructed(case)
    ref_scores, ref_pred = R.mc_scores(stack, n_options, pool)
    scores, pred = _run(hw, stack, n_options, pool)
    for q, want in expect.items():
        assert int(ref_pred[q]) == want                     # (the restatement agrees with the construction)
        assert int(pred[q]) == want, (q, int(pred[q]), want)
    if n_options >= 2:                                      # the tie really is one: equal bits, above every other option of the group
        grp = scores.view(-1, n_options)[n_q]
        lo, hi = (n_options - 1) // 3, n_options - 1
        assert grp[lo] == grp[hi] and int((grp >= grp[lo]).sum()) == 2
    sat = scores.view(-1, n_options)[n_q + (1 if n_options >= 2 else 0):]
    want_sat = [1.0, None] if c == 1 else [0.5, 0.5, 1.0, 0.0]
    for row, want in zip(sat, want_sat):
        assert bool((row == row[0]).all())
        if want is not None:
            assert float(row[0]) == want
        else:
            assert 0.0 < float(row[0]) < 1e-30               # sigmoid(-80) = 1.8e-35: small, not flushed to zero
    err = (scores.double() - ref_scores).abs()
    random_stack, refs = _random_case(case)
    assert float(err[:n_random].max()) <= R.score_bound(random_stack)      # the random rows: their own (tighter) bound
    assert float(err.max()) <= R.score_bound(stack)
    assert torch.equal(pred[:n_q], refs[pool][1])


@pytest.mark.parametrize("pool", list(MODES))
@pytest.mark.parametrize("case,pad,offset", [((3, 7, 5, 2), 3, 1), ((3, 7, 5, 2), 2, 2), ((2, 53, 5, 1), 5, 1), ((16, 86, 3, 2), 1, 1)],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else str(v))
def test_padded_and_misaligned_stack(hw, case, pad, offset, pool):
    """a view with dim-0 stride R*C + pad whose base sits ``offset`` floats into its buffer: an odd stride or an odd offset forbids the
    8-byte loads of the C == 2 path, (pad 2, offset 2) keeps them on a padded stack.  Same bits as the contiguous stack."""
    n_clips, n_q, n_options, c = case
    stack, refs = _random_case(case)
    rows = n_q * n_options
    stride = rows * c + pad
    buf = torch.full((offset + n_clips * stride,), float("nan"))           # (a read of the padding would poison the scores)
    view = buf[offset:].as_strided((n_clips, rows, c), (stride, c, 1))
    view.copy_(stack)
    dev_view = hw(buf)[offset:].as_strided((n_clips, rows, c), (stride, c, 1))
    assert dev_view.data_ptr() % 8 == (4 * offset) % 8 and dev_view.stride(0) == stride
    scores, pred = ops.mc_predict(dev_view, n_options, MODES[pool])
    want_scores, want_pred = ops.mc_predict(hw(stack), n_options, MODES[pool])
    assert torch.equal(scores.cpu(), want_scores.cpu()) and torch.equal(pred.cpu(), want_pred.cpu())
    assert float((scores.cpu().double() - refs[pool][0]).abs().max()) <= R.score_bound(stack)
    assert torch.equal(pred.cpu().long(), refs[pool][1])
    # the stride handed over explicitly means the same
    scores2, pred2 = ops.mc_predict(dev_view, n_options, MODES[pool], clip_stride=stride)
    assert torch.equal(scores2.cpu(), scores.cpu()) and torch.equal(pred2.cpu(), pred.cpu())


def test_nan_counts_as_the_largest_score(hw):
    """torch.max: a NaN beats every number, the first NaN wins"""
    stack = torch.tensor([[[0.5], [float("nan")], [3.0], [float("nan")], [1.0], [2.0]]])          # (1, 6, 1): two groups of 3
    scores, pred = _run(hw, stack, 3, "mean")
    ref_scores, ref_pred = R.mc_scores(stack, 3, "mean")
    assert pred.tolist() == ref_pred.tolist() == [1, 0]
    assert torch.isnan(scores).tolist() == torch.isnan(ref_scores).tolist()


def test_error_paths(hw):
    ok = hw(torch.zeros(2, 10, 2))
    with pytest.raises(RuntimeError, match="cb_mc_predict: C must be 1 or 2"):
        ops.mc_predict(hw(torch.zeros(2, 10, 3)), 5, ops.AGG_MEAN)
    with pytest.raises(ValueError, match="not a multiple of n_options"):
        ops.mc_predict(ok, 4, ops.AGG_MEAN)
    with pytest.raises(RuntimeError, match="cb_mc_predict: clip_stride 19 is smaller than"):
        ops.mc_predict(ok, 5, ops.AGG_MEAN, clip_stride=19)
    with pytest.raises(RuntimeError, match="cb_mc_predict: unknown mode 7"):
        ops.mc_predict(ok, 5, 7)
    with pytest.raises(ValueError, match="fp32"):
        ops.mc_predict(ok.double(), 5, ops.AGG_MEAN)


def test_refuses_cpu_tensors_on_the_product_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mc_predict(torch.zeros(1, 5, 2), 5, ops.AGG_MEAN)


def test_abi_entry():
    from clipbert_amd import _lib
    assert _lib.get().cb_version() >= 16 and "cb_mc_predict" in _lib.EXPORTED_SYMBOLS
    assert (ops.AGG_MEAN, ops.AGG_MAX, ops.AGG_LSE) == (0, 1, 2)
