"""cb_retrieval_rank through ops.retrieval_rank -- the exact integer keys of the rounded retrieval scores and the rank of every query's
ground truth -- against the NumPy restatement (retrieval_rank_restatement.py), on the host emulator and on the GPU, and
tasks.eval_retrieval_matrix against the reference's eval_retrieval executed from its source.  Every comparison is integer or ==
equality: the keys are exact (the product float64(p) * 1e4 is), the rank is a count.

The tie rule is the kernel's own -- a stable descending sort -- because the reference's torch.sort(descending=True) without stable=True
defines none (DESIGN.md "Retrieval evaluation on the device"): tie-heavy inputs are held to the stable restatement, the reference is
asked only about inputs that are tie-free by construction."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import retrieval_rank_restatement as R
from clipbert_amd import _lib, ops, tasks
from oracle import ref_functions, ref_shim

live = pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")

# (n_rows, n_cols): one element; fewer candidates than a vector / a wave either way round; exactly one wave of queries and of candidates; a
# second workgroup on both axes with a partial wave and rows whose 16-byte cut moves (ld 130); several workgroups, more than one vector
# per lane, an odd ld
SHAPES = [(1, 1), (5, 7), (7, 5), (64, 64), (65, 130), (300, 257)]
AXES = {"rows": ops.RANK_ROW_QUERIES, "cols": ops.RANK_COL_QUERIES}
TIE_VALUES = np.array([0.0, 0.00005, 0.1234, 0.5, 0.99995, 1.0], dtype=np.float32)      # six scores with six different keys


def _ids(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _n_queries(shape, axis):
    return shape[1] if axis == ops.RANK_COL_QUERIES else shape[0]


def _n_candidates(shape, axis):
    return shape[0] if axis == ops.RANK_COL_QUERIES else shape[1]


@functools.lru_cache(maxsize=None)
def _tie_case(shape):
    """tie-heavy scores of the shape and, per axis, a random ground truth and its restated ranks: computed once, never written to"""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    scores = TIE_VALUES[rng.integers(0, len(TIE_VALUES), shape)]
    per_axis = {}
    for axis in AXES.values():
        gt = rng.integers(0, _n_candidates(shape, axis), _n_queries(shape, axis)).astype(np.int32)
        want = R.ranks_by_counting(scores, gt, axis)
        assert np.array_equal(want, R.ranks_by_stable_sort(scores, gt, axis))          # the two statements of the rule agree
        per_axis[axis] = (gt, want)
    return scores, R.keys(scores), per_axis


def _device_view(hw, scores, pad=0, offset=0):
    """the matrix as a view with row stride n_cols + pad whose base sits ``offset`` floats into a NaN-filled buffer (a read of the padding
    would turn into the largest key and poison the ranks)"""
    n_rows, n_cols = scores.shape
    ld = n_cols + pad
    buf = torch.full((offset + n_rows * ld + 1,), float("nan"))
    buf[offset:].as_strided((n_rows, n_cols), (ld, 1)).copy_(torch.from_numpy(np.ascontiguousarray(scores)))
    dev = hw(buf)
    view = dev[offset:].as_strided((n_rows, n_cols), (ld, 1))
    assert view.data_ptr() == dev.data_ptr() + 4 * offset and dev.data_ptr() % 16 == 0
    return view


def _rank(hw, scores, gt, axis, want_keys=False, **view):
    out = ops.retrieval_rank(_device_view(hw, scores, **view), hw(torch.from_numpy(np.asarray(gt, dtype=np.int32))), axis, want_keys=want_keys)
    rank, keys = out if want_keys else (out, None)
    assert rank.dtype == torch.int32 and tuple(rank.shape) == (_n_queries(scores.shape, axis),)
    if want_keys:
        assert keys.dtype == torch.int32 and tuple(keys.shape) == tuple(scores.shape) and keys.is_contiguous()
        return rank.cpu().numpy().astype(np.int64), keys.cpu().numpy().astype(np.int64)
    return rank.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("pad", [0, 3], ids=["dense", "padded"])
@pytest.mark.parametrize("axis", list(AXES), ids=list(AXES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_tie_heavy_ranks_and_keys_equal_the_restatement(hw, shape, axis, pad, offset):
    scores, want_keys, per_axis = _tie_case(shape)
    gt, want = per_axis[AXES[axis]]
    rank, keys = _rank(hw, scores, gt, AXES[axis], want_keys=True, pad=pad, offset=offset)
    assert np.array_equal(keys, want_keys)
    assert np.array_equal(rank, want)
    assert np.array_equal(_rank(hw, scores, gt, AXES[axis], pad=pad, offset=offset), want)      # (without the key matrix: the same ranks)


def _boundary_scores():
    ks = np.arange(0, 10000, 31, dtype=np.float64)                                  # 323 of the 10^4 rounding boundaries
    mid = ((ks + 0.5) / 1e4).astype(np.float32)
    parts = [np.arange(0, 33, dtype=np.float32) / 32,                               # every m / 32: exactly representable, 1/32 -> 0.0312 (half-even)
             mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1)),
             np.array([0.0, -0.0, 1.0, 1e-45, -1e-45, 1e-40, 1.1754944e-38, 0.99999994, 3e5, -3e5, np.inf, -np.inf, 3.4e38], dtype=np.float32)]
    return np.concatenate(parts)


def test_boundary_scores_give_exact_keys(hw):
    """the halves, both fp32 neighbours of every sampled (k + 0.5) / 1e4, 0, 1, denormals and the saturating values: the kernel's key is
    the restatement's, and for every score inside [0, 1] it is Python's round(p, 4) -- the reference's expression (:687) -- as an integer"""
    vals = _boundary_scores()
    n = len(vals)
    scores = np.stack([vals, vals[::-1], np.roll(vals, 7)])                         # (3, n): row queries see them contiguous, column queries strided
    want = R.keys(scores)
    for axis in AXES.values():
        gt = np.zeros(_n_queries(scores.shape, axis), dtype=np.int32)
        rank, keys = _rank(hw, scores, gt, axis, want_keys=True, offset=1)
        assert np.array_equal(keys, want)
        assert np.array_equal(rank, R.ranks_by_counting(scores, gt, axis))
    for p, k in zip(vals.tolist(), want[0].tolist()):
        if 0.0 <= p <= 1.0:
            assert k / 1e4 == round(p, 4), (p, k)
    assert want[0][:5].tolist() == [0, 312, 625, 938, 1250]                         # 1/32 = 0.03125 -> 0.0312, 3/32 = 0.09375 -> 0.0938
    assert want[0][n - 5:].tolist() == [2000000000, -2000000000, 2000000000, -2000000000, 2000000000]


def test_nan_ranks_first(hw):
    """torch.sort(descending=True) puts a NaN before every number; two NaNs keep their index order"""
    nan = float("nan")
    scores = np.array([[0.5, nan, 0.9, 0.1],
                       [nan, 0.2, nan, 1.0],
                       [0.3, 0.3, 0.3, nan]], dtype=np.float32)
    for gt, want in (([1, 0, 3], [1, 1, 1]), ([2, 2, 0], [2, 2, 2]), ([0, 3, 2], [3, 3, 4])):
        assert _rank(hw, scores, gt, ops.RANK_ROW_QUERIES).tolist() == want == R.ranks_by_stable_sort(scores, gt, ops.RANK_ROW_QUERIES).tolist()
    gt = [2, 0, 0, 1]                                        # the columns: a number below a NaN and a number; the NaN; two numbers below the NaN
    want = R.ranks_by_counting(scores, gt, ops.RANK_COL_QUERIES)
    rank, keys = _rank(hw, scores, gt, ops.RANK_COL_QUERIES, want_keys=True)
    assert rank.tolist() == want.tolist() == [3, 1, 2, 2]
    assert keys[0].tolist() == [5000, 2 ** 31 - 1, 9000, 1000]


@pytest.mark.parametrize("axis", list(AXES), ids=list(AXES))
def test_ground_truth_at_the_ends_and_out_of_range(hw, axis):
    """gt at candidate 0 and at the last candidate; gt outside the candidates gives rank 0, nothing is read through it and the neighbouring
    queries keep their ranks"""
    shape = (65, 130)
    scores, _, per_axis = _tie_case(shape)
    base_gt, base_want = per_axis[AXES[axis]]
    n_q, n_cand = _n_queries(shape, AXES[axis]), _n_candidates(shape, AXES[axis])
    for fill in (0, n_cand - 1):
        gt = np.full(n_q, fill, dtype=np.int32)
        assert np.array_equal(_rank(hw, scores, gt, AXES[axis], pad=3), R.ranks_by_counting(scores, gt, AXES[axis]))
    gt = base_gt.copy()
    bad = {0: -1, 1: n_cand, 5: 2 ** 31 - 1, n_q // 2: -2 ** 31, n_q - 1: n_cand + 64}
    for q, g in bad.items():
        gt[q] = g
    rank, keys = _rank(hw, scores, gt, AXES[axis], want_keys=True, pad=3, offset=1)
    want = base_want.copy()
    want[list(bad)] = 0
    assert np.array_equal(rank, want) and np.array_equal(rank, R.ranks_by_counting(scores, gt, AXES[axis]))
    assert np.array_equal(keys, R.keys(scores))              # (the keys of a query without a ground truth are still written)
    assert np.array_equal(_rank(hw, scores, gt, AXES[axis], pad=3, offset=1), want)


def test_empty_sizes(hw):
    for shape in ((0, 5), (4, 0), (0, 0)):
        for axis in AXES.values():
            n_q = _n_queries(shape, axis)
            rank, keys = ops.retrieval_rank(hw(torch.zeros(shape)), hw(torch.zeros(n_q, dtype=torch.int32)), axis, want_keys=True)
            assert tuple(keys.shape) == shape and rank.cpu().tolist() == [0] * n_q          # no candidates: every rank is 0


def test_error_paths(hw):
    ok, gt5, gt7 = hw(torch.zeros(5, 7)), hw(torch.zeros(5, dtype=torch.int32)), hw(torch.zeros(7, dtype=torch.int32))
    assert ops.retrieval_rank(ok, gt5, ops.RANK_ROW_QUERIES).cpu().tolist() == [1] * 5
    assert ops.retrieval_rank(ok, gt7, ops.RANK_COL_QUERIES).cpu().tolist() == [1] * 7
    with pytest.raises(ValueError, match="fp32"):
        ops.retrieval_rank(ok.double(), gt5, ops.RANK_ROW_QUERIES)
    with pytest.raises(ValueError, match="fp32"):
        ops.retrieval_rank(ok.view(-1), gt5, ops.RANK_ROW_QUERIES)
    with pytest.raises(ValueError, match="last dimension"):
        ops.retrieval_rank(hw(torch.zeros(7, 5)).t(), gt5, ops.RANK_ROW_QUERIES)
    with pytest.raises(ValueError, match="gt must be 5 contiguous"):
        ops.retrieval_rank(ok, gt7, ops.RANK_ROW_QUERIES)
    with pytest.raises(ValueError, match="gt must be 7 contiguous"):
        ops.retrieval_rank(ok, gt5, ops.RANK_COL_QUERIES)
    with pytest.raises(ValueError, match="gt must be"):
        ops.retrieval_rank(ok, gt5.long(), ops.RANK_ROW_QUERIES)
    with pytest.raises(ValueError, match="overlap"):
        ops.retrieval_rank(ok.as_strided((5, 7), (6, 1)), gt5, ops.RANK_ROW_QUERIES)
    with pytest.raises(RuntimeError, match="cb_retrieval_rank: unknown axis 7"):
        ops.retrieval_rank(ok, gt5, 7)
    # what the wrapper never lets through: the entry point's own checks (each returns before anything is launched or dereferenced)
    lib, rank, keys = _lib.get(), hw(torch.zeros(7, dtype=torch.int32)), hw(torch.zeros(5, 7, dtype=torch.int32))
    p = lambda t: ctypes.c_void_p(t.data_ptr())             # noqa: E731
    for args, msg in (((p(ok), 6, 5, 7, 0, p(gt5), p(rank), None, 0), "ld 6 is smaller than n_cols = 7"),
                      ((p(ok), 7, 5, 7, 0, p(gt5), p(rank), p(keys), 6), "the keys' ld 6 is smaller than n_cols = 7"),
                      ((p(ok), 7, -1, 7, 0, p(gt5), p(rank), None, 0), "negative size"),
                      ((p(ok), 7, 5, -7, 1, p(gt5), p(rank), None, 0), "negative size"),
                      ((p(ok), 7, 5, 7, 2, p(gt5), p(rank), None, 0), "unknown axis 2"),
                      ((None, 7, 5, 7, 0, p(gt5), p(rank), None, 0), "null pointer"),
                      ((p(ok), 7, 5, 7, 0, None, p(rank), None, 0), "null pointer"),
                      ((p(ok), 7, 5, 7, 1, p(gt7), None, None, 0), "null pointer")):
        assert lib.cb_retrieval_rank(*args, None) != 0
        assert msg in lib.cb_last_error().decode(), (msg, lib.cb_last_error().decode())
    assert lib.cb_retrieval_rank(None, 7, 0, 7, 0, None, None, None, 0, None) == 0           # no queries: legal, nothing to do


def test_refuses_cpu_tensors_on_the_product_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.retrieval_rank(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32), ops.RANK_ROW_QUERIES)


def test_abi_entry():
    assert _lib.get().cb_version() >= 19 and "cb_retrieval_rank" in _lib.EXPORTED_SYMBOLS
    assert (ops.RANK_ROW_QUERIES, ops.RANK_COL_QUERIES) == (R.ROW_QUERIES, R.COL_QUERIES) == (0, 1)


def test_rounding_to_4_places_is_exact_in_integers():
    """CPU only, no kernel: for 2e5 fp32 values -- uniform, saturated sigmoids, every m / 32, and all three of x and its two fp32 neighbours
    for x = (k + 0.5) / 1e4, every k -- Python's round(float(p), 4), the reference's expression (:687), is rint(float64(p) * 1e4) / 1e4"""
    rng = np.random.default_rng(7)
    mid = ((np.arange(10000, dtype=np.float64) + 0.5) / 1e4).astype(np.float32)
    sig = (1.0 / (1.0 + np.exp(-rng.normal(0, 8, 60000)))).astype(np.float32)       # most of them within 1e-4 of 0 or 1
    vals = np.concatenate([rng.random(110000, dtype=np.float32), sig, np.arange(0, 33, dtype=np.float32) / 32,
                           mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1))])
    assert len(vals) >= 200000
    k = np.rint(vals.astype(np.float64) * 1e4)
    assert np.array_equal(k, R.keys(vals))
    assert (k / 1e4).tolist() == [round(p, 4) for p in vals.tolist()]


# ---- the reference's eval_retrieval, executed from its source, on tie-free matrices ---------------------------------------------------
def _tie_free_matrix(n_videos, n_captions, seed):
    """S = float32(perm / 1e4), perm a permutation of 0 .. n_videos * n_captions - 1 (<= 10^4 of them): the keys are perm itself"""
    assert n_videos * n_captions <= 10000
    perm = np.random.default_rng(seed).permutation(n_videos * n_captions).reshape(n_videos, n_captions)
    return (perm / 1e4).astype(np.float32), perm


@live
@pytest.mark.parametrize("n_videos,n_captions", [(7, 9), (7, 14), (100, 100)], ids=["9x7", "7x14", "100x100"])
def test_metrics_equal_the_reference_eval_retrieval_run_from_source(emul, n_videos, n_captions):
    """(9, 7): nine captions over seven videos (two videos own two captions; the reference's video -> text direction needs a caption for every
    video, so the nine cannot be the videos); (7, 14): two captions per video; (100, 100): one each, rows longer than the 16 candidates up
    to which the reference's unstable sort happens to be stable -- immaterial here, the keys are pairwise distinct (asserted)."""
    scores, perm = _tie_free_matrix(n_videos, n_captions, seed=n_videos + n_captions)
    assert len(np.unique(R.keys(scores))) == scores.size and np.array_equal(R.keys(scores), perm)
    vid_ids, txt_ids = [f"video{i}" for i in range(n_videos)], [f"cap{j}" for j in range(n_captions)]
    gt = {t: vid_ids[(3 * j + 1) % n_videos] for j, t in enumerate(txt_ids)}
    assert set(gt.values()) == set(vid_ids)
    matrix = tasks.RetrievalMatrix(vid_ids, txt_ids, torch.from_numpy(scores))
    rows = tasks.retrieval_rows(matrix)
    assert len(rows) == scores.size and rows[1] == dict(vid_id="video0", txt_id="cap1", score=int(perm[0, 1]) / 1e4)
    want = ref_functions.retrieval_metric_functions()["eval_retrieval"](rows, gt, None)
    got = tasks.eval_retrieval_matrix(matrix, gt)
    assert got["text2video"] == want["text2video"] and got["video2text"] == want["video2text"]
    assert set(got) == set(want) and all(type(v) is float for m in got.values() for v in m.values())
    assert got == tasks.eval_retrieval(rows, gt)             # (and the existing host path, tie-free)
