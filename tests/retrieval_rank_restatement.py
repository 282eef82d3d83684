"""NumPy restatement of cb_retrieval_rank (include/clipbert_hip.h): the exact integer keys of the scores rounded to 4 places
(src/tasks/run_video_retrieval.py:687) and the rank of every query's ground truth in a STABLE descending sort of them (:546-560; the
reference's torch.sort leaves the order of equal scores undefined, DESIGN.md "Retrieval evaluation on the device").  Two statements of the
rank: the counting formula, and torch.sort(..., descending=True, stable=True) as a cross-check."""
import numpy as np
import torch

ROW_QUERIES, COL_QUERIES = 0, 1
INT32_MAX = np.int64(2 ** 31 - 1)


def keys(scores) -> np.ndarray:
    """int64 (same shape): rint(float64(p) * 1e4), round-half-even (the product is exact), saturated at +-2e9; a NaN is INT32_MAX"""
    s = np.asarray(scores, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.clip(np.rint(s.astype(np.float64) * 1e4), -2.0e9, 2.0e9)
    return np.where(np.isnan(s), INT32_MAX, np.nan_to_num(k, nan=0.0).astype(np.int64))


def _query_major(scores, axis):
    k = keys(scores)
    return k.T if axis == COL_QUERIES else k


def ranks_by_counting(scores, gt, axis) -> np.ndarray:
    """rank[q] = 1 + #{c: key[q, c] > key[q, gt[q]]} + #{c < gt[q]: key[q, c] == key[q, gt[q]]}; gt[q] outside the candidates: 0"""
    k = _query_major(scores, axis)
    n_q, n_cand = k.shape
    out = np.zeros(n_q, dtype=np.int64)
    for q, g in enumerate(np.asarray(gt, dtype=np.int64)):
        if 0 <= g < n_cand:
            out[q] = 1 + int((k[q] > k[q, g]).sum()) + int((k[q, :g] == k[q, g]).sum())
    return out


def ranks_by_stable_sort(scores, gt, axis) -> np.ndarray:
    """the position of gt[q] in torch.sort(keys, dim=1, descending=True, stable=True), 1-based; gt[q] outside the candidates: 0"""
    k = torch.from_numpy(np.ascontiguousarray(_query_major(scores, axis)))
    n_q, n_cand = k.shape
    out = np.zeros(n_q, dtype=np.int64)
    if n_cand == 0:
        return out
    order = torch.sort(k, dim=1, descending=True, stable=True)[1].numpy()
    for q, g in enumerate(np.asarray(gt, dtype=np.int64)):
        if 0 <= g < n_cand:
            out[q] = 1 + int(np.nonzero(order[q] == g)[0][0])
    return out
