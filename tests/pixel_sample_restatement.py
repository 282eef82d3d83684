"""The device-side pixel sub-sampling (cb_pixel_sample, include/clipbert_hip.h) restated in NumPy integer arithmetic, written from the
definition in the header:

    s      = (seed + *seed_ptr) mod 2^64                              (dropout_restatement.effective_seed)
    key_i  = (hash64(s, i) & ~0xFFFF) | i            for i in [0, Lv)   (dropout_restatement.hash64: the splitmix64 finaliser)
    sample = sort(argsort(key)[:n])                                   (all keys differ: the index sits in the low 16 bits)

Nothing of clipbert_amd is imported at module level; site_sample alone reads modeling.runtime (the seed of the model's site).
Helper module: no tests in here."""
import numpy as np

from dropout_restatement import effective_seed, hash64

_LOW16 = np.uint64(0xFFFF)


def keys(seed: int, lv: int) -> np.ndarray:
    """uint64 (lv,): the sort keys under the EFFECTIVE seed"""
    assert 1 <= lv <= 65536
    i = np.arange(lv, dtype=np.uint64)
    return (hash64(seed, i) & ~_LOW16) | i


def sample(seed: int, lv: int, n: int) -> np.ndarray:
    """int32 (n,): the n indices with the smallest keys, ascending.  ``seed`` is the effective seed."""
    assert 1 <= n <= lv
    k = keys(seed, lv)
    assert np.unique(k).size == lv
    return np.sort(np.argsort(k, kind="stable")[:n]).astype(np.int32)


def site_sample(fwd_i: int, seed_word: int, lv: int, n: int) -> np.ndarray:
    """the selection of the model's fwd_i-th forward under the device seed word ``seed_word``"""
    from clipbert_amd.modeling.runtime import _SITE_PIXEL, _seed
    return sample(effective_seed(_seed(_SITE_PIXEL, 0, fwd_i), seed_word), lv, n)
