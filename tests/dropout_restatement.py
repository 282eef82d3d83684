"""The product's stateless dropout mask restated in NumPy integer arithmetic, written from the comment block and the three helpers
of clipbert_amd/csrc/common.h (cb_hash64, dropout_threshold, dropout_mult4 / dropout_mult1) -- the yardstick of every test that
holds a dropout site to an fp64 reference built from the SAME mask:

    group      = row * ceil(cols / 4) + col // 4                  (a flat stream of n elements is rows = 1, cols = n)
    z          = splitmix64-finaliser(seed + group * 0x9E3779B97F4A7C15)            (all arithmetic mod 2^64)
    kept       iff ((z >> 16 * (col % 4)) & 0xffff) >= uint32(float32(p) * 65536)
    multiplier = float32(1) / (float32(1) - float32(p)) where kept, 0 where dropped
    seed       = (dropout_seed + *seed_ptr) mod 2^64

Attention probabilities: rows = B * H * L with row (b * H + h) * L + i, cols = L.  For cols % 4 == 0 the 2-D and the flat form coincide.
Nothing of clipbert_amd is imported at module level; site_mask alone reads modeling.runtime._seed (the seed of a model site).
Helper module: no tests in here."""
import numpy as np
import torch

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def effective_seed(dropout_seed: int, seed_word: int = 0) -> int:
    """what the kernels hash with: the host seed plus the device word behind seed_ptr, mod 2^64"""
    return (int(dropout_seed) + int(seed_word)) % (1 << 64)


def hash64(seed: int, idx: np.ndarray) -> np.ndarray:
    """cb_hash64 on an array of group indices"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed % (1 << 64)) + idx.astype(np.uint64) * _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def threshold(p: float) -> int:
    """dropout_threshold: the float32 product p * 65536 truncated to uint32"""
    return int(np.uint32(np.float32(p) * np.float32(65536.0)))


def multiplier(p: float) -> float:
    """the float32 value a kept element is multiplied by"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(seed: int, rows: int, cols: int, p: float) -> torch.Tensor:
    """bool (rows, cols): True where the element survives.  ``seed`` is the effective seed."""
    r = np.arange(rows, dtype=np.uint64).reshape(rows, 1)
    c = np.arange(cols, dtype=np.uint64).reshape(1, cols)
    group = r * np.uint64((cols + 3) // 4) + (c >> np.uint64(2))
    z = hash64(seed, group)
    bits = (z >> (np.uint64(16) * (c & np.uint64(3)))) & np.uint64(0xFFFF)
    return torch.from_numpy(bits >= np.uint64(threshold(p)))


def mult_mask(seed: int, rows: int, cols: int, p: float, dtype=torch.float64) -> torch.Tensor:
    """(rows, cols) of 0 / multiplier(p): what a site multiplies its values by"""
    return keep_mask(seed, rows, cols, p).to(dtype) * multiplier(p)


def attention_mult(seed: int, B: int, H: int, L: int, p: float, dtype=torch.float64) -> torch.Tensor:
    """(B, H, L, L) multipliers of the attention probabilities: row (b * H + h) * L + i of a (B * H * L, L) site"""
    return mult_mask(seed, B * H * L, L, p, dtype).view(B, H, L, L)


def site_mask(site: int, layer: int, fwd_i: int, seed_word: int, shape, p: float, dtype=torch.float32) -> torch.Tensor:
    """multipliers of one dropout site of the model, shaped like the tensor the site drops.  The attention site (B, H, L, L) is the
    2-D form above; every other site is a contiguous (..., d) tensor whose last dimension is the site's column count."""
    from clipbert_amd.modeling.runtime import _SITE_ATTN, _seed
    seed = effective_seed(_seed(site, layer, fwd_i), seed_word)
    shape = tuple(int(s) for s in shape)
    if site == _SITE_ATTN:
        b, h, l, l2 = shape
        assert l == l2
        return attention_mult(seed, b, h, l, p, dtype)
    cols = shape[-1]
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    return mult_mask(seed, rows, cols, p, dtype).view(shape)
