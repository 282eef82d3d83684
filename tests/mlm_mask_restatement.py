"""The device-side masked-LM token masking (cb_mlm_mask, include/clipbert_hip.h) restated in NumPy integer arithmetic, written from the
definition in the header.  For element i = r * Lt + t of a padded (rows, Lt) int64 id matrix:

    s        = (seed + *seed_ptr) mod 2^64                                   (dropout_restatement.effective_seed)
    z        = hash64(s, i)                                                  (dropout_restatement.hash64: the splitmix64 finaliser)
    eligible = ids[i] is none of the special ids and ids[i] != pad_id        (pad_id None or negative: no pad token)
    labelled = eligible and (z >> 40) < uint32(float32(p) * 16777216)
    kind     = (((z >> 24) & 0xFFFF) * 10) >> 16                             (0..7 [MASK], 8 a random word, 9 unchanged)
    word     = ((z & 0xFFFFFF) * V) >> 24
    ids_out  = labelled ? (kind <= 7 ? mask_id : kind == 8 ? word : ids) : ids
    labels   = labelled ? ids : ignore_index

Nothing of clipbert_amd is imported at module level; site_mask alone reads modeling.runtime (the seed of the model's site).
Helper module: no tests in here."""
import numpy as np

from dropout_restatement import effective_seed, hash64


def threshold(p: float) -> int:
    """the float32 product p * 2^24 truncated to uint32"""
    return int(np.uint32(np.float32(p) * np.float32(16777216.0)))


def fields(seed: int, n: int):
    """(the 24-bit label draw, kind 0..9, the 24-bit word draw) of elements 0..n-1 under the EFFECTIVE seed, uint64 each"""
    z = hash64(seed, np.arange(n, dtype=np.uint64))
    kind = (((z >> np.uint64(24)) & np.uint64(0xFFFF)) * np.uint64(10)) >> np.uint64(16)
    return z >> np.uint64(40), kind, z & np.uint64(0xFFFFFF)


def mask(ids: np.ndarray, p: float, seed: int, vocab_size: int, special_ids=(101, 102), pad_id=0, mask_id=103, ignore_index=-100):
    """-> (ids_out, labels), int64 arrays of ids' shape.  ``seed`` is the effective seed."""
    ids = np.asarray(ids, dtype=np.int64)
    assert 1 <= vocab_size <= 1 << 24 and len(special_ids) <= 4
    flat = ids.reshape(-1)
    draw, kind, low = fields(seed, flat.size)
    eligible = np.ones(flat.shape, dtype=bool)
    for s in special_ids:
        eligible &= flat != s
    if pad_id is not None and pad_id >= 0:
        eligible &= flat != pad_id
    labelled = eligible & (draw < np.uint64(threshold(p)))
    word = ((low * np.uint64(vocab_size)) >> np.uint64(24)).astype(np.int64)
    repl = np.where(kind <= 7, np.int64(mask_id), np.where(kind == 8, word, flat))
    out = np.where(labelled, repl, flat)
    labels = np.where(labelled, flat, np.int64(ignore_index))
    return out.reshape(ids.shape), labels.reshape(ids.shape)


def site_seed(fwd_i: int, seed_word: int = 0) -> int:
    """the effective seed of the model's masking site at forward (or validation batch) ``fwd_i`` under the device word ``seed_word``"""
    from clipbert_amd.modeling.runtime import _SITE_MLM, _seed
    return effective_seed(_seed(_SITE_MLM, 0, fwd_i), seed_word)


def site_mask(ids: np.ndarray, p: float, fwd_i: int, seed_word: int, vocab_size: int, **kw):
    """the masking of the model's fwd_i-th forward under the device seed word ``seed_word``"""
    return mask(ids, p, site_seed(fwd_i, seed_word), vocab_size, **kw)
