// Pooling of one class's per-clip logits and the arg-max order of the answer kernels (mc.hip, qa.hip): ONE copy of the arithmetic, so that
// cb_mc_predict and cb_qa_predict pool to the same bits.  The arithmetic of clip_agg_fwd_kernel (misc.hip).
#pragma once
#include "common.h"

constexpr int kMcNone = 0x7fffffff;                           // "no candidate seen yet": every real index beats it

// running maximum m and sum s of one class over the clips
__device__ __forceinline__ void pool_begin(float v, float& m, float& s) { m = v; s = v; }
__device__ __forceinline__ void pool_add(float v, float& m, float& s) {
    m = v > m || v != v ? v : m;                              // (a NaN stays a NaN: torch.max propagates it)
    s += v;
}

// the pooled logit from (m, s); x[k * clip_stride] is clip k of the class (read again by the log-sum-exp only)
__device__ __forceinline__ float pool_finish(float m, float s, const float* x, int64_t clip_stride, int n_clips, int mode) {
    if (mode == CB_AGG_MEAN) return s / (float)n_clips;
    if (mode == CB_AGG_MAX) return m;
    if (!(fabsf(m) <= 3.0e38f)) return m;                     // an infinite or NaN maximum is the result (torch.logsumexp)
    float e = 0.f;                                            // log-sum-exp over the clips, shifted by their maximum (a second pass: a few KB, cache-resident)
    for (int k = 0; k < n_clips; ++k) e += expf(x[(int64_t)k * clip_stride] - m);
    return m + logf(e);
}

// does (bm, bi) replace (am, ai)?  The larger score; among equals the lower index; a NaN is larger than any number (torch.max).
__device__ __forceinline__ bool mc_better(float am, int ai, float bm, int bi) {
    if (bi == kMcNone) return false;
    if (ai == kMcNone) return true;
    const bool an = am != am, bn = bm != bm;
    if (an || bn) return bn && (!an || bi < ai);
    return bm > am || (bm == am && bi < ai);
}

// the best (score, index) of a wave in every lane
__device__ __forceinline__ void wave_best(float& bm, int& bi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(bm, off);
        const int oi = __shfl_xor(bi, off);
        if (mc_better(bm, bi, om, oi)) {
            bm = om;
            bi = oi;
        }
    }
}
