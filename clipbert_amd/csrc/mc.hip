// MSRVTT multiple-choice scoring (src/tasks/run_msrvtt_mc.py:172-195): the clip pooling, the row's probability and the arg-max over each
// question's options in ONE launch over the fp32 stack of per-clip logits -- in place of the pooling, logsumexp, softmax and max launches
// and the per-clip device-to-host copies of the runner.
#include "clip_pool.h"

namespace {

constexpr int kMcThreads = 256;
constexpr int kMcWaves = kMcThreads / 64;

__device__ __forceinline__ bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// sigmoid(d) without an overflowing exponential: z = exp(-|d|) <= 1
__device__ __forceinline__ float mc_sigmoid(float d) {
    const float z = expf(-fabsf(d));
    return (d >= 0.f ? 1.0f : z) / (1.0f + z);
}

// the probability of one row: pool per class over the clips, then softmax[1] = sigmoid(p1 - p0) (C == 2) or sigmoid(p0) (C == 1)
template <int C>
__device__ __forceinline__ float mc_row_score(const float* x, int64_t clip_stride, int n_clips, int mode, bool vec) {
    float m[C], s[C];
    for (int k = 0; k < n_clips; ++k) {
        const float* p = x + (int64_t)k * clip_stride;
        float v[C];
        if (C == 2 && vec) {
            const f32x2 t = *reinterpret_cast<const f32x2*>(p);
            v[0] = t[0];
            v[C - 1] = t[1];
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = p[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (k == 0) pool_begin(v[c], m[c], s[c]);
            else pool_add(v[c], m[c], s[c]);
        }
    }
    float pooled[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        pooled[c] = pool_finish(m[c], s[c], x + c, clip_stride, n_clips, mode);                      // (clip_pool.h: shared with qa.hip)
    }
    return mc_sigmoid(C == 2 ? pooled[C - 1] - pooled[0] : pooled[0]);
}

// one WAVE per question, kMcWaves questions per workgroup; the lanes stride over the options, so a group of any size stays inside its wave
template <int C>
__global__ void __launch_bounds__(kMcThreads) mc_predict_kernel(const float* logits, int64_t clip_stride, int n_clips, int n_q, int n_options,
                                                               int mode, float* scores, int32_t* pred) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * kMcWaves + wave;
    if (q >= n_q) return;                                     // (the whole wave leaves: no barrier in this kernel)
    const bool vec = C == 2 && aligned8(logits) && (clip_stride & 1) == 0;       // every row's pair then sits on 8 bytes
    const int64_t r0 = q * n_options;
    float bm = 0.f;
    int bi = kMcNone;
    for (int o = lane; o < n_options; o += 64) {
        const float sc = mc_row_score<C>(logits + (r0 + o) * C, clip_stride, n_clips, mode, vec);
        scores[r0 + o] = sc;
        if (mc_better(bm, bi, sc, o)) {
            bm = sc;
            bi = o;
        }
    }
    wave_best(bm, bi);
    if (lane == 0) pred[q] = bi;
}

}  // namespace

extern "C" int cb_mc_predict(const float* logits, int64_t clip_stride, int32_t n_clips, int32_t n_q, int32_t n_options, int32_t C, int32_t mode,
                             float* scores, int32_t* pred, void* stream) {
    CB_REQUIRE(C == 1 || C == 2, "cb_mc_predict: C must be 1 or 2 (got %d)", C);
    CB_REQUIRE(mode >= CB_AGG_MEAN && mode <= CB_AGG_LSE, "cb_mc_predict: unknown mode %d", mode);
    CB_REQUIRE(n_clips > 0 && n_q > 0 && n_options > 0, "cb_mc_predict: bad counts (n_clips %d, n_q %d, n_options %d: all must be positive)",
               n_clips, n_q, n_options);
    CB_REQUIRE(clip_stride >= (int64_t)n_q * n_options * C, "cb_mc_predict: clip_stride %lld is smaller than n_q * n_options * C = %lld",
               (long long)clip_stride, (long long)n_q * n_options * C);
    CB_REQUIRE(logits && scores && pred, "cb_mc_predict: null pointer");
    const dim3 g((unsigned)(((int64_t)n_q + kMcWaves - 1) / kMcWaves)), b(kMcThreads);
    if (C == 2)
        hipLaunchKernelGGL((mc_predict_kernel<2>), g, b, 0, cb_stream(stream), logits, clip_stride, n_clips, n_q, n_options, mode, scores, pred);
    else
        hipLaunchKernelGGL((mc_predict_kernel<1>), g, b, 0, cb_stream(stream), logits, clip_stride, n_clips, n_q, n_options, mode, scores, pred);
    return cb_launch_status("cb_mc_predict");
}
