// Video-QA validation (src/tasks/run_video_qa.py:241-279 and the loss it accumulates at :250-259): the clip pooling, the answer -- arg-max
// over the classes, or round-and-clamp of the count regression -- and the per-question loss in ONE launch over the fp32 stack of per-clip
// logits, in place of the pooling / logsumexp / max launches, the per-clip loss launches and the per-clip device-to-host copies of the
// runner.  No atomics and no workspace: what leaves the kernel is per question, so every sum over questions is formed later in a fixed order.
//
// C <= 64: one WAVE per question (lane c owns class c), four questions per workgroup, no barrier.
// C  > 64: one 256-thread workgroup per question, lanes striding over the classes so that every clip's row is read coalesced.  The loss makes
// TWO SWEEPS over the question's n_clips x C tile instead of staging it in LDS: sweep 1 takes each clip's maximum (exact: no rounding), sweep
// 2 the sum of the shifted exponentials.  The frameqa tile (16 clips x 1540 classes) is 96 KB: staged, it would hold a workgroup per CU and
// would bound n_clips * C by the LDS size; swept, it is read from L2 / L1 (the first sweep put it there), LDS holds 8 floats per clip, and
// the only bound is n_clips <= kQaMaxClips.  A plain sum per lane, a shuffle tree per wave and a two-level merge of the four waves also keep the
// rounding analysis of the tests short: ceil(C / 256) + 8 additions feed each clip's sum of exponentials.
#include "clip_pool.h"

namespace {

constexpr int kQaThreads = 256;
constexpr int kQaWaves = kQaThreads / 64;
constexpr int kQaSmallC = 64;                                 // up to here a wave holds a question's classes, one per lane
constexpr int kQaMaxClips = 256;                              // C > 64: per-clip statistics of the four waves live in LDS

// the count answer (:278): (pooled + 0.5).long().clamp(1, 10) -- truncation toward zero; clamped as a float first, so that the conversion
// never sees a value outside int32 (a NaN leaves fmaxf as 1)
__device__ __forceinline__ int qa_count_answer(float pooled) {
    return (int)fminf(fmaxf(truncf(pooled + 0.5f), 1.0f), 10.0f);
}

__device__ __forceinline__ float qa_nan() { return __builtin_nanf(""); }

// one WAVE per question; lane c holds class c (lanes >= C hold nothing)
__global__ void __launch_bounds__(kQaThreads) qa_predict_wave_kernel(const float* logits, int64_t clip_stride, int n_clips, int n_q, int C, int mode,
                                                                    int kind, const void* labels, int32_t* pred, float* loss, float* pooled_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * kQaWaves + wave;
    if (q >= n_q) return;                                     // (the whole wave leaves: no barrier in this kernel)
    const bool own = lane < C;
    const float* x = logits + q * C + (own ? lane : 0);       // (idle lanes read class 0 and drop it)
    float m, s;
    for (int k = 0; k < n_clips; ++k) {
        const float v = x[(int64_t)k * clip_stride];
        if (k == 0) pool_begin(v, m, s);
        else pool_add(v, m, s);
    }
    const float pooled = pool_finish(m, s, x, clip_stride, n_clips, mode);
    if (own && pooled_out) pooled_out[q * C + lane] = pooled;
    if (kind == CB_QA_COUNT) {                                // C == 1: lane 0 is the question
        if (lane != 0) return;
        pred[q] = qa_count_answer(pooled);
        if (loss) {
            const float y = static_cast<const float*>(labels)[q];
            float acc = 0.f;
            for (int k = 0; k < n_clips; ++k) {
                const float d = x[(int64_t)k * clip_stride] - y;
                acc += d * d;
            }
            loss[q] = acc / (float)n_clips;
        }
        return;
    }
    float bm = own ? pooled : 0.f;
    int bi = own ? lane : kMcNone;
    wave_best(bm, bi);
    if (lane == 0) pred[q] = bi;
    if (!loss) return;
    const int label = static_cast<const int32_t*>(labels)[q];
    const bool label_ok = label >= 0 && label < C;            // (a label outside the classes: the loss is NaN, nothing is read for it)
    float acc = 0.f;
    for (int k = 0; k < n_clips; ++k) {                       // cross entropy of clip k: logsumexp_c x[k, :] - x[k, label], max-shifted
        const float v = own ? x[(int64_t)k * clip_stride] : -INFINITY;
        const float mk = wave_max(v);
        const float sk = wave_sum(own ? expf(v - mk) : 0.f);
        const float at = __shfl(v, label_ok ? label : 0);
        acc += (mk + logf(sk)) - at;
    }
    if (lane == 0) loss[q] = label_ok ? acc / (float)n_clips : qa_nan();
}

// one WORKGROUP per question; thread t owns classes t, t + 256, ...
__global__ void __launch_bounds__(kQaThreads) qa_predict_block_kernel(const float* logits, int64_t clip_stride, int n_clips, int C, int mode,
                                                                     const int32_t* labels, int32_t* pred, float* loss, float* pooled_out) {
    __shared__ float s_max[kQaMaxClips * kQaWaves];           // [clip][wave]: the wave's maximum of the clip's row
    __shared__ float s_sum[kQaMaxClips * kQaWaves];           // [clip][wave]: the wave's sum of exp(x - the clip's maximum)
    __shared__ float s_bm[kQaWaves];
    __shared__ int s_bi[kQaWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const float* x = logits + q * C;
    float bm = 0.f;
    int bi = kMcNone;
    for (int c = tid; c < C; c += kQaThreads) {               // pooling: ascending classes per thread, consecutive classes across the lanes
        float m, s;
        for (int k = 0; k < n_clips; ++k) {
            const float v = x[(int64_t)k * clip_stride + c];
            if (k == 0) pool_begin(v, m, s);
            else pool_add(v, m, s);
        }
        const float pooled = pool_finish(m, s, x + c, clip_stride, n_clips, mode);
        if (pooled_out) pooled_out[q * C + c] = pooled;
        if (mc_better(bm, bi, pooled, c)) {
            bm = pooled;
            bi = c;
        }
    }
    wave_best(bm, bi);
    if (lane == 0) {
        s_bm[wave] = bm;
        s_bi[wave] = bi;
    }
    if (loss) {                                               // sweep 1 (uniform branch): each clip's maximum over this wave's classes
        for (int k = 0; k < n_clips; ++k) {
            const float* row = x + (int64_t)k * clip_stride;
            float mk = -INFINITY;
            for (int c = tid; c < C; c += kQaThreads) mk = fmaxf(mk, row[c]);
            mk = wave_max(mk);
            if (lane == 0) s_max[k * kQaWaves + wave] = mk;
        }
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kQaWaves; ++w)
            if (mc_better(bm, bi, s_bm[w], s_bi[w])) {
                bm = s_bm[w];
                bi = s_bi[w];
            }
        pred[q] = bi;
    }
    if (!loss) return;
    for (int k = 0; k < n_clips; ++k) {                       // sweep 2: the sum of exponentials shifted by the clip's maximum
        const float* row = x + (int64_t)k * clip_stride;
        const float* pm = s_max + k * kQaWaves;
        const float mk = fmaxf(fmaxf(pm[0], pm[1]), fmaxf(pm[2], pm[3]));
        float sk = 0.f;
        for (int c = tid; c < C; c += kQaThreads) sk += expf(row[c] - mk);
        sk = wave_sum(sk);
        if (lane == 0) s_sum[k * kQaWaves + wave] = sk;
    }
    __syncthreads();
    if (tid != 0) return;
    const int label = labels[q];
    if (label < 0 || label >= C) {                            // (a label outside the classes: the loss is NaN, nothing is read for it)
        loss[q] = qa_nan();
        return;
    }
    float acc = 0.f;
    for (int k = 0; k < n_clips; ++k) {                       // the clips in index order: a fixed order of additions
        const float* pm = s_max + k * kQaWaves;
        const float* ps = s_sum + k * kQaWaves;
        const float mk = fmaxf(fmaxf(pm[0], pm[1]), fmaxf(pm[2], pm[3]));
        const float sk = (ps[0] + ps[1]) + (ps[2] + ps[3]);
        acc += (mk + logf(sk)) - x[(int64_t)k * clip_stride + label];
    }
    loss[q] = acc / (float)n_clips;
}

}  // namespace

extern "C" int cb_qa_predict(const float* logits, int64_t clip_stride, int32_t n_clips, int32_t n_q, int32_t C, int32_t mode, int32_t kind,
                             const void* labels, int32_t* pred, float* loss, float* pooled, void* stream) {
    CB_REQUIRE(mode >= CB_AGG_MEAN && mode <= CB_AGG_LSE, "cb_qa_predict: unknown mode %d", mode);
    CB_REQUIRE(kind == CB_QA_CLASSIFY || kind == CB_QA_COUNT, "cb_qa_predict: unknown kind %d", kind);
    CB_REQUIRE(n_clips > 0 && n_q > 0 && C > 0, "cb_qa_predict: bad counts (n_clips %d, n_q %d, C %d: all must be positive)", n_clips, n_q, C);
    CB_REQUIRE(kind != CB_QA_COUNT || C == 1, "cb_qa_predict: kind count needs C == 1 (got %d)", C);
    CB_REQUIRE(clip_stride >= (int64_t)n_q * C, "cb_qa_predict: clip_stride %lld is smaller than n_q * C = %lld", (long long)clip_stride,
               (long long)n_q * C);
    CB_REQUIRE(logits && pred, "cb_qa_predict: null pointer (logits %p, pred %p)", (const void*)logits, (void*)pred);
    if (!labels) loss = nullptr;                              // (no labels, no loss: nothing is written there)
    if (C <= kQaSmallC) {
        const dim3 g((unsigned)(((int64_t)n_q + kQaWaves - 1) / kQaWaves)), b(kQaThreads);
        hipLaunchKernelGGL(qa_predict_wave_kernel, g, b, 0, cb_stream(stream), logits, clip_stride, n_clips, n_q, C, mode, kind, labels, pred, loss,
                           pooled);
    } else {
        CB_REQUIRE(!loss || n_clips <= kQaMaxClips, "cb_qa_predict: the loss over C = %d > %d classes takes at most %d clips (got %d)", C, kQaSmallC,
                   kQaMaxClips, n_clips);
        hipLaunchKernelGGL(qa_predict_block_kernel, dim3((unsigned)n_q), dim3(kQaThreads), 0, cb_stream(stream), logits, clip_stride, n_clips, C, mode,
                           static_cast<const int32_t*>(labels), pred, loss, pooled);
    }
    return cb_launch_status("cb_qa_predict");
}
