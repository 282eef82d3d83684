// Image-VQA head over SPARSE answers: the row sum of the BCE-with-logits loss, the arg-max and the VQA soft accuracy of the arg-max in one
// pass over the fp32 logits (rows, C), and a backward that writes the classifier GEMMs' A operand directly in the compute dtype.  The
// soft targets stay what the annotations are -- at most K (answer id, score) slots per question -- and are never scattered into a
// (rows, C) matrix.
#include "common.h"

namespace {

constexpr int kVqaThreads = 256;
constexpr int kVqaWaves = kVqaThreads / 64;
constexpr int kVqaMaxK = 32;
constexpr float kNegHuge = -3.0e38f;
constexpr int kNoIndex = 0x7fffffff;

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the softplus of head_loss_kernel's BCE (misc.hip): max(x, 0) + log1p(exp(-|x|))
__device__ __forceinline__ float softplusf_(float x) { return fmaxf(x, 0.f) + log1pf(__expf(-fabsf(x))); }

// the row's K slots into LDS; a padding slot (id outside [0, C)) becomes id -1, score 0: it matches no column
__device__ __forceinline__ void load_slots(const int32_t* ans_ids, const float* ans_scores, int r, int K, int C, int tid, int* s_id, float* s_sc) {
    if (tid < K) {
        const int a = ans_ids[(int64_t)r * K + tid];
        const bool ok = a >= 0 && a < C;
        s_id[tid] = ok ? a : -1;
        s_sc[tid] = ok ? ans_scores[(int64_t)r * K + tid] : 0.f;
    }
    __syncthreads();
}

struct Best {
    float m;
    int i;
};
__device__ __forceinline__ void best_merge(Best& a, float bm, int bi) {
    if (bm > a.m || (bm == a.m && bi < a.i)) {                // (the lowest index wins ties, as torch.max documents)
        a.m = bm;
        a.i = bi;
    }
}
__device__ __forceinline__ void best_add(Best& a, float x, int c) {     // (c ascends within a thread: strict > keeps the lowest index)
    if (x > a.m) {
        a.m = x;
        a.i = c;
    }
}

// one workgroup per row, ONE pass over the row
__global__ void __launch_bounds__(kVqaThreads) vqa_loss_fwd_kernel(const float* logits, int64_t ld, const int32_t* ans_ids,
                                                                   const float* ans_scores, int K, int C, float* loss_rows,
                                                                   int64_t* pred_rows, float* pred_score) {
    __shared__ int s_id[kVqaMaxK];
    __shared__ float s_sc[kVqaMaxK];
    __shared__ float red_m[kVqaWaves], red_s[kVqaWaves], red_t[kVqaWaves];
    __shared__ int red_i[kVqaWaves];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    load_slots(ans_ids, ans_scores, r, K, C, tid, s_id, s_sc);
    const float* x = logits + (int64_t)r * ld;
    Best a = {kNegHuge, kNoIndex};
    float sp = 0.f;                                           // this thread's share of sum_c softplus(x_c)
    if (aligned16(x)) {
        const int C4 = C & ~3;
        for (int c = tid * 4; c < C4; c += kVqaThreads * 4) {
            const f32x4 v = load4(x + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) best_add(a, v[e], c + e);
            sp += (softplusf_(v[0]) + softplusf_(v[1])) + (softplusf_(v[2]) + softplusf_(v[3]));
        }
        const int c = C4 + tid;                               // the last C % 4 columns
        if (c < C) {
            const float v = x[c];
            best_add(a, v, c);
            sp += softplusf_(v);
        }
    } else {
        for (int c = tid; c < C; c += kVqaThreads) {
            const float v = x[c];
            best_add(a, v, c);
            sp += softplusf_(v);
        }
    }
    float tgt = 0.f;                                          // s_k x[a_k] of slot k = tid (the K <= 32 slots all sit in wave 0)
    if (tid < K && s_id[tid] >= 0) tgt = s_sc[tid] * x[s_id[tid]];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float bm = __shfl_xor(a.m, o);
        const int bi = __shfl_xor(a.i, o);
        best_merge(a, bm, bi);
    }
    sp = wave_sum(sp);
    tgt = wave_sum(tgt);
    if (lane == 0) {
        red_m[wave] = a.m; red_i[wave] = a.i; red_s[wave] = sp; red_t[wave] = tgt;
    }
    __syncthreads();
    if (tid == 0) {
        float s = red_s[0], t = red_t[0];
        for (int w = 1; w < kVqaWaves; ++w) {
            best_merge(a, red_m[w], red_i[w]);
            s += red_s[w];
            t += red_t[w];
        }
        float hit = 0.f;                                      // the soft accuracy of the prediction: 0 when it is none of the answers
        for (int k = 0; k < K; ++k)
            if (s_id[k] == a.i) hit += s_sc[k];
        loss_rows[r] = s - t;
        pred_rows[r] = a.i;
        pred_score[r] = hit;
    }
}

__device__ __forceinline__ void store1(float* p, float v) { *p = v; }
__device__ __forceinline__ void store1(bf16* p, float v) { *p = (bf16)v; }

// dlogits[r, c] = dloss * (sigmoid(x) - t[c]) in T, fp32 arithmetic rounded once; t[c] = the scores of the row's slots that name column c,
// looked up in the K slots (LDS, every lane reads the same word) per vector of four columns; the columns C..ldd-1 get zeros
template <typename T>
__global__ void __launch_bounds__(kVqaThreads) vqa_loss_bwd_kernel(const float* logits, int64_t ld, const int32_t* ans_ids,
                                                                   const float* ans_scores, int K, const float* dloss_rows, T* dlogits,
                                                                   int64_t ldd, int C) {
    __shared__ int s_id[kVqaMaxK];
    __shared__ float s_sc[kVqaMaxK];
    const int r = blockIdx.x, tid = threadIdx.x;
    load_slots(ans_ids, ans_scores, r, K, C, tid, s_id, s_sc);
    const float* x = logits + (int64_t)r * ld;
    T* dl = dlogits + (int64_t)r * ldd;
    const float g = dloss_rows[r];
    const bool vec = aligned16(x) && (reinterpret_cast<uintptr_t>(dl) & (4 * sizeof(T) - 1)) == 0;
    const int Cv = vec ? (C & ~3) : 0;
    for (int c = tid * 4; c < Cv; c += kVqaThreads * 4) {
        const f32x4 v = load4(x + c);
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < K; ++k) {
            const int d = s_id[k] - c;
            if ((unsigned)d < 4u) {
                const float s = s_sc[k];
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] += d == e ? s : 0.f;
            }
        }
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = g * (sigmoidf_(v[e]) - t[e]);
        store4(dl + c, o);
    }
    for (int64_t c = Cv + tid; c < ldd; c += kVqaThreads) {  // scalar path / the last C % 4 columns / the pad columns (never read from x)
        float o = 0.f;
        if (c < C) {
            float t = 0.f;
            for (int k = 0; k < K; ++k)
                if (s_id[k] == (int)c) t += s_sc[k];
            o = g * (sigmoidf_(x[c]) - t);
        }
        store1(dl + c, o);
    }
}

}  // namespace

extern "C" int cb_vqa_loss_fwd(const float* logits, int64_t ld, const int32_t* ans_ids, const float* ans_scores, int32_t K, int32_t rows,
                               int32_t C, float* loss_rows, int64_t* pred_rows, float* pred_score, void* stream) {
    CB_REQUIRE(rows >= 0 && C > 0 && ld >= C && K >= 1 && K <= kVqaMaxK, "cb_vqa_loss_fwd: bad shape (rows %d, C %d, ld %lld, K %d: 1..%d)", rows,
               C, (long long)ld, K, kVqaMaxK);
    if (rows == 0) return 0;
    CB_REQUIRE(logits && ans_ids && ans_scores && loss_rows && pred_rows && pred_score, "cb_vqa_loss_fwd: null pointer");
    hipLaunchKernelGGL(vqa_loss_fwd_kernel, dim3(rows), dim3(kVqaThreads), 0, cb_stream(stream), logits, ld, ans_ids, ans_scores, K, C,
                       loss_rows, pred_rows, pred_score);
    return cb_launch_status("cb_vqa_loss_fwd");
}

extern "C" int cb_vqa_loss_bwd(int32_t dtype, const float* logits, int64_t ld, const int32_t* ans_ids, const float* ans_scores, int32_t K,
                               const float* dloss_rows, void* dlogits, int64_t ldd, int32_t rows, int32_t C, void* stream) {
    CB_REQUIRE(rows >= 0 && C > 0 && ld >= C && ldd >= C && K >= 1 && K <= kVqaMaxK,
               "cb_vqa_loss_bwd: bad shape (rows %d, C %d, ld %lld, ldd %lld, K %d: 1..%d)", rows, C, (long long)ld, (long long)ldd, K, kVqaMaxK);
    CB_REQUIRE(dtype == CB_BF16 || dtype == CB_F32, "cb_vqa_loss_bwd: bad dtype");
    if (rows == 0) return 0;
    CB_REQUIRE(logits && ans_ids && ans_scores && dloss_rows && dlogits, "cb_vqa_loss_bwd: null pointer");
    const dim3 g(rows), b(kVqaThreads);
    if (dtype == CB_BF16)
        hipLaunchKernelGGL((vqa_loss_bwd_kernel<bf16>), g, b, 0, cb_stream(stream), logits, ld, ans_ids, ans_scores, K, dloss_rows,
                           (bf16*)dlogits, ldd, C);
    else
        hipLaunchKernelGGL((vqa_loss_bwd_kernel<float>), g, b, 0, cb_stream(stream), logits, ld, ans_ids, ans_scores, K, dloss_rows,
                           (float*)dlogits, ldd, C);
    return cb_launch_status("cb_vqa_loss_bwd");
}
