// Masked-LM head over the LABELLED text rows only: device-side compaction of the labelled rows (no host read of the count) and the
// softmax cross-entropy / arg-max of the compact (cap, V) logits, whose backward writes the decoder GEMMs' A operand directly in the
// compute dtype.  The GEMMs between them are cb_gemm's gather / row-map modes.
#include "common.h"

namespace {

constexpr int kMlmThreads = 256;
constexpr int kMlmWaves = kMlmThreads / 64;
constexpr float kNegHuge = -3.0e38f;
constexpr int kNoIndex = 0x7fffffff;

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl(v, lane >= o ? lane - o : 0);
        if (lane >= o) v += t;
    }
    return v;
}

// ONE workgroup walks the rows in chunks of its size: per chunk a wave scan of the "labelled" flags, the wave totals through LDS,
// and a running base -- slots come out in ascending row order whatever the chunking.
__global__ void __launch_bounds__(kMlmThreads) mlm_select_kernel(const int64_t* labels, int64_t ignore_index, int rows, int Lt, int L, int d,
                                                                 int V, int cap, int32_t* slot_row, int64_t* slot_label, cb_pixel* tab,
                                                                 int32_t* rowmap, int64_t* counts, float* loss_rows, int64_t* pred_rows) {
    __shared__ int wave_tot[kMlmWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int running = 0;
    for (int r0 = 0; r0 < rows; r0 += kMlmThreads) {
        const int r = r0 + tid;
        int64_t y = ignore_index;
        if (r < rows) {
            y = labels[r];
            loss_rows[r] = 0.f;
            pred_rows[r] = -100;
        }
        const int flag = (r < rows && y != ignore_index && y >= 0 && y < (int64_t)V) ? 1 : 0;      // (an out-of-range label counts as ignored)
        const int incl = wave_scan_incl(flag, lane);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int base = running, total = 0;
#pragma unroll
        for (int w = 0; w < kMlmWaves; ++w) {
            if (w < wave) base += wave_tot[w];
            total += wave_tot[w];
        }
        const int j = base + incl - flag;
        if (flag && j < cap) {
            const int b = r / Lt, t = r - b * Lt;
            const int srow = b * L + t;                      // the row of (b, t) in the (B, L, d) sequence buffer
            slot_row[j] = r;
            slot_label[j] = y;
            cb_pixel px;
            px.off = srow * d;
            px.ih0 = 0;
            px.iw0 = (int16_t)t;
            tab[j] = px;
            rowmap[j] = srow;
        }
        running += total;
        __syncthreads();                                     // (wave_tot is rewritten by the next chunk)
    }
    const int kept = running < cap ? running : cap;
    const int dump = (rows / Lt) * L;                        // the extra row behind the B * L real ones
    for (int j = kept + tid; j < cap; j += kMlmThreads) {
        slot_row[j] = -1;
        slot_label[j] = ignore_index;
        cb_pixel px;
        px.off = 0;                                          // valid memory, and ih0 = -1 fails the gather's bounds test: the row reads as zeros
        px.ih0 = -1;
        px.iw0 = 0;
        tab[j] = px;
        rowmap[j] = dump;
    }
    if (tid == 0) {
        counts[0] = running;
        if (running > cap) counts[1] += running - cap;
    }
}

// running softmax statistics of the elements a thread (then a wave, then the workgroup) has seen: s = sum exp(x - m), i = first index of m
struct Online {
    float m, s;
    int i;
};
__device__ __forceinline__ void online_merge(Online& a, float bm, float bs, int bi) {
    const bool take = bm > a.m || (bm == a.m && bi < a.i);   // (the lowest index wins ties, as torch.max documents)
    const float M = fmaxf(a.m, bm);
    a.s = a.s * __expf(a.m - M) + bs * __expf(bm - M);
    a.m = M;
    if (take) a.i = bi;
}
__device__ __forceinline__ void online_add4(Online& a, f32x4 v, int c) {
    float vm = v[0];
    int vi = 0;
#pragma unroll
    for (int e = 1; e < 4; ++e)
        if (v[e] > vm) { vm = v[e]; vi = e; }
    if (vm > a.m) {                                          // (c ascends within a thread: strict > keeps the lowest index)
        a.s *= __expf(a.m - vm);
        a.m = vm;
        a.i = c + vi;
    }
    a.s += (__expf(v[0] - a.m) + __expf(v[1] - a.m)) + (__expf(v[2] - a.m) + __expf(v[3] - a.m));
}
__device__ __forceinline__ void online_add1(Online& a, float x, int c) {
    if (x > a.m) {
        a.s = a.s * __expf(a.m - x) + 1.0f;
        a.m = x;
        a.i = c;
    } else {
        a.s += __expf(x - a.m);
    }
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// one workgroup per slot, ONE pass over the row
__global__ void __launch_bounds__(kMlmThreads) mlm_loss_fwd_kernel(const float* logits, int64_t ld, const int32_t* slot_row,
                                                                   const int64_t* slot_label, int64_t ignore_index, int V, float* lse,
                                                                   float* loss_rows, int64_t* pred_rows) {
    __shared__ float red_m[kMlmWaves], red_s[kMlmWaves], red_t[kMlmWaves];
    __shared__ int red_i[kMlmWaves];
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t y = slot_label[j];
    if (y == ignore_index || y < 0 || y >= (int64_t)V) return;          // padding slot (uniform over the workgroup): writes nothing
    const float* x = logits + (int64_t)j * ld;
    const int label = (int)y;
    Online a = {kNegHuge, 0.f, kNoIndex};
    float tgt = 0.f;                                          // x[label]: exactly one thread meets it
    if (aligned16(x)) {
        const int V4 = V & ~3;
        for (int c = tid * 4; c < V4; c += kMlmThreads * 4) {
            const f32x4 v = load4(x + c);
            online_add4(a, v, c);
            if ((unsigned)(label - c) < 4u) tgt = v[label - c];
        }
        const int c = V4 + tid;                               // the last V % 4 columns
        if (c < V) {
            const float v = x[c];
            online_add1(a, v, c);
            if (c == label) tgt = v;
        }
    } else {
        for (int c = tid; c < V; c += kMlmThreads) {
            const float v = x[c];
            online_add1(a, v, c);
            if (c == label) tgt = v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float bm = __shfl_xor(a.m, o), bs = __shfl_xor(a.s, o);
        const int bi = __shfl_xor(a.i, o);
        online_merge(a, bm, bs, bi);
    }
    tgt = wave_sum(tgt);                                      // (zeros everywhere but at the one thread)
    if (lane == 0) {
        red_m[wave] = a.m; red_s[wave] = a.s; red_i[wave] = a.i; red_t[wave] = tgt;
    }
    __syncthreads();
    if (tid == 0) {
        float t = red_t[0];
        for (int w = 1; w < kMlmWaves; ++w) {
            online_merge(a, red_m[w], red_s[w], red_i[w]);
            t += red_t[w];
        }
        const float l = a.m + __logf(a.s);
        const int r = slot_row[j];
        lse[j] = l;
        loss_rows[r] = l - t;
        pred_rows[r] = a.i;
    }
}

__device__ __forceinline__ void store1(float* p, float v) { *p = v; }
__device__ __forceinline__ void store1(bf16* p, float v) { *p = (bf16)v; }

// dlogits[j, c] = dloss * (exp(x - lse) - [c == label]) in T, fp32 arithmetic rounded once; padding slots and the columns V..ldd-1 get zeros
template <typename T>
__global__ void __launch_bounds__(kMlmThreads) mlm_loss_bwd_kernel(const float* logits, int64_t ld, const float* lse, const int32_t* slot_row,
                                                                   const int64_t* slot_label, int64_t ignore_index, const float* dloss_rows,
                                                                   T* dlogits, int64_t ldd, int V) {
    const int j = blockIdx.x, tid = threadIdx.x;
    const int64_t y = slot_label[j];
    const bool pad = (y == ignore_index || y < 0 || y >= (int64_t)V);
    const float* x = logits + (int64_t)j * ld;
    T* dl = dlogits + (int64_t)j * ldd;
    const int label = pad ? -1 : (int)y;
    const float g = pad ? 0.f : dloss_rows[slot_row[j]];
    const float l = pad ? 0.f : lse[j];
    const bool vec = aligned16(x) && (reinterpret_cast<uintptr_t>(dl) & (4 * sizeof(T) - 1)) == 0;
    const int Vv = vec ? (V & ~3) : 0;
    if (pad) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int c = tid * 4; c < Vv; c += kMlmThreads * 4) store4(dl + c, z);
    } else {
        for (int c = tid * 4; c < Vv; c += kMlmThreads * 4) {
            const f32x4 v = load4(x + c);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = g * (__expf(v[e] - l) - (c + e == label ? 1.0f : 0.0f));
            store4(dl + c, o);
        }
    }
    for (int64_t c = Vv + tid; c < ldd; c += kMlmThreads) {  // scalar path / the last V % 4 columns / the pad columns (never read from x)
        float o = 0.f;
        if (!pad && c < V) o = g * (__expf(x[c] - l) - ((int)c == label ? 1.0f : 0.0f));
        store1(dl + c, o);
    }
}

}  // namespace

extern "C" int cb_mlm_select(const int64_t* labels, int64_t ignore_index, int32_t rows, int32_t Lt, int32_t L, int32_t d, int32_t V,
                             int32_t cap, int32_t* slot_row, int64_t* slot_label, cb_pixel* tab, int32_t* c_rowmap, int64_t* counts,
                             float* loss_rows, int64_t* pred_rows, void* stream) {
    CB_REQUIRE(labels && slot_row && slot_label && tab && c_rowmap && counts && loss_rows && pred_rows, "cb_mlm_select: null pointer");
    CB_REQUIRE(rows >= 0 && Lt > 0 && Lt <= 32767 && L >= Lt && d > 0 && V > 0 && cap > 0 && rows % Lt == 0,
               "cb_mlm_select: bad shape (rows %d, Lt %d, L %d, d %d, V %d, cap %d)", rows, Lt, L, d, V, cap);
    CB_REQUIRE(((int64_t)(rows / Lt) * L + 1) * d < ((int64_t)1 << 31), "cb_mlm_select: the sequence buffer exceeds the table's 32-bit offsets");
    hipLaunchKernelGGL(mlm_select_kernel, dim3(1), dim3(kMlmThreads), 0, cb_stream(stream), labels, ignore_index, rows, Lt, L, d, V, cap,
                       slot_row, slot_label, tab, c_rowmap, counts, loss_rows, pred_rows);
    return cb_launch_status("cb_mlm_select");
}

extern "C" int cb_mlm_loss_fwd(const float* logits, int64_t ld, const int32_t* slot_row, const int64_t* slot_label, int64_t ignore_index,
                               int32_t cap, int32_t V, float* lse, float* loss_rows, int64_t* pred_rows, void* stream) {
    CB_REQUIRE(logits && slot_row && slot_label && lse && loss_rows && pred_rows, "cb_mlm_loss_fwd: null pointer");
    CB_REQUIRE(cap > 0 && V > 0 && ld >= V, "cb_mlm_loss_fwd: bad shape (cap %d, V %d, ld %lld)", cap, V, (long long)ld);
    hipLaunchKernelGGL(mlm_loss_fwd_kernel, dim3(cap), dim3(kMlmThreads), 0, cb_stream(stream), logits, ld, slot_row, slot_label,
                       ignore_index, V, lse, loss_rows, pred_rows);
    return cb_launch_status("cb_mlm_loss_fwd");
}

extern "C" int cb_mlm_loss_bwd(int32_t dtype, const float* logits, int64_t ld, const float* lse, const int32_t* slot_row,
                               const int64_t* slot_label, int64_t ignore_index, const float* dloss_rows, void* dlogits, int64_t ldd,
                               int32_t cap, int32_t V, void* stream) {
    CB_REQUIRE(logits && lse && slot_row && slot_label && dloss_rows && dlogits, "cb_mlm_loss_bwd: null pointer");
    CB_REQUIRE(cap > 0 && V > 0 && ld >= V && ldd >= V, "cb_mlm_loss_bwd: bad shape (cap %d, V %d, ld %lld, ldd %lld)", cap, V, (long long)ld,
               (long long)ldd);
    const dim3 g(cap), b(kMlmThreads);
    if (dtype == CB_BF16)
        hipLaunchKernelGGL((mlm_loss_bwd_kernel<bf16>), g, b, 0, cb_stream(stream), logits, ld, lse, slot_row, slot_label, ignore_index,
                           dloss_rows, (bf16*)dlogits, ldd, V);
    else if (dtype == CB_F32)
        hipLaunchKernelGGL((mlm_loss_bwd_kernel<float>), g, b, 0, cb_stream(stream), logits, ld, lse, slot_row, slot_label, ignore_index,
                           dloss_rows, (float*)dlogits, ldd, V);
    else
        return cb_fail("cb_mlm_loss_bwd: bad dtype");
    return cb_launch_status("cb_mlm_loss_bwd");
}
