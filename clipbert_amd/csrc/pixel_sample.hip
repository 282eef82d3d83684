// Random pixel sub-sampling of the visual tokens (pre-training, training phase: modeling.py:15-34, 80-88) drawn on the DEVICE: a uniformly
// random n-subset of {0..Lv-1} in ascending order, from the same stateless hash and seed convention as the dropout masks -- one launch,
// no host randomness, no scratch, so that a captured step draws a fresh selection per replay (the graph advances the seed word).
//
//   s     = seed + *seed_ptr                                   (mod 2^64)
//   key_i = (cb_hash64(s, i) & ~0xFFFF) | i                    (48 random bits over the index: all keys differ)
//   sel   = the n indices with the smallest keys, ascending
#include "common.h"

namespace {

constexpr int kPsThreads = 256;          // == the number of radix bins: thread b owns bin b of the histogram
constexpr int kPsWaves = kPsThreads / 64;

__device__ __forceinline__ uint64_t ps_key(uint64_t s, int i) { return (cb_hash64(s, (uint64_t)i) & ~0xFFFFull) | (uint64_t)i; }

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ int ps_wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl(v, lane >= o ? lane - o : 0);
        if (lane >= o) v += t;
    }
    return v;
}

// inclusive prefix sum over the workgroup (v of thread tid); `tot` is rewritten: barriers on both sides
__device__ __forceinline__ int ps_block_scan_incl(int v, int lane, int wave, int* tot, int& total) {
    const int incl = ps_wave_scan_incl(v, lane);
    if (lane == 63) tot[wave] = incl;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kPsWaves; ++w) {
        if (w < wave) base += tot[w];
        total += tot[w];
    }
    __syncthreads();
    return base + incl;
}

// ONE workgroup.  Radix select of the n-th smallest key, 8 bits per pass from the top: a 256-bin LDS histogram of the keys that match
// the prefix found so far (keys are hashed again each pass, never stored), a workgroup scan of the bins, and the bin that holds the n-th
// key extends the prefix.  As soon as the keys up to and including that bin are exactly n, the prefix decides membership and the passes
// stop -- at the latest after the eighth, where a bin is a single key.  Then an ordered compaction, blockDim indices per chunk.
__global__ void __launch_bounds__(kPsThreads) pixel_sample_kernel(int32_t* sel, int Lv, int n, uint64_t seed, const uint64_t* seed_ptr) {
    __shared__ int hist[kPsThreads];
    __shared__ int tot[kPsWaves];
    __shared__ int pick[3];                                  // the chosen bin, keys left to find below it, 1 = membership is decided
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t s = seed + (seed_ptr ? *seed_ptr : 0ull);
    uint64_t prefix = 0;                                     // the top bits of the n-th smallest key, (key >> shift) form
    int shift = 64, need = n;                                // `need`: rank of that key among the keys sharing its prefix
    if (n == Lv) {                                           // everything is kept
        shift = 0;
        prefix = ~0ull;
    }
    while (shift > 0) {
        const int above = shift;                             // bits [above, 64) are fixed
        shift -= 8;
        hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < Lv; i += kPsThreads) {
            const uint64_t k = ps_key(s, i);
            if (above == 64 || (k >> above) == prefix) atomicAdd(&hist[(int)((k >> shift) & 0xFF)], 1);
        }
        __syncthreads();
        const int h = hist[tid];
        int total;
        const int incl = ps_block_scan_incl(h, lane, wave, tot, total);
        if (incl >= need && incl - h < need) {               // exactly one bin: the first whose running count reaches `need`
            pick[0] = tid;
            pick[1] = need - (incl - h);
            pick[2] = incl == need ? 1 : 0;
        }
        __syncthreads();
        prefix = (prefix << 8) | (uint64_t)pick[0];
        need = pick[1];
        if (pick[2]) break;                                  // (at shift 0 a bin is one key: always set there)
    }
    int running = 0;
    for (int i0 = 0; i0 < Lv && running < n; i0 += kPsThreads) {
        const int i = i0 + tid;
        const int flag = (i < Lv && (ps_key(s, i) >> shift) <= prefix) ? 1 : 0;
        int total;
        const int incl = ps_block_scan_incl(flag, lane, wave, tot, total);
        const int j = running + incl - flag;
        if (flag && j < n) sel[j] = i;
        running += total;
    }
}

}  // namespace

extern "C" int cb_pixel_sample(int32_t* sel, int32_t Lv, int32_t n, uint64_t seed, const uint64_t* seed_ptr, void* stream) {
    CB_REQUIRE(sel, "cb_pixel_sample: null pointer");
    CB_REQUIRE(n >= 1 && n <= Lv && Lv <= 65536, "cb_pixel_sample: need 1 <= n <= Lv <= 65536 (n %d, Lv %d)", n, Lv);
    hipLaunchKernelGGL(pixel_sample_kernel, dim3(1), dim3(kPsThreads), 0, cb_stream(stream), sel, Lv, n, seed, seed_ptr);
    return cb_launch_status("cb_pixel_sample");
}
