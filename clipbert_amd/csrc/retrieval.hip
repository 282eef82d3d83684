// Retrieval evaluation (src/tasks/run_video_retrieval.py:546-560 get_retrieval_scores, on the scores rounded at :687): the rank of every query's
// ground-truth candidate in the video-major score matrix S (one row per video, one column per caption), in ONE launch per direction, in place
// of the million dict rows, the rebuilt matrix and the two CPU sorts of the runner.
//
// Exact in integers.  key(p) = rint(double(p) * 1e4), round-half-even: the product is exact (a 24-bit significand times 10^4 = 2^4 * 625 needs
// at most 34 bits), so the key is the integer Python's round(float(p), 4) rounds to, and ordering the keys is ordering the rounded scores.  The
// key saturates at +-2e9; a NaN becomes INT32_MAX (torch.sort(descending=True) puts a NaN first).  No sort: the rank of candidate g is
// 1 + #{c: key[c] > key[g]} + #{c < g: key[c] == key[g]} -- the position a STABLE descending sort gives it (the reference's torch.sort leaves
// the order of equal scores undefined; DESIGN.md "Retrieval evaluation on the device").  A count is a sum of integers: no atomics, no
// workspace, and nothing depends on the order of execution.
//
// Two kernels behind one entry point, both reading S coalesced:
//   CB_RANK_ROW_QUERIES (video -> text: a query's candidates are contiguous).  One WAVE per query, four queries per workgroup, no barrier.
//     The row is cut at its 16-byte boundaries: up to 3 leading floats (lane i reads float i), the aligned body as f32x4 per lane, lanes
//     striding over the vectors (1 KiB per wave instruction), up to 3 trailing floats.  A row whose base is only 4-byte aligned, or an ld
//     that is no multiple of 4, only moves the cut: there is no separate misaligned kernel.  The lanes' counts meet in a shuffle tree.
//   CB_RANK_COL_QUERIES (text -> video: a query's candidates are ld apart, adjacent queries are adjacent floats).  A workgroup owns 64
//     adjacent queries -- lane l of every wave owns query 64 b + l -- and its four waves share out the rows (wave w walks rows w, w + 4, ...),
//     so every load of a wave is 256 contiguous bytes.  The four partial counts of a query meet in LDS (1 KiB) behind one barrier.
// The 10^6 scores of an MSRVTT 1k-A evaluation are 4 MB read once per direction: each launch is a few microseconds of memory traffic and
// is bound by its launch.  Not tuned beyond coalescing.
#include "common.h"

namespace {

constexpr int kRankThreads = 256;
constexpr int kRankWaves = kRankThreads / 64;

__device__ __forceinline__ int32_t rank_key(float p) {
    if (p != p) return 0x7fffffff;
    const double k = rint((double)p * 1e4);                   // (exact product; round-half-even)
    return (int32_t)fmin(fmax(k, -2.0e9), 2.0e9);             // (+-inf and everything beyond +-2e5 saturate)
}

// does candidate c with key k rank before the ground truth (index g, key kg)?
__device__ __forceinline__ int rank_before(int32_t k, int c, int32_t kg, int g) { return (k > kg || (k == kg && c < g)) ? 1 : 0; }

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one WAVE per query; the lanes stride over the query's contiguous candidates
__global__ void __launch_bounds__(kRankThreads) rank_row_queries_kernel(const float* S, int64_t ld, int n_q, int n_cand, const int32_t* gt,
                                                                      int32_t* rank, int32_t* keys, int64_t ldk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * kRankWaves + wave;
    if (q >= n_q) return;                                     // (the whole wave leaves: no barrier in this kernel)
    const float* row = S + q * ld;
    int32_t* krow = keys ? keys + q * ldk : nullptr;
    const int g = gt[q];
    const bool valid = g >= 0 && g < n_cand;                  // (outside the candidates: rank 0, nothing is read through g)
    const int32_t kg = valid ? rank_key(row[g]) : 0;
    if (!valid && !keys) {
        if (lane == 0) rank[q] = 0;
        return;
    }
    int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 2);      // floats before the first 16-byte boundary
    head = head < n_cand ? head : n_cand;
    const int n_vec = (n_cand - head) >> 2;
    const int tail0 = head + 4 * n_vec;
    int cnt = 0;
    if (lane < head) {
        const int32_t k = rank_key(row[lane]);
        if (krow) krow[lane] = k;
        cnt += rank_before(k, lane, kg, g);
    }
    for (int v = lane; v < n_vec; v += 64) {
        const int c0 = head + 4 * v;
        const f32x4 x = *reinterpret_cast<const f32x4*>(row + c0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int32_t k = rank_key(x[e]);
            if (krow) krow[c0 + e] = k;
            cnt += rank_before(k, c0 + e, kg, g);
        }
    }
    if (tail0 + lane < n_cand) {                              // (at most 3 floats)
        const int c = tail0 + lane;
        const int32_t k = rank_key(row[c]);
        if (krow) krow[c] = k;
        cnt += rank_before(k, c, kg, g);
    }
    cnt = wave_sum_i32(cnt);
    if (lane == 0) rank[q] = valid ? 1 + cnt : 0;
}

// one WORKGROUP per 64 adjacent queries (the columns); wave w walks rows w, w + kRankWaves, ...
__global__ void __launch_bounds__(kRankThreads) rank_col_queries_kernel(const float* S, int64_t ld, int n_q, int n_cand, const int32_t* gt,
                                                                      int32_t* rank, int32_t* keys, int64_t ldk) {
    __shared__ int s_cnt[kRankWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 64 + lane;
    const bool own = q < n_q;                                 // (idle lanes stay for the barrier and read nothing)
    const int g = own ? gt[q] : -1;
    const bool valid = g >= 0 && g < n_cand;
    const int32_t kg = valid ? rank_key(S[(int64_t)g * ld + q]) : 0;
    int cnt = 0;
    if (own && (valid || keys)) {
#pragma unroll 4
        for (int r = wave; r < n_cand; r += kRankWaves) {
            const int32_t k = rank_key(S[(int64_t)r * ld + q]);
            if (keys) keys[(int64_t)r * ldk + q] = k;
            cnt += rank_before(k, r, kg, g);
        }
    }
    s_cnt[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0 && own) rank[q] = valid ? 1 + ((s_cnt[0][lane] + s_cnt[1][lane]) + (s_cnt[2][lane] + s_cnt[3][lane])) : 0;
}

}  // namespace

extern "C" int cb_retrieval_rank(const float* S, int64_t ld, int32_t n_rows, int32_t n_cols, int32_t axis, const int32_t* gt, int32_t* rank,
                                 int32_t* keys, int64_t ldk, void* stream) {
    CB_REQUIRE(axis == CB_RANK_ROW_QUERIES || axis == CB_RANK_COL_QUERIES, "cb_retrieval_rank: unknown axis %d", axis);
    CB_REQUIRE(n_rows >= 0 && n_cols >= 0, "cb_retrieval_rank: negative size (n_rows %d, n_cols %d)", n_rows, n_cols);
    CB_REQUIRE(ld >= n_cols, "cb_retrieval_rank: ld %lld is smaller than n_cols = %d", (long long)ld, n_cols);
    CB_REQUIRE(!keys || ldk >= n_cols, "cb_retrieval_rank: the keys' ld %lld is smaller than n_cols = %d", (long long)ldk, n_cols);
    const int n_q = axis == CB_RANK_ROW_QUERIES ? n_rows : n_cols, n_cand = axis == CB_RANK_ROW_QUERIES ? n_cols : n_rows;
    if (n_q == 0) return 0;                                   // no queries: nothing to write
    CB_REQUIRE(gt && rank, "cb_retrieval_rank: null pointer (gt %p, rank %p)", (const void*)gt, (void*)rank);
    if (n_cand == 0) {                                        // no candidates: every ground truth is out of range
        const hipError_t e = hipMemsetAsync(rank, 0, sizeof(int32_t) * (size_t)n_q, cb_stream(stream));
        CB_REQUIRE(e == hipSuccess, "cb_retrieval_rank: hipMemsetAsync: %s", hipGetErrorString(e));
        return 0;
    }
    CB_REQUIRE(S, "cb_retrieval_rank: null pointer (scores)");
    if (axis == CB_RANK_ROW_QUERIES) {
        const dim3 grid((unsigned)(((int64_t)n_q + kRankWaves - 1) / kRankWaves));
        hipLaunchKernelGGL(rank_row_queries_kernel, grid, dim3(kRankThreads), 0, cb_stream(stream), S, ld, n_q, n_cand, gt, rank, keys, ldk);
    } else {
        const dim3 grid((unsigned)(((int64_t)n_q + 63) / 64));
        hipLaunchKernelGGL(rank_col_queries_kernel, grid, dim3(kRankThreads), 0, cb_stream(stream), S, ld, n_q, n_cand, gt, rank, keys, ldk);
    }
    return cb_launch_status("cb_retrieval_rank");
}
