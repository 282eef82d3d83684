// Masked-LM token masking (the pre-training collator's mask_batch_text_tokens, src/datasets/data_utils.py:23-70) drawn on the DEVICE: which
// tokens are labelled, and what stands in their place, from the same stateless hash and seed convention as the dropout masks -- one
// elementwise launch in front of cb_mlm_select, no host randomness, no scratch, so that a captured step masks afresh per replay (the graph
// advances the seed word).  ONE hash per token, cut into three fields:
//
//   s        = seed + *seed_ptr                                  (mod 2^64)
//   z        = cb_hash64(s, i)                                   i = r * Lt + t
//   labelled = eligible and (z >> 40) < (uint32)(p * 2^24)       bits 40..63
//   kind     = (((z >> 24) & 0xFFFF) * 10) >> 16                 bits 24..39: 0..7 [MASK], 8 a random word, 9 unchanged
//   word     = ((z & 0xFFFFFF) * V) >> 24                        bits  0..23
#include "common.h"

namespace {

constexpr int kMaskThreads = 256;
constexpr int kMaskMaxBlocks = 4096;        // more elements than that many workgroups hold: the grid strides
constexpr int kMaskMaxSpecial = 4;

struct MaskSpecial {                        // the special ids by value in the kernel arguments: no table in device memory
    int64_t id[kMaskMaxSpecial];
};

// One token per thread and trip, 8-byte accesses (the buffers are 8-byte aligned only); a thread reads its own element before it writes
// it, so ids_out may be ids.
__global__ void __launch_bounds__(kMaskThreads) mlm_mask_kernel(const int64_t* ids, int64_t n, MaskSpecial special, int n_special, int64_t pad_id,
                                                                int64_t mask_id, uint32_t V, uint32_t thr, uint64_t seed, const uint64_t* seed_ptr,
                                                                int64_t* ids_out, int64_t* labels, int64_t ignore_index) {
    const uint64_t s = seed + (seed_ptr ? *seed_ptr : 0ull);
    const int64_t stride = (int64_t)gridDim.x * kMaskThreads;
    for (int64_t i = (int64_t)blockIdx.x * kMaskThreads + threadIdx.x; i < n; i += stride) {
        const int64_t x = ids[i];
        bool eligible = pad_id < 0 || x != pad_id;
#pragma unroll
        for (int k = 0; k < kMaskMaxSpecial; ++k)
            if (k < n_special && x == special.id[k]) eligible = false;
        const uint64_t z = cb_hash64(s, (uint64_t)i);
        const bool labelled = eligible && (uint32_t)(z >> 40) < thr;
        const uint32_t kind = (uint32_t)((((z >> 24) & 0xFFFFull) * 10ull) >> 16);
        const int64_t word = (int64_t)(((z & 0xFFFFFFull) * (uint64_t)V) >> 24);
        ids_out[i] = labelled ? (kind <= 7u ? mask_id : kind == 8u ? word : x) : x;
        labels[i] = labelled ? x : ignore_index;
    }
}

}  // namespace

extern "C" int cb_mlm_mask(const int64_t* ids, int64_t rows, int32_t Lt, const int64_t* special, int32_t n_special, int64_t pad_id,
                           int64_t mask_id, int32_t V, float p, uint64_t seed, const uint64_t* seed_ptr, int64_t* ids_out, int64_t* labels,
                           int64_t ignore_index, void* stream) {
    CB_REQUIRE(ids && ids_out && labels, "cb_mlm_mask: null pointer");
    CB_REQUIRE(rows >= 1 && Lt >= 1, "cb_mlm_mask: need rows >= 1 and Lt >= 1 (rows %lld, Lt %d)", (long long)rows, Lt);
    CB_REQUIRE(n_special >= 0 && n_special <= kMaskMaxSpecial && (n_special == 0 || special),
               "cb_mlm_mask: need 0 <= n_special <= %d and the ids behind it (n_special %d)", kMaskMaxSpecial, n_special);
    CB_REQUIRE(V >= 1 && V <= (1 << 24), "cb_mlm_mask: need 1 <= V <= 2^24 (V %d)", V);
    CB_REQUIRE(p >= 0.0f && p <= 1.0f, "cb_mlm_mask: need 0 <= p <= 1 (p %g)", (double)p);      // (a NaN fails both comparisons)
    CB_REQUIRE(rows <= (((int64_t)1 << 62) / Lt), "cb_mlm_mask: rows * Lt overflows (rows %lld, Lt %d)", (long long)rows, Lt);
    MaskSpecial sp = {{0, 0, 0, 0}};
    for (int k = 0; k < n_special; ++k) sp.id[k] = special[k];
    const int64_t n = rows * Lt;
    const int64_t blocks = (n + kMaskThreads - 1) / kMaskThreads;
    const uint32_t thr = (uint32_t)(p * 16777216.0f);
    hipLaunchKernelGGL(mlm_mask_kernel, dim3((unsigned)(blocks < kMaskMaxBlocks ? blocks : kMaskMaxBlocks)), dim3(kMaskThreads), 0,
                       cb_stream(stream), ids, n, sp, n_special, pad_id, mask_id, (uint32_t)V, thr, seed, seed_ptr, ids_out, labels,
                       ignore_index);
    return cb_launch_status("cb_mlm_mask");
}
