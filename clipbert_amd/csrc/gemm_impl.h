// Templates of the cb_gemm kernels (included by gemm.hip and by the per-tile instantiation units gemm_inst_*.hip, so that
// the tile sizes compile in parallel).  See gemm.hip for the description of the kernel.
#pragma once
#include "common.h"
#include <stdlib.h>
#include <type_traits>

namespace cbgemm {


constexpr int NTHREADS = 256;

// EPS elements per 16-byte segment; BK = K step; SEGS segments per LDS row; ROWB bytes per LDS row;
// RB rows per transposing block
template <typename T> struct Tr;
template <> struct Tr<bf16> { static constexpr int EPS = 8, BK = 64, SEGS = 8, ROWB = 128, RB = 8; };
template <> struct Tr<float> { static constexpr int EPS = 4, BK = 32, SEGS = 8, ROWB = 144, RB = 4; };

template <typename T> __device__ __forceinline__ int lds_off(int row, int seg);
template <> __device__ __forceinline__ int lds_off<bf16>(int row, int seg) { return row * 128 + ((seg ^ (row & 7)) << 4); }
template <> __device__ __forceinline__ int lds_off<float>(int row, int seg) { return row * 144 + (seg << 4); }

struct GP {
    const void* A; const void* B; void* C; void* C2; const void* residual; const void* mask;
    const void* dact_pre; float* a_rowsum; int64_t ldd;
    int relu_bwd;
    int cls_rows;               // cb_gemm_desc.dgrad_s2: rows per parity class (M / 4), 0: an ordinary problem (see dgrad_s2_class)
    const float* post_scale; const float* post_scale2;   // ResNet-block ReLU x FrozenBN backward epilogue
    int batch;
    int fast_epi;               // index into FAST_EPI_COMBOS: the specialised epilogue of this call (fast_epilogue), 0: the generic epilogue_cols
    int64_t bs_a, bs_b, bs_c, bs_r;      // strided-batched problems on gridDim.z (strides in BYTES; bs_r in floats)
    const float* scale; const float* shift;
    const cb_pixel* a_tab; const cb_pixel* b_tab; const int32_t* c_rowmap;
    int64_t lda, ldb, ldc, ldc2, ldr, ldm, sH, sW;
    int M, N, K;
    int a_mode, b_mode;
    int R, S, Ct, H, W;
    int flip;                   // CB_KROW_TAPS: 0 tap t reads weight tap t, 1 the flipped one; >= TAP_S2: a parity class of dgrad_s2 (tap_weight)
    int c_f32, accumulate, split_k, act, relu_after;
    float alpha, dropout_p;
    uint64_t seed;
    const uint64_t* seed_ptr;
    short c_vec, c_vec8;        // (shorts: ten of these structs travel in the 4 KiB argument block of a grouped launch)
    short xcd_remap;            // 1: remap workgroup ids so that each XCD (own L2) owns a contiguous chunk of tiles
    short wt;                   // 1: the row-contiguous epilogue's bf16 C / C2 stores are write-through (sc1), see store8_wt
    int zfill;                  // zero_fill_pitch (see the header)
    uint32_t a_bytes, b_bytes;
    int ktiles;
    int slab_base, cnt_base;    // grouped launch with slab K split (gemm_tile): this problem's first slab unit / first tile counter
    const int32_t* res_rowmap;  // cb_gemm_desc.res_rowmap (4-wave kernels only)
    float* sq_slots;            // cb_gemm_desc.sq_slots (this problem's first slot): output tile t stores the sum of the squares of its C to sq_slots[t]
#ifdef CB_STAMPS
    unsigned long long* stamps;   // diagnostic build only (tools/stamps_*.py): this launch's record area, or null
#endif
};

// Specialised epilogues (round 6).  The generic epilogue (gemm_epilogue.h epilogue_cols) resolves every option of cb_gemm_desc by wave-uniform runtime branches around
// 64-bit address arithmetic and loads its M x N operands (residual / mask / stored derivative) one chunk after the other, each a
// dependent memory round trip.  The launches that make up the training step use a dozen option COMBINATIONS; each gets a straight-line
// body (fast_epilogue<FLAGS>, same header: `if constexpr` per option, packed fp32 math, 32-bit buffer offsets, write-through stores) whose
// operand loads leave BEFORE the staging barriers.  The host (gemm_prepare) maps a call's options to the index of its combination
// (GP::fast_epi, 0 = none: generic path); bf16 row-contiguous epilogues only, alpha 1, no row map / zero fill / accumulate / relu_bwd.
enum { EF_SCALE = 1, EF_SHIFT = 2, EF_RELU = 4, EF_GELU2 = 8, EF_DROP = 16, EF_RES = 32, EF_RELU_AFTER = 64, EF_MASK = 128, EF_MULAUX = 256,
       EF_RBWD = 512,      // cb_gemm_desc.relu_bwd: t = (acc [+ residual]) where mask > 0; C2 = t [* post_scale2]; C = t * post_scale
       EF_PS2 = 1024,
       EF_F32 = 2048,      // fp32 C STORED (accumulate 0 / 2), nothing else: the weight-gradient forms; + the tile's share of the squared norm
       EF_GELU1 = 4096,    // C = gelu(.), no second output (inference)
       EF_RMAP = 8192,     // the residual is read through GP::res_rowmap (-1: none for this row) -- 4-wave kernels only
       EF_CMAP = 16384 };  // C and the mask live at row GP::c_rowmap[m] (the classes of cb_gemm_desc.dgrad_s2) -- 4-wave kernels only
constexpr int FAST_EPI_COMBOS[] = {
    -1,                                                  // 0: generic
    0,                                                   // 1: C = acc                                  (data gradients without epilogue, grid conv)
    EF_SHIFT,                                            // 2: + bias                                   (fused QKV projection)
    EF_SHIFT | EF_GELU2,                                 // 3: C = gelu(.), C2 = gelu'(.)               (BertIntermediate forward, training)
    EF_SHIFT | EF_DROP | EF_RES,                         // 4: bias, dropout, + residual                (BertSelfOutput / BertOutput dense, training)
    EF_SHIFT | EF_RES,                                   // 5: the same in eval
    EF_MULAUX,                                           // 6: x stored gelu'                           (data gradient of BertOutput.dense)
    EF_RES,                                              // 7: + residual                               (data gradients that close a residual branch)
    EF_SCALE | EF_SHIFT | EF_RELU,                       // 8: FrozenBN + ReLU                          (bottleneck conv1 / conv2)
    EF_SCALE | EF_SHIFT,                                 // 9: FrozenBN                                 (projection shortcut)
    EF_SCALE | EF_SHIFT | EF_RES | EF_RELU_AFTER,        // 10: FrozenBN + shortcut + ReLU              (bottleneck conv3)
    EF_SCALE | EF_MASK,                                  // 11: x FrozenBN scale where the producer's ReLU was open (data gradients inside a block)
    EF_RBWD,                                             // 12-15: the ReLU x FrozenBN backward of the block that consumes the result, fused
    EF_RBWD | EF_RES,                                    //        (identity shortcut: + its gradient)
    EF_RBWD | EF_PS2,                                    //        (projection shortcut: second output x its FrozenBN scale)
    EF_RBWD | EF_PS2 | EF_RES,
    EF_F32,                                              // 16: dW stored by its first writer (+ sum of squares to GP::sq_slots) -- weight-gradient kernels only
    EF_SHIFT | EF_GELU1,                                 // 17: C = gelu(. + bias)                        (BertIntermediate forward, inference)
    EF_SCALE | EF_SHIFT | EF_RES | EF_RELU_AFTER | EF_RMAP,   // 18: 10 with the block input gathered at the even pixels (conv3 of a tail block)
    EF_RBWD | EF_RES | EF_RMAP,                          // 19: 13 with the compact shortcut gradient scattered to the even pixels (conv1 dgrad of a tail block)
    EF_SCALE | EF_MASK | EF_CMAP,                        // 20: 11 through the output row map (3x3 stride-2 data gradient by parity classes)
};
constexpr int FAST_EPI_F32 = 16;
constexpr int FAST_EPI_N = sizeof(FAST_EPI_COMBOS) / sizeof(int);

// ---------------------------------------------------------------------------------------------
// In-kernel time stamps (diagnostic build -DCB_STAMPS only, never the product library): thread 0 of a workgroup reads the
// chip-wide 100 MHz counter (s_memrealtime: the same clock on every XCD) at its phase boundaries and writes one record;
// the launch's header keeps min(start) / max(end) / #workgroups over ALL its workgroups.
//   area = [min start][max end][workgroups] + CB_STAMP_WGS x [t0 entry][t1 first K tile in LDS][t2 K loop done]
//          [t3 epilogue issued][t4 stores retired][hw id]
// ---------------------------------------------------------------------------------------------
#ifdef CB_STAMPS
constexpr int CB_STAMP_WGS = 512, CB_STAMP_REC = 6, CB_STAMP_HDR = 3;
constexpr int CB_STAMP_AREA = CB_STAMP_HDR + CB_STAMP_WGS * CB_STAMP_REC;       // u64 words per launch
struct Stamps {
    unsigned long long t[5];
    __device__ __forceinline__ void mark(int i) { t[i] = __builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ void flush(unsigned long long* area, unsigned lin, int tid) {
        if (!area || tid != 0) return;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long t4 = __builtin_amdgcn_s_memrealtime();
        atomicMin(area, t[0]);
        atomicMax(area + 1, t4);
        atomicAdd(area + 2, 1ull);
        if (lin < (unsigned)CB_STAMP_WGS) {
            unsigned long long* r = area + CB_STAMP_HDR + (size_t)lin * CB_STAMP_REC;
            r[0] = t[0]; r[1] = t[1]; r[2] = t[2]; r[3] = t[3]; r[4] = t4;
            unsigned hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            r[5] = ((unsigned long long)xcc << 32) | hw;
        }
    }
};
#define CB_STAMP_DECL() Stamps stamps_
#define CB_STAMP(i) stamps_.mark(i)
#define CB_STAMP_FLUSH(p, lin, tid) stamps_.flush((p).stamps, (lin), (tid))
#else
#define CB_STAMP_DECL() do {} while (0)
#define CB_STAMP(i) do {} while (0)
#define CB_STAMP_FLUSH(p, lin, tid) do {} while (0)
#endif

template <typename T> __device__ __forceinline__ u32x4 load_guarded(const T* src, int nvalid) {
    constexpr int EPS = Tr<T>::EPS;
    union { u32x4 v; T e[EPS]; } u;
#pragma unroll
    for (int i = 0; i < EPS; ++i) u.e[i] = (i < nvalid) ? src[i] : (T)0.f;
    return u.v;
}

// Buffer-descriptor loads: the hardware range check returns zeros for any byte offset >= num_records, so
// predication (rows past M, taps in the padding, K tails) is ONE select of the offset to OOB -- no branches,
// no 64-bit address arithmetic in the K loop.  Operands must be < 2 GiB (else the generic loaders run).
constexpr uint32_t OOB = 0x80000000u;
typedef decltype(__builtin_amdgcn_make_buffer_rsrc((void*)nullptr, (short)0, 0, 0)) rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ u32x4 bload16(rsrc_t r, uint32_t off) { return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0); }

// CB_KROW_TAPS: the weight tap that reduction tap `tap` reads.  GP::flip >= TAP_S2 (set per workgroup by dgrad_s2_class): the taps of one
// parity class of the 3x3 stride-2 data gradient -- window position (jr, js) of the R x S (1 or 2 each) window of g meets weight tap
// (r0 - 2 jr, s0 - 2 js), and flip - TAP_S2 = 3 r0 + s0.
constexpr int TAP_S2 = 16;
__device__ __forceinline__ int tap_weight(const GP& p, int tap) {
    if (p.flip >= TAP_S2) {
        const int jr = p.S == 2 ? tap >> 1 : tap, js = p.S == 2 ? tap & 1 : 0;
        return p.flip - TAP_S2 - 6 * jr - 2 * js;
    }
    return p.flip ? (p.R * p.S - 1 - tap) : tap;
}

// one operand of the GEMM as the loaders see it
struct Opnd {
    const void* base; const cb_pixel* tab; int64_t ld; int mode; uint32_t bytes;
};

// ---------------------------------------------------------------------------------------------
// ROWK loaders: tile rows are GEMM rows, 16-byte segments run along k.  Per-row state is fixed for the
// whole K loop; `Stage` holds one K-tile of loaded registers; load() must be called for consecutive
// K-tiles (it advances the thread's k -> (tap, channel) position incrementally: no divisions).
// ---------------------------------------------------------------------------------------------
template <typename T, int ROWS, bool FAST> struct RowkLoader {
    using X = Tr<T>;
    static constexpr bool TR = false;
    static constexpr bool KROW = false;        // operand stored [k][row] (dgrad's B, wgrad's A and B)
    static constexpr int NS = ROWS * X::SEGS / NTHREADS;
    static constexpr int ESZ = (int)sizeof(T);
    static_assert(ROWS * X::SEGS % NTHREADS == 0, "tile/threads mismatch");
    struct Stage { u32x4 r[NS]; };
    int64_t off[NS];            // element offset of (row, k=0)        (generic path)
    uint32_t boff[NS];          // byte offset of (row, k=0), or OOB   (fast path)
    int ih[NS], iw[NS];
    bool ok[NS];
    int c, rr, ss;              // this thread's segment: channel within the tap, tap = (rr, ss)
    bool gather;
    rsrc_t rs;
    const T* base;

    __device__ __forceinline__ void init(const GP& p, const Opnd& o, int row0, int bound, int kt0, int tid) {
        gather = o.mode == CB_ROWK_GATHER;
        base = reinterpret_cast<const T*>(o.base);
        if constexpr (FAST) rs = make_rsrc(o.base, o.bytes);
        int k = kt0 * X::BK + (tid % X::SEGS) * X::EPS;
        c = k; rr = 0; ss = 0;
        if (gather) {
            int tap = k / p.Ct;
            c = k - tap * p.Ct;
            rr = tap / p.S; ss = tap - rr * p.S;
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            int idx = tid + i * NTHREADS;
            int row = row0 + idx / X::SEGS;
            ok[i] = row < bound;
            ih[i] = 0; iw[i] = 0;
            int64_t e = (int64_t)row * o.ld;
            if (gather) {
                cb_pixel px = {0, 0, 0};
                if (ok[i]) px = o.tab[row];
                e = px.off; ih[i] = px.ih0; iw[i] = px.iw0;
            }
            off[i] = e;
            boff[i] = ok[i] ? (uint32_t)e * (uint32_t)ESZ : OOB;
        }
    }
    template <bool CHECK> __device__ __forceinline__ void load(Stage& st, const GP& p) {
        const bool kv = gather ? (rr < p.R) : (c < p.K);
        const int klim = gather ? p.Ct : p.K;
        const int64_t tapoff = gather ? (rr * p.sH + ss * p.sW) : 0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            bool v = kv && ok[i];
            if (gather) v = v && (unsigned)(ih[i] + rr) < (unsigned)p.H && (unsigned)(iw[i] + ss) < (unsigned)p.W;
            if constexpr (FAST) {
                uint32_t o32 = boff[i] + (uint32_t)(tapoff + c) * (uint32_t)ESZ;
                st.r[i] = bload16(rs, v ? o32 : OOB);
            } else {
                u32x4 z = {0u, 0u, 0u, 0u};
                st.r[i] = v ? load_guarded<T>(base + off[i] + tapoff + c, klim - c) : z;
            }
        }
        c += X::BK;
        if (gather) {
            while (c >= p.Ct) { c -= p.Ct; if (++ss == p.S) { ss = 0; ++rr; } }
        }
    }
    __device__ __forceinline__ void store(const Stage& st, unsigned char* tile, int tid) const {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            int idx = tid + i * NTHREADS;
            *reinterpret_cast<u32x4*>(tile + lds_off<T>(idx / X::SEGS, idx % X::SEGS)) = st.r[i];
        }
    }
};

// ---------------------------------------------------------------------------------------------
// KROW loaders: memory has the reduction index outermost; each thread moves a (4 k) x (RB rows) block
// and transposes it in registers on its way into the [row][k] LDS tile.
// ---------------------------------------------------------------------------------------------
template <typename T, int ROWS, bool FAST> struct KrowLoader {
    using X = Tr<T>;
    static constexpr bool TR = false;
    static constexpr bool KROW = true;        // operand stored [k][row] (dgrad's B, wgrad's A and B)
    static constexpr int RBLK = ROWS / X::RB;              // row blocks per tile
    static constexpr int CNT = RBLK * (X::BK / 4);         // thread-blocks per tile
    static constexpr int NI = (CNT + NTHREADS - 1) / NTHREADS;
    static constexpr int ESZ = (int)sizeof(T);
    struct Stage { u32x4 r[NI][4]; };
    int mode, bound;
    int64_t ld;
    const cb_pixel* tab;
    const T* base;
    rsrc_t rs;
    int kb0[NI];        // k of the block's first row (advances by BK per tile)
    int co[NI], tap[NI];// CB_KROW_TAPS: k -> (tap, co)
    int row[NI];        // global row of the block's first element
    int rr[NI], ss[NI]; // CB_KROW_GATHER: tap of this row block
    int64_t rowoff[NI]; // element offset contributed by the row (and its tap for GATHER)
    bool act[NI];

    __device__ __forceinline__ void init(const GP& p, const Opnd& o, int row0, int bnd, int kt0, int tid) {
        mode = o.mode; bound = bnd; ld = o.ld; tab = o.tab;
        base = reinterpret_cast<const T*>(o.base);
        if constexpr (FAST) rs = make_rsrc(o.base, o.bytes);
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            int b = tid + it * NTHREADS;
            act[it] = b < CNT;
            int rb = b % RBLK, kb = b / RBLK;
            row[it] = row0 + rb * X::RB;
            kb0[it] = kt0 * X::BK + kb * 4;        // the 4 k of a block never straddle a tap (Ct % 4 == 0)
            rowoff[it] = row[it];
            co[it] = kb0[it]; tap[it] = 0; rr[it] = 0; ss[it] = 0;
            if (mode == CB_KROW_TAPS) {            // weights [Ct][taps][bound] read for a transposed conv
                tap[it] = kb0[it] / p.Ct;
                co[it] = kb0[it] - tap[it] * p.Ct;
            } else if (mode == CB_KROW_GATHER) {   // row = (tap, channel) of the gathered image
                int tp = row[it] / p.Ct;
                int ch = row[it] - tp * p.Ct;
                rr[it] = tp / p.S; ss[it] = tp - rr[it] * p.S;
                rowoff[it] = rr[it] * p.sH + ss[it] * p.sW + ch;
            }
        }
    }
    template <bool CHECK> __device__ __forceinline__ void load(Stage& st, const GP& p) {
        u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            if (!act[it]) { st.r[it][0] = z; st.r[it][1] = z; st.r[it][2] = z; st.r[it][3] = z; continue; }
            const int nvalid = bound - row[it];
            int64_t ro = rowoff[it];
            if (mode == CB_KROW_TAPS) {
                int tapw = tap_weight(p, tap[it]);
                ro = (int64_t)tapw * bound + row[it];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = kb0[it] + j;
                bool v = k < p.K && nvalid > 0;
                int64_t e;
                if (mode == CB_KROW_GATHER) {
                    cb_pixel px = {0, 0, 0};
                    if (v) px = tab[k];
                    v = v && (unsigned)(px.ih0 + rr[it]) < (unsigned)p.H && (unsigned)(px.iw0 + ss[it]) < (unsigned)p.W;
                    e = px.off + ro;
                } else if (mode == CB_KROW_TAPS) {
                    e = (int64_t)(co[it] + j) * ld + ro;
                } else {
                    e = (int64_t)k * ld + ro;
                }
                if constexpr (FAST) {
                    // rows past `bound` inside a block read neighbouring (in-buffer) data: those tile rows only feed
                    // outputs the epilogue discards; past the buffer end the descriptor returns zeros
                    st.r[it][j] = bload16(rs, v ? (uint32_t)e * (uint32_t)ESZ : OOB);
                } else {
                    st.r[it][j] = v ? load_guarded<T>(base + e, nvalid) : z;
                }
            }
            kb0[it] += X::BK;
            if (mode == CB_KROW_TAPS) {
                co[it] += X::BK;
                while (co[it] >= p.Ct) { co[it] -= p.Ct; ++tap[it]; }
            }
        }
    }
    __device__ __forceinline__ void store(const Stage& st, unsigned char* tile, int tid) const {
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            int b = tid + it * NTHREADS;
            if (b >= CNT) continue;
            int rb = b % RBLK, kb = b / RBLK;
            int r0 = rb * X::RB;
            if constexpr (sizeof(T) == 2) {
                // st.r[it][j][d] holds rows (2d, 2d+1) at k = kb*4 + j
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    uint32_t a0 = st.r[it][0][d], a1 = st.r[it][1][d], a2 = st.r[it][2][d], a3 = st.r[it][3][d];
                    u32x2 even = {(a0 & 0xffffu) | (a1 << 16), (a2 & 0xffffu) | (a3 << 16)};
                    u32x2 odd = {(a0 >> 16) | (a1 & 0xffff0000u), (a2 >> 16) | (a3 & 0xffff0000u)};
                    *reinterpret_cast<u32x2*>(tile + lds_off<T>(r0 + 2 * d, kb >> 1) + (kb & 1) * 8) = even;
                    *reinterpret_cast<u32x2*>(tile + lds_off<T>(r0 + 2 * d + 1, kb >> 1) + (kb & 1) * 8) = odd;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    u32x4 o = {st.r[it][0][e], st.r[it][1][e], st.r[it][2][e], st.r[it][3][e]};
                    *reinterpret_cast<u32x4*>(tile + lds_off<T>(r0 + e, kb)) = o;
                }
            }
        }
    }
};

// =============================================================================================
// FAST loaders (compile-time addressing mode, range-checked buffer loads): the steady-state K loop costs
// one v_add + one buffer_load per 16 bytes (plus two compares per load for convolution gathers).
// =============================================================================================
enum { KM_PLAIN = 0, KM_TAPS = 1, KM_GATHER = 2 };

template <typename T, int ROWS, bool GATHER> struct RowkFast {
    using X = Tr<T>;
    static constexpr bool TR = false;
    static constexpr bool KROW = false;        // operand stored [k][row] (dgrad's B, wgrad's A and B)
    static constexpr int NS = ROWS * X::SEGS / NTHREADS;
    static constexpr uint32_t ESZ = (uint32_t)sizeof(T);
    struct Stage { u32x4 r[NS]; };
    rsrc_t rs;
    uint32_t voff[NS];          // byte offset of this thread's segment (k position included unless GATHER), or OOB
    int ih[NS], iw[NS];         // GATHER: top-left input pixel of the row's receptive field
    int c, rr, ss;              // GATHER: channel within the tap, tap = (rr, ss)
    int krem;                   // !GATHER: K - (k of this thread's segment)

    __device__ __forceinline__ void init(const GP& p, const Opnd& o, int row0, int bound, int kt0, int tid) {
        rs = make_rsrc(o.base, o.bytes);
        const int k = kt0 * X::BK + (tid % X::SEGS) * X::EPS;
        c = k; rr = 0; ss = 0; krem = p.K - k;
        if constexpr (GATHER) {
            int tap = k / p.Ct;
            c = k - tap * p.Ct;
            rr = tap / p.S; ss = tap - rr * p.S;
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int row = row0 + (tid + i * NTHREADS) / X::SEGS;
            const bool ok = row < bound;
            ih[i] = 0; iw[i] = 0;
            if constexpr (GATHER) {
                cb_pixel px = {0, 0, 0};
                if (ok) px = o.tab[row];
                ih[i] = px.ih0; iw[i] = px.iw0;
                voff[i] = ok ? (uint32_t)px.off * ESZ : OOB;
            } else {
                voff[i] = ok ? ((uint32_t)row * (uint32_t)o.ld + (uint32_t)k) * ESZ : OOB;
            }
        }
    }
    template <bool CHECK> __device__ __forceinline__ void load(Stage& st, const GP& p) {
        if constexpr (GATHER) {
            const bool kv = rr < p.R;
            const uint32_t koff = (uint32_t)(rr * (int)p.sH + ss * (int)p.sW + c) * ESZ;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const bool v = kv && (unsigned)(ih[i] + rr) < (unsigned)p.H && (unsigned)(iw[i] + ss) < (unsigned)p.W;
                st.r[i] = bload16(rs, v ? voff[i] + koff : OOB);
            }
            if (p.Ct >= X::BK) {
                c += X::BK;
                if (c >= p.Ct) { c -= p.Ct; if (++ss == p.S) { ss = 0; ++rr; } }
            } else {                                   // several taps per K step (stem: 32 channels per tap)
                ss += X::BK / p.Ct;
                while (ss >= p.S) { ss -= p.S; ++rr; }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                uint32_t o32 = voff[i];
                if (CHECK && krem <= 0) o32 = OOB;
                st.r[i] = bload16(rs, o32);
                voff[i] += X::BK * ESZ;
            }
            krem -= X::BK;
        }
    }
    __device__ __forceinline__ void store(const Stage& st, unsigned char* tile, int tid) const {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            int idx = tid + i * NTHREADS;
            *reinterpret_cast<u32x4*>(tile + lds_off<T>(idx / X::SEGS, idx % X::SEGS)) = st.r[i];
        }
    }
};

// KB = k-lines per thread block (8: 8x8 transpose -> ds_write_b128; 4: ds_write_b64; 2: ds_write_b32), chosen so
// that the tile's blocks cover all 256 threads; SHIFT rotates the thread -> block map so that two half-occupancy
// operands (A and B both KROW) land on different waves.
// Lane mapping: the k-block index varies fastest, so the lanes of one LDS write group fill ONE tile row
// (all 32 banks, conflict-free) while lanes NKB apart read adjacent 16-byte chunks of the same k-line.
template <typename T, int ROWS, int KMODE, int KB_ = 4, int SHIFT = 0> struct KrowFast {
    using X = Tr<T>;
    static constexpr bool TR = false;
    static constexpr bool KROW = true;        // operand stored [k][row] (dgrad's B, wgrad's A and B)
    static constexpr int KB = sizeof(T) == 2 ? KB_ : 4;
    static constexpr int NKB = X::BK / KB;
    static constexpr int RBLK = ROWS / X::RB;
    static constexpr int CNT = RBLK * NKB;
    static constexpr int NI = (CNT + NTHREADS - 1) / NTHREADS;
    static constexpr uint32_t ESZ = (uint32_t)sizeof(T);
    struct Stage { u32x4 r[NI][KB]; };
    rsrc_t rs;
    const cb_pixel* tab;
    uint32_t ldb;               // bytes between consecutive reduction indices
    uint32_t voff[NI];          // PLAIN: byte offset of (k = kb0, row) | TAPS/GATHER: byte offset contributed by the row
    int kb0[NI];                // k of the block's first line
    int co[NI], tap[NI];        // TAPS
    int rr[NI], ss[NI];         // GATHER
    cb_pixel px[NI][KB];        // GATHER: table entries of the NEXT tile (prefetched one call ahead)
    bool act[NI];
    uint32_t bound;

    __device__ __forceinline__ void init(const GP& p, const Opnd& o, int row0, int bnd, int kt0, int tid) {
        rs = make_rsrc(o.base, o.bytes);
        tab = o.tab; ldb = (uint32_t)o.ld * ESZ; bound = (uint32_t)bnd;
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            const int b = ((tid + SHIFT) % NTHREADS) + it * NTHREADS;
            const int kb = b % NKB, rb = b / NKB;
            const int row = row0 + rb * X::RB;
            act[it] = (b < CNT) && (row < bnd);
            kb0[it] = kt0 * X::BK + kb * KB;
            co[it] = kb0[it]; tap[it] = 0; rr[it] = 0; ss[it] = 0;
            if constexpr (KMODE == KM_PLAIN) {
                voff[it] = ((uint32_t)kb0[it] * (uint32_t)o.ld + (uint32_t)row) * ESZ;
            } else if constexpr (KMODE == KM_TAPS) {        // weights [Ct][taps][bound] of a transposed conv
                tap[it] = kb0[it] / p.Ct;
                co[it] = kb0[it] - tap[it] * p.Ct;
                voff[it] = (uint32_t)row * ESZ;
            } else {                                        // row = (tap, channel) of the gathered image
                const int tp = row / p.Ct, ch = row - tp * p.Ct;
                rr[it] = tp / p.S; ss[it] = tp - rr[it] * p.S;
                voff[it] = (uint32_t)(rr[it] * (int)p.sH + ss[it] * (int)p.sW + ch) * ESZ;
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    cb_pixel e = {0, (int16_t)-30000, (int16_t)-30000};
                    if (act[it] && kb0[it] + j < p.K) e = tab[kb0[it] + j];
                    px[it][j] = e;
                }
            }
        }
    }
    template <bool CHECK> __device__ __forceinline__ void load(Stage& st, const GP& p) {
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            if constexpr (KMODE == KM_PLAIN) {
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    bool v = act[it];
                    if (CHECK) v = v && (kb0[it] + j < p.K);
                    st.r[it][j] = bload16(rs, v ? voff[it] + (uint32_t)j * ldb : OOB);
                }
                voff[it] += X::BK * ldb;
                kb0[it] += X::BK;
            } else if constexpr (KMODE == KM_TAPS) {        // (Ct % 8 == 0: a block never straddles a tap)
                const int tapw = tap_weight(p, tap[it]);
                const bool v = act[it] && tap[it] < p.R * p.S;
                const uint32_t base = (uint32_t)co[it] * ldb + (uint32_t)tapw * bound * ESZ + voff[it];
#pragma unroll
                for (int j = 0; j < KB; ++j) st.r[it][j] = bload16(rs, v ? base + (uint32_t)j * ldb : OOB);
                co[it] += X::BK;
                while (co[it] >= p.Ct) { co[it] -= p.Ct; ++tap[it]; }
            } else {
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const cb_pixel e = px[it][j];
                    const bool v = (unsigned)(e.ih0 + rr[it]) < (unsigned)p.H && (unsigned)(e.iw0 + ss[it]) < (unsigned)p.W;
                    st.r[it][j] = bload16(rs, v ? (uint32_t)e.off * ESZ + voff[it] : OOB);
                }
                kb0[it] += X::BK;
#pragma unroll
                for (int j = 0; j < KB; ++j) {              // table entries of the next K tile
                    cb_pixel e = {0, (int16_t)-30000, (int16_t)-30000};
                    if (act[it] && kb0[it] + j < p.K) e = tab[kb0[it] + j];
                    px[it][j] = e;
                }
            }
        }
    }
    __device__ __forceinline__ void store(const Stage& st, unsigned char* tile, int tid) const {
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            const int b = ((tid + SHIFT) % NTHREADS) + it * NTHREADS;
            if (b >= CNT) continue;
            const int kb = b % NKB, rb = b / NKB;
            const int r0 = rb * X::RB;
            if constexpr (sizeof(T) == 2 && KB == 8) {
                // 8x8 16-bit transpose: st.r[it][j][d] holds rows (2d, 2d+1) at k = kb*8 + j; one 16-byte store per row
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    u32x4 even, odd;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        even[q] = __builtin_amdgcn_perm(st.r[it][2 * q + 1][d], st.r[it][2 * q][d], 0x05040100u);
                        odd[q] = __builtin_amdgcn_perm(st.r[it][2 * q + 1][d], st.r[it][2 * q][d], 0x07060302u);
                    }
                    *reinterpret_cast<u32x4*>(tile + lds_off<T>(r0 + 2 * d, kb)) = even;
                    *reinterpret_cast<u32x4*>(tile + lds_off<T>(r0 + 2 * d + 1, kb)) = odd;
                }
            } else if constexpr (sizeof(T) == 2 && KB == 2) {
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const uint32_t even = __builtin_amdgcn_perm(st.r[it][1][d], st.r[it][0][d], 0x05040100u);
                    const uint32_t odd = __builtin_amdgcn_perm(st.r[it][1][d], st.r[it][0][d], 0x07060302u);
                    *reinterpret_cast<uint32_t*>(tile + lds_off<T>(r0 + 2 * d, kb >> 2) + (kb & 3) * 4) = even;
                    *reinterpret_cast<uint32_t*>(tile + lds_off<T>(r0 + 2 * d + 1, kb >> 2) + (kb & 3) * 4) = odd;
                }
            } else if constexpr (sizeof(T) == 2) {
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    u32x2 even = {__builtin_amdgcn_perm(st.r[it][1][d], st.r[it][0][d], 0x05040100u),
                                  __builtin_amdgcn_perm(st.r[it][3][d], st.r[it][2][d], 0x05040100u)};
                    u32x2 odd = {__builtin_amdgcn_perm(st.r[it][1][d], st.r[it][0][d], 0x07060302u),
                                 __builtin_amdgcn_perm(st.r[it][3][d], st.r[it][2][d], 0x07060302u)};
                    *reinterpret_cast<u32x2*>(tile + lds_off<T>(r0 + 2 * d, kb >> 1) + (kb & 1) * 8) = even;
                    *reinterpret_cast<u32x2*>(tile + lds_off<T>(r0 + 2 * d + 1, kb >> 1) + (kb & 1) * 8) = odd;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    u32x4 o = {st.r[it][0][e], st.r[it][1][e], st.r[it][2][e], st.r[it][3][e]};
                    *reinterpret_cast<u32x4*>(tile + lds_off<T>(r0 + e, kb)) = o;
                }
            }
        }
    }
};

// =============================================================================================
// KROW operands, bf16: no register transpose at all.  The tile is stored in LDS in its NATURAL image
// [k][rows] (each k-line = ROWS contiguous elements = what a fully coalesced global read delivers) and the MFMA
// fragments are produced by the LDS transpose-read ds_read_b64_tr_b16: per 16-lane group, lane p supplies the
// address of 4 consecutive rows of line (kbase + p/4) and lane i receives column i of that 4 x 16 block
// (semantics verified on gfx950 by tools/tr_probe.hip).  16-byte chunks of a line are XOR-swizzled with the
// line index so that the 8 lines read by one 32-lane bank group fall into 8 distinct 32-byte windows.
// =============================================================================================
typedef __attribute__((ext_vector_type(4))) short s16x4;
__device__ __forceinline__ s16x4 lds_read_tr(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

template <int ROWS> __device__ __forceinline__ int tr_chunk_swz(int kline) {
    if constexpr (ROWS >= 128) return (((kline & 3) | (((kline >> 3) & 1) << 2)) << 1);          // 8 windows per line
    else return ((((kline >> 1) & 1) | (((kline >> 3) & 1) << 1)) << 1);                        // 4 windows, 2 lines per bank row
}
// byte offset of rows [r, r+4) of line k in a KROW tile
template <int ROWS> __device__ __forceinline__ int tr_off(int kline, int r) {
    const int chunk = (r >> 3) ^ tr_chunk_swz<ROWS>(kline);
    return kline * (ROWS * 2) + (chunk << 4) + ((r & 7) << 1);
}

// MFMA fragment (rows r0..r0+15, k = kk*32 + 8*(lane>>4) .. +7) of a natural-image KROW tile
template <int ROWS> __device__ __forceinline__ bf16x8 tr_frag(const unsigned char* tile, int r0, int kk, int lane) {
    const int p = lane & 15, kbase = kk * 32 + 8 * (lane >> 4) + (p >> 2);
    const int r = r0 + 4 * (p & 3);
    union { struct { s16x4 lo, hi; } h; bf16x8 v; } u;
    u.h.lo = lds_read_tr(tile + tr_off<ROWS>(kbase, r));
    u.h.hi = lds_read_tr(tile + tr_off<ROWS>(kbase + 4, r));
    return u.v;
}

template <int ROWS, int KMODE> struct KrowTr {
    using X = Tr<bf16>;
    static constexpr bool TR = true;
    static constexpr bool KROW = true;
    static constexpr int CH = ROWS / 8;                           // 16-byte chunks per k-line
    static constexpr int NS = CH * X::BK / NTHREADS;
    static_assert(CH * X::BK % NTHREADS == 0, "tile/threads mismatch");
    static constexpr uint32_t ESZ = 2;
    struct Stage { u32x4 r[NS]; };
    rsrc_t rs;
    const cb_pixel* tab;
    uint32_t ldb, bound;
    uint32_t voff[NS];          // PLAIN: byte offset of (k-line, chunk) | TAPS / GATHER: the part contributed by the rows
    int kl[NS];                 // global k of the slot's line
    int co[NS], tap[NS];        // TAPS
    int rr, ss;                 // GATHER (the 8 rows of a chunk share a tap)
    cb_pixel px[NS];            // GATHER: table entries of the NEXT tile
    bool act[NS];

    __device__ __forceinline__ void init(const GP& p, const Opnd& o, int row0, int bnd, int kt0, int tid) {
        rs = make_rsrc(o.base, o.bytes);
        tab = o.tab; ldb = (uint32_t)o.ld * ESZ; bound = (uint32_t)bnd;
        rr = 0; ss = 0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int idx = tid + i * NTHREADS;
            const int chunk = idx % CH, kline = idx / CH;
            const int row = row0 + chunk * 8;
            act[i] = row < bnd;
            kl[i] = kt0 * X::BK + kline;
            co[i] = kl[i]; tap[i] = 0;
            if constexpr (KMODE == KM_PLAIN) {
                voff[i] = ((uint32_t)kl[i] * (uint32_t)o.ld + (uint32_t)row) * ESZ;
            } else if constexpr (KMODE == KM_TAPS) {
                tap[i] = kl[i] / p.Ct;
                co[i] = kl[i] - tap[i] * p.Ct;
                voff[i] = (uint32_t)row * ESZ;
            } else {
                const int tp = row / p.Ct, ch = row - tp * p.Ct;        // chunk is the same for all slots of a thread
                rr = tp / p.S; ss = tp - rr * p.S;
                voff[i] = (uint32_t)(rr * (int)p.sH + ss * (int)p.sW + ch) * ESZ;
                cb_pixel e = {0, (int16_t)-30000, (int16_t)-30000};
                if (act[i] && kl[i] < p.K) e = tab[kl[i]];
                px[i] = e;
            }
        }
    }
    template <bool CHECK> __device__ __forceinline__ void load(Stage& st, const GP& p) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            if constexpr (KMODE == KM_PLAIN) {
                bool v = act[i];
                if (CHECK) v = v && (kl[i] < p.K);
                st.r[i] = bload16(rs, v ? voff[i] : OOB);
                voff[i] += X::BK * ldb;
                kl[i] += X::BK;
            } else if constexpr (KMODE == KM_TAPS) {
                const int tapw = tap_weight(p, tap[i]);
                const bool v = act[i] && tap[i] < p.R * p.S;
                st.r[i] = bload16(rs, v ? (uint32_t)co[i] * ldb + (uint32_t)tapw * bound * ESZ + voff[i] : OOB);
                co[i] += X::BK;
                while (co[i] >= p.Ct) { co[i] -= p.Ct; ++tap[i]; }
            } else {
                const cb_pixel e = px[i];
                const bool v = (unsigned)(e.ih0 + rr) < (unsigned)p.H && (unsigned)(e.iw0 + ss) < (unsigned)p.W;
                st.r[i] = bload16(rs, v ? (uint32_t)e.off * ESZ + voff[i] : OOB);
                kl[i] += X::BK;
                cb_pixel nx = {0, (int16_t)-30000, (int16_t)-30000};
                if (act[i] && kl[i] < p.K) nx = tab[kl[i]];
                px[i] = nx;
            }
        }
    }
    __device__ __forceinline__ void store(const Stage& st, unsigned char* tile, int tid) const {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int idx = tid + i * NTHREADS;
            const int chunk = idx % CH, kline = idx / CH;
            *reinterpret_cast<u32x4*>(tile + kline * (ROWS * 2) + ((chunk ^ tr_chunk_swz<ROWS>(kline)) << 4)) = st.r[i];
        }
    }
};

// Workgroup -> (n tile, m tile, k split).  The dispatcher deals consecutive workgroup ids round-robin over the 8 XCDs,
// each with its own L2.  Remapped, XCD x owns the x-th contiguous eighth of the (split, m tile, n tile) order, so the
// A rows / K slices its blocks share are fetched into ONE L2 instead of all eight.
struct TileId { int bx, by, bz; };
__device__ __forceinline__ TileId tile_id(const GP& p) {
    TileId t;
    if (!p.xcd_remap) { t.bx = blockIdx.x; t.by = blockIdx.y; t.bz = blockIdx.z; return t; }
    const unsigned gx = gridDim.x, gy = gridDim.y;
    const unsigned total = gx * gy * gridDim.z;
    const unsigned lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const unsigned xcd = lin & 7u, i = lin >> 3;
    const unsigned q = total >> 3, r = total & 7u;
    const unsigned l2 = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
    t.bx = (int)(l2 % gx);
    const unsigned rest = l2 / gx;
    t.by = (int)(rest % gy);
    t.bz = (int)(rest / gy);
    return t;
}

// strided-batched problems: grid z = batch * split_k + k split.  Rebases the operands of this block's problem.
__device__ __forceinline__ void apply_batch(GP& p, TileId& t) {
    if (p.batch <= 1) return;
    // (the quotient is computed on the VALU; pinned to an SGPR, the rebased operands -- and the loaders' buffer descriptors made from them --
    // stay scalar whatever the rest of the kernel does with C: left to the compiler, the descriptors of the 128x128 kernels moved to VGPRs
    // and every buffer load of the K loop into a waterfall loop once the generic epilogue became one function, +9 % on those launches)
    const int b = __builtin_amdgcn_readfirstlane(t.bz / p.split_k);
    t.bz -= b * p.split_k;
    const int64_t oa = b * p.bs_a, ob = b * p.bs_b;
    p.A = reinterpret_cast<const unsigned char*>(p.A) + oa;
    p.B = reinterpret_cast<const unsigned char*>(p.B) + ob;
    p.C = reinterpret_cast<unsigned char*>(p.C) + b * p.bs_c;
    if (p.a_bytes) p.a_bytes -= (uint32_t)oa;              // the range check of the buffer descriptors keeps covering the
    if (p.b_bytes) p.b_bytes -= (uint32_t)ob;              // rest of the stacked buffer
    if (p.a_rowsum) p.a_rowsum += b * p.bs_r;
}

// cb_gemm_desc.dgrad_s2: the four parity classes of a 3x3 stride-2 data gradient share one grid, each class tiled on its own (grid y =
// 4 * ceil(cls_rows / BM), dgrad_s2_grid_y).  Along y the CLASS varies fastest, the four-tap class first: four consecutive workgroups
// work on the same block of pixels -- the same rows of g, neighbouring output rows -- and every run of the grid holds the same mix of
// 4-, 2-, 2- and 1-tap tiles.  (Class-major tiles, as the rows are laid out, put all four-tap tiles -- 4/9 of the work -- on the last two
// of the eight XCDs under the XCD-compact order and at the end of the grid under the dispatch order: measured 45 / 35 us at
// 50176 x 128 x 1152 against the figure in DESIGN.md for this order.)  A workgroup turns its copy of the parameter block into the ordinary
// gather x CB_KROW_TAPS problem of ITS class (py, px): M = cls_rows rows, an R x S = (1 + py) x (1 + px) window of g at the table's pixel,
// K = R * S * Ct, weight taps (1 + py - 2 jr, 1 + px - 2 js) (tap_weight), and the class's part of the output row map.  Everything after
// this point -- loaders, K loop, epilogue -- is the code every data gradient runs.
template <int BM, int BK>
__device__ __forceinline__ void dgrad_s2_class(GP& p, TileId& bid) {
    if (p.cls_rows <= 0) return;                                 // (block-uniform)
    const int cls = 3 - (bid.by & 3);
    bid.by >>= 2;
    const int py = cls >> 1, px = cls & 1;
    p.M = p.cls_rows;
    p.R = 1 + py; p.S = 1 + px;
    p.K = p.R * p.S * p.Ct;
    p.ktiles = (p.K + BK - 1) / BK;
    p.flip = TAP_S2 + 3 * (1 + py) + (1 + px);
    p.c_rowmap += (int64_t)cls * p.cls_rows;
}
inline int dgrad_s2_grid_y(const GP& p, int BM) { return p.cls_rows > 0 ? 4 * ((p.cls_rows + BM - 1) / BM) : (p.M + BM - 1) / BM; }

}  // namespace cbgemm
#include "gemm_epilogue.h"      // the generic option chain (epilogue_cols), the specialised bodies (fast_epilogue), tile_epilogue
namespace cbgemm {

// OCC = blocks per CU the register allocation must leave room for (__launch_bounds__'s second argument counts waves per SIMD;
// a 256-thread block puts one wave on each SIMD)
// One output tile of one problem: everything a workgroup of gemm_kernel / gemm_group_kernel does once it knows its (problem, tile).
template <typename T, int BM, int BN, typename LA, typename LB, int PF, bool RS, int OCC>
__device__ __forceinline__ void gemm_tile(GP& p, TileId bid, float* slab = nullptr, int* cnt = nullptr) {
    using X = Tr<T>;
    constexpr int BK = X::BK;
    constexpr int WM = BM / 2, WN = BN / 2, FM = WM / 16, FN = WN / 16;
    constexpr int TILE_A = BM * X::ROWB, TILE_B = BN * X::ROWB;
    constexpr int SMEM_BYTES = 2 * (TILE_A + TILE_B);
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    CB_STAMP_DECL();
    CB_STAMP(0);
#ifdef CB_STAMPS
    const unsigned stamp_lin = (unsigned)bid.bx + (unsigned)((p.N + BN - 1) / BN) * ((unsigned)bid.by + (unsigned)((p.M + BM - 1) / BM) * (unsigned)bid.bz);
#endif
    // index of this output tile among the problem's tiles (batch member outermost; K parts of one tile share it): GP::sq_slots
    const int tile_lin = ((p.batch > 1 ? bid.bz / p.split_k : 0) * ((p.M + BM - 1) / BM) + bid.by) * ((p.N + BN - 1) / BN) + bid.bx;
    apply_batch(p, bid);
    if constexpr (!LA::KROW && LB::KROW) dgrad_s2_class<BM, BK>(p, bid);
    const int m0 = bid.by * BM, n0 = bid.bx * BN;
    const int kt_per = (p.ktiles + p.split_k - 1) / p.split_k;
    const int kt0 = bid.bz * kt_per;
    const int nt = ((kt0 + kt_per < p.ktiles) ? kt0 + kt_per : p.ktiles) - kt0;
    if (nt <= 0) return;

    LA la;
    LB lb;
    {
        Opnd oa = {p.A, p.a_tab, p.lda, p.a_mode, p.a_bytes};
        Opnd ob = {p.B, p.b_tab, p.ldb, p.b_mode, p.b_bytes};
        la.init(p, oa, m0, p.M, kt0, tid);
        lb.init(p, ob, n0, p.N, kt0, tid);
    }
    typename LA::Stage sa[PF];
    typename LB::Stage sb[PF];

    // tiles are loaded strictly in order (the loaders advance their k position on every call)
    auto load_tiles = [&](typename LA::Stage& xa, typename LB::Stage& xb) {      // steady state: full K tiles only
        la.template load<false>(xa, p);
        lb.template load<false>(xb, p);
    };
    auto load_tiles_checked = [&](typename LA::Stage& xa, typename LB::Stage& xb) {
        la.template load<true>(xa, p);
        lb.template load<true>(xb, p);
    };
    auto store_tiles = [&](const typename LA::Stage& xa, const typename LB::Stage& xb, int buf) {
        unsigned char* As = smem + buf * (TILE_A + TILE_B);
        la.store(xa, As, tid);
        lb.store(xb, As + TILE_A, tid);
    };

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) { f32x4 z = {0.f, 0.f, 0.f, 0.f}; acc[i][j] = z; }
    // RS: row sums of A over k (bias gradients of a weight-gradient GEMM) ride on the matrix core: one extra MFMA per A
    // fragment against an all-ones B fragment, in the first column of blocks only
    f32x4 accr[RS ? FM : 1];
#pragma unroll
    for (int i = 0; i < (RS ? FM : 1); ++i) { f32x4 z = {0.f, 0.f, 0.f, 0.f}; accr[i] = z; }
    const bool rs_on = RS && p.a_rowsum != nullptr && bid.bx == 0 && wn == 0;     // wave-uniform

    // prologue: K-tile j lives in register stage j % PF
#pragma unroll
    for (int s = 0; s < PF; ++s)
        if (s < nt) load_tiles_checked(sa[s], sb[s]);
    // epilogue operands (residual, mask / GELU pre-activation) requested now, consumed after the K loop
    // Only the data-gradient forms carry it (the registers would cost the weight-gradient kernels occupancy), and only for the fused
    // ReLU x FrozenBN backward (two operands: block output y and the shortcut gradient): measured on MI355X -10 % there
    // (50176x512x128: 48.3 -> 42.7 us), nothing or slightly negative for single-operand epilogues (forward residual, GELU').
    // The 128x128 two-blocks-per-CU data-gradient kernel prefetches ONE operand, for the GELU' epilogue (dgrad of BertOutput.dense: the
    // 16 MB pre-activation would otherwise be requested by all blocks at once after their last MFMA).
    constexpr bool DGRAD = sizeof(T) == 2 && !LA::KROW && LB::KROW;
    constexpr int EPF = !DGRAD ? 0 : (BM * BN <= 128 * 64 ? 2 : (OCC >= 2 ? 1 : 0));
    EpiPre<BM, BN, EPF != 1> epre;
    const bool epf_on = EPF != 0 && p.c_vec8 && (EPF == 2 ? p.relu_bwd != 0 : (p.dact_pre != nullptr && !p.relu_bwd));      // block-uniform
    if constexpr (EPF != 0) {
        if (epf_on) epi_prefetch<T, BM, BN, EPF != 1>(p, epre, m0, n0, tid);
    }
    store_tiles(sa[0], sb[0], 0);
    if (PF < nt) load_tiles_checked(sa[0], sb[0]);
    __syncthreads();
    CB_STAMP(1);

    auto compute_tile = [&](int buf) {
        const unsigned char* As = smem + buf * (TILE_A + TILE_B);
        const unsigned char* Bs = As + TILE_A;
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int kk = 0; kk < BK / 32; ++kk) {
                bf16x8 af[FM], bfr[FN];
#pragma unroll
                for (int i = 0; i < FM; ++i) {
                    if constexpr (LA::TR) af[i] = tr_frag<BM>(As, wm * WM + i * 16, kk, lane);
                    else af[i] = *reinterpret_cast<const bf16x8*>(As + lds_off<T>(wm * WM + i * 16 + (lane & 15), kk * 4 + (lane >> 4)));
                }
#pragma unroll
                for (int j = 0; j < FN; ++j) {
                    if constexpr (LB::TR) bfr[j] = tr_frag<BN>(Bs, wn * WN + j * 16, kk, lane);
                    else bfr[j] = *reinterpret_cast<const bf16x8*>(Bs + lds_off<T>(wn * WN + j * 16 + (lane & 15), kk * 4 + (lane >> 4)));
                }
#pragma unroll
                for (int i = 0; i < FM; ++i)
#pragma unroll
                    for (int j = 0; j < FN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
                if constexpr (RS) {
                    if (rs_on) {
                        bf16x8 ones;
#pragma unroll
                        for (int e = 0; e < 8; ++e) ones[e] = (bf16)1.0f;
#pragma unroll
                        for (int i = 0; i < FM; ++i) accr[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, af[i], accr[i], 0, 0, 0);
                    }
                }
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk) {
                float af[FM], bfr[FN];
#pragma unroll
                for (int i = 0; i < FM; ++i)
                    af[i] = *reinterpret_cast<const float*>(As + lds_off<T>(wm * WM + i * 16 + (lane & 15), kk) + (lane >> 4) * 4);
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    bfr[j] = *reinterpret_cast<const float*>(Bs + lds_off<T>(wn * WN + j * 16 + (lane & 15), kk) + (lane >> 4) * 4);
#pragma unroll
                for (int i = 0; i < FM; ++i)
#pragma unroll
                    for (int j = 0; j < FN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bfr[j], af[i], acc[i][j], 0, 0, 0);
                if constexpr (RS) {
                    if (rs_on) {
#pragma unroll
                        for (int i = 0; i < FM; ++i) accr[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, af[i], accr[i], 0, 0, 0);
                    }
                }
            }
        }
    };

    int t = 0;
    // steady state: branch-free body (compute tile t, stage tile t+1 into LDS, issue the loads of tile t+1+PF),
    // so the PF register stages really stay in flight across iterations
    while (t + 2 * PF < nt - 1) {                 // ... and never the last (possibly partial) K tile
#pragma unroll
        for (int s = 0; s < PF; ++s) {            // t % PF == s: static register-stage indices
            const int S1 = (s + 1) % PF;
            compute_tile(t & 1);
            store_tiles(sa[S1], sb[S1], (t + 1) & 1);
            load_tiles(sa[S1], sb[S1]);
            __syncthreads();
            ++t;
        }
    }
    // tail: at most 2*PF+1 tiles, guarded (K tail handled by the checked loads)
    while (t < nt) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
            if (t < nt) {
                const int S1 = (s + 1) % PF;
                compute_tile(t & 1);
                if (t + 1 < nt) {
                    store_tiles(sa[S1], sb[S1], (t + 1) & 1);
                    if (t + 1 + PF < nt) load_tiles_checked(sa[S1], sb[S1]);
                }
                __syncthreads();
                ++t;
            }
        }
    }

    if constexpr (RS) {
        if (rs_on && (lane >> 4) == 0) {                 // every accumulator row holds the sum: take row 0 of lanes 0..15
#pragma unroll
            for (int i = 0; i < FM; ++i) {
                const int m = m0 + wm * WM + i * 16 + lane;
                if (m < p.M) atomicAdd(p.a_rowsum + m, accr[i][0]);
            }
        }
    }
    CB_STAMP(2);
    // ---- slab K split (grouped weight gradients, round 5) ------------------------------------------------------------------------
    // Instead of 64 KB of memory-side fp32 atomics per workgroup (profiles/r05w: 0.09 ms of the step), every K part of an output tile
    // writes its partial tile to scratch in the accumulators' own layout (16 B per lane, one contiguous 4 KB run per wave instruction)
    // and takes a ticket; the LAST part to arrive adds all parts IN PART ORDER and runs the ordinary epilogue once (C (+)= sum, row-
    // contiguous 32-byte stores).  The sum no longer depends on the order of arrival: the weight gradient is bit-reproducible.
    // Visibility across the XCDs' non-coherent L2s WITHOUT fences: the parts are stored write-through and loaded with device scope
    // (sc1 on both: the accesses of an agent-scope atomic store / load), the ticket is taken after s_waitcnt vmcnt(0) + a barrier.  A
    // __threadfence() pair here (buffer_wbl2 + buffer_inv: the whole L2 of the XCD invalidated once per workgroup) cost the co-resident
    // workgroups their operand reuse: +0.45 ms per step (profiles/r05x_slab_ksplit_ab.txt, first variant).
    if (slab != nullptr && p.split_k > 1) {                                 // (block-uniform)
        __shared__ int s_last;
        constexpr int SC1 = 16;
        const int tile_lin = bid.by * ((p.N + BN - 1) / BN) + bid.bx;
        const int parts = (p.ktiles + kt_per - 1) / kt_per;                 // K parts that hold K tiles (the others returned above)
        float* const base = slab + ((int64_t)p.slab_base + (int64_t)tile_lin * p.split_k) * (BM * BN);
        {
            const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base + (int64_t)bid.bz * (BM * BN), (short)0, BM * BN * 4, 0x00020000);
#pragma unroll
            for (int i = 0; i < BM / 32; ++i)
#pragma unroll
                for (int j = 0; j < BN / 32; ++j) {
                    union { f32x4 f; u32x4 r; } u;
                    u.f = acc[i][j];
                    __builtin_amdgcn_raw_buffer_store_b128(u.r, rs, (uint32_t)(((i * (BN / 32) + j) * NTHREADS + tid) * 16), 0, SC1);
                }
        }
        __builtin_amdgcn_s_waitcnt(0x0f70);                                 // vmcnt(0): this thread's parts have left for the memory side
        __syncthreads();
        if (tid == 0) s_last = atomicAdd(cnt + p.cnt_base + tile_lin, 1) == parts - 1;
        __syncthreads();
        if (!s_last) {
            CB_STAMP(3);
            CB_STAMP_FLUSH(p, stamp_lin, tid);
            return;
        }
#pragma unroll
        for (int i = 0; i < BM / 32; ++i)
#pragma unroll
            for (int j = 0; j < BN / 32; ++j) { f32x4 z = {0.f, 0.f, 0.f, 0.f}; acc[i][j] = z; }
#pragma unroll 2                                                                 // (two parts' loads in flight; the additions keep the part order)
        for (int z = 0; z < parts; ++z) {
            const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base + (int64_t)z * (BM * BN), (short)0, BM * BN * 4, 0x00020000);
#pragma unroll
            for (int i = 0; i < BM / 32; ++i)
#pragma unroll
                for (int j = 0; j < BN / 32; ++j) {
                    union { u32x4 r; f32x4 f; } u;
                    u.r = __builtin_amdgcn_raw_buffer_load_b128(rs, (uint32_t)(((i * (BN / 32) + j) * NTHREADS + tid) * 16), 0, SC1);
                    acc[i][j] += u.f;
                }
        }
        if (tid == 0) atomicExch(cnt + p.cnt_base + tile_lin, 0);           // ready for the next launch (same stream: ordered)
        p.split_k = 1;                                                      // the epilogue below is the plain one
    }
    constexpr int FORM_ = LA::KROW ? 0 : (LB::KROW ? 2 : 1);
    if constexpr (EPF != 0) tile_epilogue<T, BM, BN, SMEM_BYTES, EPF, false, FORM_>(p, acc, smem, m0, n0, tid, epre, epf_on);
    else tile_epilogue<T, BM, BN, SMEM_BYTES, 0, LA::KROW, FORM_>(p, acc, smem, m0, n0, tid, EpiPre<BM, BN, true>{}, false, tile_lin);
    CB_STAMP(3);
    CB_STAMP_FLUSH(p, stamp_lin, tid);
}

template <typename T, int BM, int BN, typename LA, typename LB, int PF, bool RS = false, int OCC = 1>
__global__ void __launch_bounds__(256, OCC) gemm_kernel(GP p) {
    gemm_tile<T, BM, BN, LA, LB, PF, RS, OCC>(p, tile_id(p));
}

// ---------------------------------------------------------------------------------------------
// Grouped launch (cb_gemm_group): up to GROUP_MAX independent problems of ONE kernel class (same tile, same loaders) share a
// grid.  The problem table travels in the kernel arguments (no device-side table to keep alive, capturable into a hipGraph as
// is); workgroup `lin` -- after the XCD-compact remap over the WHOLE grid, so that a problem's tiles stay on one L2 -- finds its
// problem by a scan over the prefix sums and then runs exactly gemm_kernel's tile code.  A launch of many small problems fills
// the chip where each of them alone is a fraction of a round of workgroups, and the problems' cold starts / store tails overlap.
// ---------------------------------------------------------------------------------------------
#ifdef CB_STAMPS
constexpr int GROUP_MAX = 9;          // (diagnostic build: GP carries the stamp pointer; the argument block must stay under 4 KiB)
#else
constexpr int GROUP_MAX = 10;
#endif
struct GroupArgs {
    int n, xcd_remap;
    int tile_end[GROUP_MAX];          // problem i owns workgroups [tile_end[i-1], tile_end[i])
    float* slab;                      // slab K split (gemm_tile): scratch for the partial tiles, and the per-tile arrival counters (zero
    int* cnt;                         // between launches); null: the split problems combine through fp32 atomics
    GP g[GROUP_MAX];
};
static_assert(sizeof(GroupArgs) + 256 <= 4096, "kernel arguments (+ the hidden ones) are limited to 4 KiB");

template <int BM, int BN>
__device__ __forceinline__ int group_locate(const GroupArgs& ga, TileId& bid) {
    const unsigned total = gridDim.x;
    unsigned lin = blockIdx.x;
    if (ga.xcd_remap) {
        const unsigned xcd = lin & 7u, i = lin >> 3;
        const unsigned q = total >> 3, r = total & 7u;
        lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
    }
    int pi = 0;
    while (pi + 1 < ga.n && lin >= (unsigned)ga.tile_end[pi]) ++pi;
    const unsigned local = lin - (pi > 0 ? (unsigned)ga.tile_end[pi - 1] : 0u);
    const unsigned gx = (unsigned)((ga.g[pi].N + BN - 1) / BN), gy = (unsigned)((ga.g[pi].M + BM - 1) / BM);
    bid.bx = (int)(local % gx);
    const unsigned rest = local / gx;
    bid.by = (int)(rest % gy);
    bid.bz = (int)(rest / gy);
    return pi;
}

template <typename T, int BM, int BN, typename LA, typename LB, int PF, bool RS = false, int OCC = 1>
__global__ void __launch_bounds__(256, OCC) gemm_group_kernel(GroupArgs ga) {
    TileId bid;
    const int pi = group_locate<BM, BN>(ga, bid);
    GP p = ga.g[pi];
    gemm_tile<T, BM, BN, LA, LB, PF, RS, OCC>(p, bid, ga.slab, ga.cnt);
}

// =============================================================================================
// LDS-DMA helpers (buffer_load_dwordx4 ... lds: no VGPR staging, no ds_write) shared by the 8-wave kernels (gemm8_impl.h) and the
// streaming kernel (gemm_stream_impl.h).  The LDS destination of an LDS-DMA is wave-uniform base + lane*16, so the XOR swizzles of the
// tile images are applied to each lane's SOURCE address.  (A 4-wave LDS-DMA ring kernel lived here in rounds 1-5: measured equal or
// slower than the register ring on every shape, profiles/r01_gemm_microbench.md, tools/dma_probe history -- deleted in round 6.)
// =============================================================================================
__device__ __forceinline__ void dma16(rsrc_t rs, unsigned char* lds_wave_base, uint32_t voff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_wave_base, 16, voff, 0, 0, 0);
}
// s_waitcnt vmcnt(N) only (expcnt / lgkmcnt fields left at "no wait")
#define CB_WAIT_VMCNT(N) __builtin_amdgcn_s_waitcnt((((N) & 15) | (7 << 4) | (15 << 8) | ((((N) >> 4) & 3) << 14)))

// LDS-only synchronisation of a workgroup: this wave's ds_* have completed (lgkmcnt(0); vmcnt / expcnt fields left at "no wait"), then
// the barrier.  The empty asm statements keep the COMPILER from moving memory accesses across it (the barrier intrinsic alone is not a
// memory operation to LLVM).
#define CB_LDS_BARRIER() do { asm volatile("" ::: "memory"); __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)

// ROWK image [rows][128 B], 16-byte segment s of row r stored at segment s ^ (r & 7)  (same image as RowkFast)
template <int ROWS, bool GATHER> struct RowkDma {
    using X = Tr<bf16>;
    static constexpr bool TR = false;
    static constexpr int NI = ROWS / 8 / 4;            // 1-KiB DMA instructions per wave per tile
    rsrc_t rs;
    uint32_t voff[NI];
    int ih[NI], iw[NI];
    int c, rr, ss, krem;

    __device__ __forceinline__ void init(const GP& p, const Opnd& o, int row0, int bound, int kt0, int tid) {
        rs = make_rsrc(o.base, o.bytes);
        const int lane = tid & 63, wave = tid >> 6;
        const int rin = lane >> 3;                                   // row within the 8-row group (= row & 7)
        const int lseg = (lane & 7) ^ rin;                           // logical segment this lane fetches
        const int k = kt0 * X::BK + lseg * 8;
        c = k; rr = 0; ss = 0; krem = p.K - k;
        if constexpr (GATHER) {
            int tap = k / p.Ct;
            c = k - tap * p.Ct;
            rr = tap / p.S; ss = tap - rr * p.S;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int row = row0 + (i * 4 + wave) * 8 + rin;
            const bool ok = row < bound;
            ih[i] = 0; iw[i] = 0;
            if constexpr (GATHER) {
                cb_pixel px = {0, 0, 0};
                if (ok) px = o.tab[row];
                ih[i] = px.ih0; iw[i] = px.iw0;
                voff[i] = ok ? (uint32_t)px.off * 2u : OOB;
            } else {
                voff[i] = ok ? ((uint32_t)row * (uint32_t)o.ld + (uint32_t)k) * 2u : OOB;
            }
        }
    }
    template <bool CHECK> __device__ __forceinline__ void issue(const GP& p, unsigned char* tile, int wave) {
        if constexpr (GATHER) {
            const bool kv = rr < p.R;
            const uint32_t koff = (uint32_t)(rr * (int)p.sH + ss * (int)p.sW + c) * 2u;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const bool v = kv && (unsigned)(ih[i] + rr) < (unsigned)p.H && (unsigned)(iw[i] + ss) < (unsigned)p.W;
                dma16(rs, tile + (i * 4 + wave) * 1024, v ? voff[i] + koff : OOB);
            }
            if (p.Ct >= X::BK) {
                c += X::BK;
                if (c >= p.Ct) { c -= p.Ct; if (++ss == p.S) { ss = 0; ++rr; } }
            } else {
                ss += X::BK / p.Ct;
                while (ss >= p.S) { ss -= p.S; ++rr; }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                uint32_t o32 = voff[i];
                if (CHECK && krem <= 0) o32 = OOB;
                dma16(rs, tile + (i * 4 + wave) * 1024, o32);
                voff[i] += X::BK * 2u;
            }
            krem -= X::BK;
        }
    }
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T, int BM, int BN, int PF, int OCC, typename LA, typename LB, bool RS = false>
int launch_k(const GP& p, hipStream_t st) {
    dim3 grid((p.N + BN - 1) / BN, dgrad_s2_grid_y(p, BM), p.split_k * (p.batch > 1 ? p.batch : 1));
    hipLaunchKernelGGL((gemm_kernel<T, BM, BN, LA, LB, PF, RS, OCC>), grid, dim3(NTHREADS), 0, st, p);
    return cb_launch_status("cb_gemm");
}
// weight-gradient form (both operands KROW): with or without the fused row sums of A
template <typename T, int BM, int BN, int PF, int OCC, typename LA, typename LB>
int launch_wgrad(const GP& p, hipStream_t st) {
    if (p.a_rowsum) return launch_k<T, BM, BN, PF, OCC, LA, LB, true>(p, st);
    return launch_k<T, BM, BN, PF, OCC, LA, LB, false>(p, st);
}

// addressing-mode dispatch: lean compile-time loaders on the fast path, the generic loaders otherwise
template <typename T, int BM, int BN, int PF, int OCC = 1>
int launch_gemm(const GP& p, bool fast, hipStream_t st) {
    const bool a_krow = p.a_mode == CB_KROW;
    const bool b_krow = p.b_mode != CB_ROWK;
    if (a_krow && !b_krow) return cb_fail("cb_gemm: unsupported operand mode combination (A KROW with B ROWK)");
    if (fast) {
        const int taps = p.R * p.S;
        if constexpr (sizeof(T) == 2) {
            // measured on MI355X: next to a ROWK operand the transpose-read image wins for 64-row tiles, the
            // register transpose (KB = 4, all 256 threads) for 128-row tiles; with two KROW operands the
            // transpose-read image wins for both tile sizes (profiles/r01_gemm_microbench.md)
            if constexpr (BN < 128) {
                if (p.a_mode == CB_ROWK && (p.b_mode == CB_KROW || (p.b_mode == CB_KROW_TAPS && taps == 1)))
                    return launch_k<T, BM, BN, PF, OCC, RowkFast<T, BM, false>, KrowTr<BN, KM_PLAIN>>(p, st);
                if (p.a_mode == CB_ROWK_GATHER && p.b_mode == CB_KROW_TAPS && p.Ct % Tr<bf16>::BK == 0)
                    return launch_k<T, BM, BN, PF, OCC, RowkFast<T, BM, true>, KrowTr<BN, KM_TAPS>>(p, st);
            }
            if (p.a_mode == CB_KROW && p.b_mode == CB_KROW)
                return launch_wgrad<T, BM, BN, PF, OCC, KrowTr<BM, KM_PLAIN>, KrowTr<BN, KM_PLAIN>>(p, st);
            if (p.a_mode == CB_KROW && p.b_mode == CB_KROW_GATHER)
                return launch_k<T, BM, BN, PF, OCC, KrowTr<BM, KM_PLAIN>, KrowTr<BN, KM_GATHER>>(p, st);
        }
        if (p.a_mode == CB_ROWK && p.b_mode == CB_ROWK)
            return launch_k<T, BM, BN, PF, OCC, RowkFast<T, BM, false>, RowkFast<T, BN, false>>(p, st);
        if (p.a_mode == CB_ROWK_GATHER && p.b_mode == CB_ROWK)
            return launch_k<T, BM, BN, PF, OCC, RowkFast<T, BM, true>, RowkFast<T, BN, false>>(p, st);
        // fp32 parity mode (and odd channel counts): register-transposing loaders.  One KROW operand next to a ROWK
        // one is spread over all 256 threads; two KROW operands take half the threads each (B shifted by 128)
        constexpr int KB1B = BN >= 128 ? 4 : 2;
        constexpr int KB2A = BM >= 128 ? 8 : 4, KB2B = BN >= 128 ? 8 : 4;
        if (p.a_mode == CB_ROWK && (p.b_mode == CB_KROW || (p.b_mode == CB_KROW_TAPS && taps == 1)))
            return launch_k<T, BM, BN, PF, OCC, RowkFast<T, BM, false>, KrowFast<T, BN, KM_PLAIN, KB1B, 0>>(p, st);
        if (p.a_mode == CB_ROWK_GATHER && p.b_mode == CB_KROW_TAPS)
            return launch_k<T, BM, BN, PF, OCC, RowkFast<T, BM, true>, KrowFast<T, BN, KM_TAPS, KB1B, 0>>(p, st);
        if (p.a_mode == CB_KROW && p.b_mode == CB_KROW)
            return launch_wgrad<T, BM, BN, PF, OCC, KrowFast<T, BM, KM_PLAIN, KB2A, 0>, KrowFast<T, BN, KM_PLAIN, KB2B, 128>>(p, st);
        if (p.a_mode == CB_KROW && p.b_mode == CB_KROW_GATHER)
            return launch_k<T, BM, BN, PF, OCC, KrowFast<T, BM, KM_PLAIN, KB2A, 0>, KrowFast<T, BN, KM_GATHER, KB2B, 128>>(p, st);
    }
    if (!a_krow && !b_krow) return launch_k<T, BM, BN, PF, OCC, RowkLoader<T, BM, false>, RowkLoader<T, BN, false>>(p, st);
    if (!a_krow) return launch_k<T, BM, BN, PF, OCC, RowkLoader<T, BM, false>, KrowLoader<T, BN, false>>(p, st);
    if (p.b_mode == CB_KROW) return launch_wgrad<T, BM, BN, PF, OCC, KrowLoader<T, BM, false>, KrowLoader<T, BN, false>>(p, st);
    return launch_k<T, BM, BN, PF, OCC, KrowLoader<T, BM, false>, KrowLoader<T, BN, false>>(p, st);
}

// ---- grouped launches: the kernel classes cb_gemm_group covers (fast path only; everything else is launched problem by problem)
enum { GC_WGRAD = 0,        // A KROW, B KROW            (weight gradient of a Linear / 1x1 stride-1 convolution)
       GC_WGRAD_GATHER = 1, // A KROW, B KROW_GATHER     (weight gradient of a convolution: pixels gathered)
       GC_FWD = 2,          // A ROWK, B ROWK            (Linear / 1x1 stride-1 convolution forward)
       GC_FWD_GATHER = 3,   // A ROWK_GATHER, B ROWK     (convolution forward)
       GC_WGRAD_RS = 4,     // GC_WGRAD whose members may carry a_rowsum (bias gradients as MFMA row sums) and a strided batch: the encoder's
                            // four kinds of 12-layer weight gradients in ONE launch (bf16, 128x128 two-per-CU tile only)
       GC_COUNT = 5 };

// launcher of a grouped kernel: the loaders of the group's class (GC_*)
template <typename T, int BM, int BN, int PF, int OCC>
int launch_gemm_group(const GroupArgs& ga, int cls, hipStream_t st) {
    const dim3 grid((unsigned)ga.tile_end[ga.n - 1]);
    if constexpr (sizeof(T) == 2 && BM == 128 && BN == 128 && OCC == 2) {
        if (cls == GC_WGRAD_RS) {
            hipLaunchKernelGGL((gemm_group_kernel<T, BM, BN, KrowTr<BM, KM_PLAIN>, KrowTr<BN, KM_PLAIN>, PF, true, OCC>), grid, dim3(NTHREADS), 0, st, ga);
            return cb_launch_status("cb_gemm_group");
        }
    }
#define CB_LAUNCH_GROUP(LA_, LB_)                                                                                     \
    do {                                                                                                              \
        hipLaunchKernelGGL((gemm_group_kernel<T, BM, BN, LA_, LB_, PF, false, OCC>), grid, dim3(NTHREADS), 0, st, ga); \
        return cb_launch_status("cb_gemm_group");                                                                     \
    } while (0)
    using RA0 = RowkFast<T, BM, false>; using RA1 = RowkFast<T, BM, true>; using RB0 = RowkFast<T, BN, false>;
    if constexpr (sizeof(T) == 2) {
        using KA = KrowTr<BM, KM_PLAIN>; using KB0 = KrowTr<BN, KM_PLAIN>; using KB2 = KrowTr<BN, KM_GATHER>;
        if (cls == GC_WGRAD) CB_LAUNCH_GROUP(KA, KB0);
        if (cls == GC_WGRAD_GATHER) CB_LAUNCH_GROUP(KA, KB2);
    } else {
        constexpr int KB2A = BM >= 128 ? 8 : 4, KB2B = BN >= 128 ? 8 : 4;
        using KA = KrowFast<T, BM, KM_PLAIN, KB2A, 0>; using KB0 = KrowFast<T, BN, KM_PLAIN, KB2B, 128>; using KB2 = KrowFast<T, BN, KM_GATHER, KB2B, 128>;
        if (cls == GC_WGRAD) CB_LAUNCH_GROUP(KA, KB0);
        if (cls == GC_WGRAD_GATHER) CB_LAUNCH_GROUP(KA, KB2);
    }
    if (cls == GC_FWD) CB_LAUNCH_GROUP(RA0, RB0);
    if (cls == GC_FWD_GATHER) CB_LAUNCH_GROUP(RA1, RB0);
#undef CB_LAUNCH_GROUP
    return cb_fail("cb_gemm_group: unknown kernel class %d", cls);
}

}  // namespace cbgemm
