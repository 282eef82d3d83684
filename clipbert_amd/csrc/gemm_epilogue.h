// Epilogues of the cb_gemm kernels: the generic option chain (epilogue_cols: every option of cb_gemm_desc, written ONCE for the three
// widths the kernels use), the specialised bodies of the training step's option combinations (fast_epilogue) and the tile epilogue of
// the 4-wave kernels (tile_epilogue).  Included by gemm_impl.h, behind GP, the EF_* flags and the buffer-descriptor helpers it uses: not
// a stand-alone header.
#pragma once

namespace cbgemm {

// activation of one element: the bf16 mode's GELU is the packed evaluation everywhere (common.h gelu_erf_both2), the fp32 parity mode's
// the 1.5e-7 scalar one
template <typename T>
__device__ __forceinline__ float act_of(int act, float v) {
    if constexpr (sizeof(T) == 2) {
        if (act == CB_ACT_GELU || act == CB_ACT_GELU_SAVE_GRAD) return gelu_erf_pk(v);
    }
    return apply_act(act, v);
}

// FrozenBN / bias-with-scale: x * scale + shift.  bf16 mode: ONE fused multiply-add, written as such in every path of the library, so that
// kernels of different structure stay bit-identical whatever -ffp-contract decides per call site.  fp32 parity mode: the product is
// rounded before the addition -- the two roundings of the reference's `x * self.weight + self.bias` (and of the oracle), so that ReLU
// masks and max-pool ties downstream are decided on the same bits (tests/test_model_small.py holds the emulator build to 2e-3 per element).
template <typename T>
__device__ __forceinline__ float scale_shift(float x, float sc, float sh) {
    if constexpr (sizeof(T) == 2) return __builtin_fmaf(x, sc, sh);
    else {
#pragma clang fp contract(off)
        const float t = x * sc;
        return t + sh;
    }
}

// 8 consecutive elements <-> float[8] (one 16-byte bf16 / two 16-byte fp32 accesses)
__device__ __forceinline__ void load8(const float* q, float (&v)[8]) {
    f32x4 a = load4(q), b = load4(q + 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) { v[r] = a[r]; v[4 + r] = b[r]; }
}
__device__ __forceinline__ void load8(const bf16* q, float (&v)[8]) {
    bf16x8 x = *reinterpret_cast<const bf16x8*>(q);
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = (float)x[r];
}
__device__ __forceinline__ void store8(float* q, const float (&v)[8]) {
    f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
    store4(q, a); store4(q + 4, b);
}
__device__ __forceinline__ void store8(bf16* q, const float (&v)[8]) {
    bf16x8 x;
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = (bf16)v[r];
    *reinterpret_cast<bf16x8*>(q) = x;
}

// Write-through form of store8 (bf16): `global_store_dwordx4 ... sc1` through a buffer descriptor over C.  A plain store leaves its line
// dirty in the XCD's L2 until the end-of-kernel release writes everything back in one burst (MI355X_MICROARCH.md "boundary": + B / 6 TB/s
// behind B dirty bytes); a write-through store sends the bytes to the memory side while the other workgroups still compute.
template <int AUX = 16 /* sc1 */>
__device__ __forceinline__ void store8_wt(void* base, int64_t elem_off, const float (&v)[8]) {
    union { bf16x8 x; u32x4 r; } u;
#pragma unroll
    for (int r = 0; r < 8; ++r) u.x[r] = (bf16)v[r];
    const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)0xffffffffu, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(u.r, rs, (uint32_t)(elem_off * 2), 0, AUX);
}

// stride-2 scatter (zero_fill_pitch): the other three pixels of output pixel m's 2x2 input patch receive zeros
template <typename T>
__device__ __forceinline__ void zero_patch8(T* base, int64_t ld, int64_t orow, int n, int pitch) {
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    store8(base + (orow + 1) * ld + n, z);
    store8(base + (orow + pitch) * ld + n, z);
    store8(base + (orow + pitch + 1) * ld + n, z);
}

// ---------------------------------------------------------------------------------------------
// The generic epilogue: W consecutive columns n .. n+W-1 of row m.  ONE option chain for the three widths (same math, bit for bit):
//   W = 8  row-contiguous: every global access is a full 16-byte lane access and a wave touches whole cache lines (GP::c_vec8 -- N and
//          every leading dimension a multiple of 8, 16-byte-aligned bases; 4-wave, 8-wave and streaming kernels, the slab reduce)
//   W = 4  one accumulator fragment in the MFMA register layout (GP::c_vec: multiples of 4) and the few-rows kernel
//   W = 1  ragged N edge / unaligned operands
// What depends on the width lives in the helpers below.
// ---------------------------------------------------------------------------------------------
// f(r) for each of the W columns, unrolled (the columns live in registers)
template <int W, typename F>
__device__ __forceinline__ void each_col(F f) {
#pragma unroll
    for (int r = 0; r < W; ++r) f(r);
}
// W consecutive elements <-> float[W]: 16-byte accesses (load8 / store8), one 16- or 8-byte access (load4 / store4), one element
template <int W, typename S>
__device__ __forceinline__ void load_cols(const S* q, float (&v)[W]) {
    if constexpr (W == 8) load8(q, v);
    else if constexpr (W == 4) { const f32x4 a = load4(q); each_col<4>([&](int r) { v[r] = a[r]; }); }
    else v[0] = to_f32(*q);
}
template <int W, typename S>
__device__ __forceinline__ void store_cols(S* q, const float (&v)[W]) {
    if constexpr (W == 8) store8(q, v);
    else if constexpr (W == 4) store4(q, f32x4{v[0], v[1], v[2], v[3]});
    else *q = from_f32<S>(v[0]);
}
// the per-column scale / shift a thread loads once for all its rows
template <int W>
__device__ __forceinline__ void load_scale_shift(const GP& p, int n, float (&sc)[W], float (&sh)[W]) {
    if (p.scale) load_cols(p.scale + n, sc);
    if (p.shift) load_cols(p.shift + n, sh);
}
// dropout multipliers of the site's groups of four columns (common.h): W / 4 whole groups, or one element of a group
template <int W>
__device__ __forceinline__ void dropout_cols(const GP& p, int m, int n, float (&v)[W]) {
    const uint64_t grp = (uint64_t)m * ((p.N + 3) >> 2) + (n >> 2);
    if constexpr (W == 1) v[0] *= dropout_mult1(p.seed, grp, n & 3, p.dropout_p);
    else {
#pragma unroll
        for (int g = 0; g < W / 4; ++g) {
            const f32x4 d = dropout_mult4(p.seed, grp + g, p.dropout_p);
            each_col<4>([&](int r) { v[4 * g + r] *= d[r]; });
        }
    }
}
// v = gelu(v), dv = gelu'(v), one evaluation for both: the bf16 mode's packed form in pairs (its scalar face for a single column)
template <typename T, int W>
__device__ __forceinline__ void gelu_both_cols(float (&v)[W], float (&dv)[W]) {
    if constexpr (sizeof(T) != 2) each_col<W>([&](int r) { gelu_erf_both(v[r], v[r], dv[r]); });
    else if constexpr (W == 1) gelu_erf_both_pk(v[0], v[0], dv[0]);
    else {
#pragma unroll
        for (int r = 0; r < W; r += 2) {
            f32x2 y, dy;
            gelu_erf_both2(f32x2{v[r], v[r + 1]}, y, dy);
            v[r] = y[0]; v[r + 1] = y[1]; dv[r] = dy[0]; dv[r + 1] = dy[1];
        }
    }
}

// sc / sh: the per-column scale / shift (load_scale_shift; read only where GP::scale / GP::shift are set).
// RMAP: the residual is read at row `rrow` (GP::res_rowmap's entry, -1: none) instead of orow; the 4-wave kernels' tile_epilogue
// instantiates RMAP = true only, every other caller false.
// Options of the row-contiguous width only (`if constexpr (W == 8)`), and what keeps them from the other two:
//   EPF    the residual / (mask | GELU pre-activation) chunk was fetched before the K loop (epi_prefetch: rpre / apre hold it) --
//          a template argument that only tile_epilogue's c_vec8 branch and the streaming kernel pass.
//   zfill  gemm_choose requires lp.c_vec8 for zero_fill_pitch on the 4-wave kernels; the 8-wave tiles always run W = 8; the streaming
//          kernel, the few-rows kernel (skinny_covers) and the grouped launches (group_class) refuse it.
//   wt     NOT guaranteed by the host: gemm_prepare sets GP::wt from dtype and extent alone, whether or not c_vec8 holds.  It means
//          "write-through where the stores are 16-byte rows"; the narrower widths ignore it and store plainly, as they always have.
// The fp32 atomic store (split_k > 1) is the reverse, W < 8 only: gemm_choose and group_launch clear c_vec8 when K parts combine
// through atomics; the slab K split (gemm_tile; 8-wave tiles + splitk_reduce_kernel) runs its epilogue with split_k = 1; the streaming
// and few-rows kernels refuse a K split.
template <typename T, int W, int EPF = 0, bool RMAP = false>
__device__ __forceinline__ void epilogue_cols(const GP& p, float (&v)[W], const float (&sc)[W], const float (&sh)[W],
                                              int m, int64_t orow, int n, bf16x8 rpre = bf16x8{}, bf16x8 apre = bf16x8{}, int64_t rrow = 0) {
    static_assert((W == 8 || W == 4 || W == 1) && (EPF == 0 || W == 8), "epilogue width");
    if constexpr (!RMAP) rrow = orow;
    const bool has_res = p.residual != nullptr && (!RMAP || rrow >= 0);      // (a prefetched chunk of a row without residual holds zeros)
    const int64_t coff = orow * p.ldc + n, c2off = orow * p.ldc2 + n;
    float t[W];                                                              // the M x N operand being applied
    auto load_res = [&] {
        if constexpr (EPF == 2) each_col<W>([&](int r) { t[r] = (float)rpre[r]; });
        else load_cols(reinterpret_cast<const T*>(p.residual) + rrow * p.ldr + n, t);
    };
    auto load_aux = [&](const void* base, int64_t ld) {
        if constexpr (EPF >= 1) each_col<W>([&](int r) { t[r] = (float)apre[r]; });
        else load_cols(reinterpret_cast<const T*>(base) + orow * ld + n, t);
    };
    auto add_t = [&] { each_col<W>([&](int r) { v[r] += t[r]; }); };
    auto mul_t = [&](float (&x)[W]) { each_col<W>([&](int r) { x[r] *= t[r]; }); };
    auto keep_t = [&] { each_col<W>([&](int r) { v[r] = t[r] > 0.f ? v[r] : 0.f; }); };          // v where t > 0, else 0
    // a T output (C or C2) at element offset off; nt: the forward's second output, next read in the backward (GP::wt & 2: sc1 + nt)
    auto store_t = [&](void* base, int64_t off, const float (&x)[W], bool nt = false) {
        if constexpr (W == 8 && sizeof(T) == 2) {
            if (nt && (p.wt & 2)) { store8_wt<18>(base, off, x); return; }
            if (p.wt) { store8_wt(base, off, x); return; }
        }
        store_cols(reinterpret_cast<T*>(base) + off, x);
    };
    auto zero_fill = [&] {
        if constexpr (W == 8) {
            if (!p.zfill) return;
            if (p.c_f32) zero_patch8(reinterpret_cast<float*>(p.C), p.ldc, orow, n, p.zfill);
            else zero_patch8(reinterpret_cast<T*>(p.C), p.ldc, orow, n, p.zfill);
            if (p.C2) zero_patch8(reinterpret_cast<T*>(p.C2), p.ldc2, orow, n, p.zfill);
        }
    };
    each_col<W>([&](int r) { v[r] *= p.alpha; });
    if (p.relu_bwd) {          // t = (acc [+ C] [+ residual]) where mask > 0;  C2 = t * post_scale2,  C = t * post_scale
        if (p.accumulate) { load_cols(reinterpret_cast<const T*>(p.C) + coff, t); add_t(); }
        if (has_res) { load_res(); add_t(); }
        load_aux(p.mask, p.ldm); keep_t();
        if (p.C2) {
            float u[W];
            each_col<W>([&](int r) { u[r] = v[r]; });
            if (p.post_scale2) { load_cols(p.post_scale2 + n, t); mul_t(u); }
            store_t(p.C2, c2off, u);
        }
        if (p.post_scale) { load_cols(p.post_scale + n, t); mul_t(v); }
        store_t(p.C, coff, v);
        zero_fill();
        return;
    }
    // scale and shift together are ONE fused multiply-add, written as such in every path of the library (this one, fast_epilogue,
    // cb_stem_pool, cb_res2_block): kernels of different structure stay bit-identical whatever -ffp-contract decides per call site
    if (p.scale && p.shift) each_col<W>([&](int r) { v[r] = scale_shift<T>(v[r], sc[r], sh[r]); });
    else if (p.scale) each_col<W>([&](int r) { v[r] *= sc[r]; });
    else if (p.shift) each_col<W>([&](int r) { v[r] += sh[r]; });
    const bool save_grad = p.act == CB_ACT_GELU_SAVE_GRAD && p.C2 != nullptr;        // C = gelu(v), C2 = gelu'(v): one evaluation for both
    float dv[W];
    if (save_grad) gelu_both_cols<T>(v, dv);
    if (p.C2) store_t(p.C2, c2off, save_grad ? dv : v, true);
    if (p.act != CB_ACT_NONE && !save_grad) each_col<W>([&](int r) { v[r] = act_of<T>(p.act, v[r]); });
    if (p.dropout_p > 0.f) dropout_cols(p, m, n, v);
    if (has_res) { load_res(); add_t(); }
    if (p.relu_after) each_col<W>([&](int r) { v[r] = v[r] > 0.f ? v[r] : 0.f; });
    if (p.mask) { load_aux(p.mask, p.ldm); keep_t(); }                               // (a mask AND a stored derivative: gemm_prepare refuses)
    else if (p.dact_pre) {                                                           // x the stored gelu', or gelu' of the stored pre-activation
        load_aux(p.dact_pre, p.ldd);
        if (p.act == CB_ACT_SAVED_GRAD) mul_t(v);
        else each_col<W>([&](int r) { v[r] *= gelu_erf_grad(t[r]); });
    }
    if (p.c_f32) {
        float* c = reinterpret_cast<float*>(p.C) + coff;
        if constexpr (W < 8) {
            if (p.split_k > 1) { each_col<W>([&](int r) { atomicAdd(c + r, v[r]); }); return; }      // K parts combine in place
        }
        if (p.accumulate) { load_cols(c, t); add_t(); }
        store_cols(c, v);
    } else {
        if (p.accumulate) { load_cols(reinterpret_cast<const T*>(p.C) + coff, t); add_t(); }
        store_t(p.C, coff, v);
    }
    zero_fill();
}

// ---------------------------------------------------------------------------------------------
// fast_epilogue<FLAGS, NT, BN, PR, NPASS>: the specialised row-contiguous bf16 epilogue of a tile (see FAST_EPI_COMBOS).  Geometry as in
// tile_epilogue / tile_epilogue8w: NT threads, NPASS passes of PR tile rows through the staging area [PR][BN * 4 + 16 B]; `stage(h)` writes
// the calling thread's share of pass h's accumulators (the caller knows its wave grid).  A thread owns the 8-column chunk cc = tid % (BN / 8)
// of the rows rl0 + it * (NT / CPR), it < ITER, of every pass.  The M x N operands of ALL chunks of a pass (of all passes when there are
// at most 8 chunks) are requested before the pass's first barrier: they land while the tile is staged.  The pass loop stays rolled when
// there are more than two passes, and for the GELU body (~2 KB): one warm copy in the instruction cache.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u32x4 pack_bf16x8(const f32x2 (&v)[4]) {
    union { bf16x8 x; u32x4 r; } u;
#pragma unroll
    for (int r = 0; r < 4; ++r) { u.x[2 * r] = (bf16)v[r][0]; u.x[2 * r + 1] = (bf16)v[r][1]; }
    return u.r;
}
__device__ __forceinline__ void unpack_bf16x8(u32x4 raw, f32x2 (&v)[4]) {
    union { u32x4 r; bf16x8 x; } u;
    u.r = raw;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = f32x2{(float)u.x[2 * r], (float)u.x[2 * r + 1]};
}

// pre_r / pre_a: the residual / (mask | stored derivative) chunks already in registers (epi_prefetch: requested before the K loop), in
// the slot order h * ITER + it; null: requested here.
template <int FLAGS, int NT, int BN, int PR, int NPASS, typename StageFn>
__device__ __forceinline__ void fast_epilogue(const GP& p, unsigned char* smem, int m0, int n0, int tid, StageFn stage, const bf16x8* pre_r = nullptr,
                                              const bf16x8* pre_a = nullptr, int tile_lin = 0) {
    constexpr int SROW = BN * 4 + 16, CPR = BN / 8, ITER = PR * CPR / NT, RSTEP = NT / CPR, NCH = NPASS * ITER;
    static_assert(PR * CPR % NT == 0 && NT % CPR == 0, "chunk map");
    constexpr bool HAS_RES = (FLAGS & EF_RES) != 0, HAS_AUX = (FLAGS & (EF_MASK | EF_MULAUX | EF_RBWD)) != 0;
    constexpr bool ALL = NCH <= 8;                               // every chunk's operands in flight at once, else pass by pass
    constexpr bool ROLL = (FLAGS & (EF_GELU2 | EF_GELU1)) != 0 || NPASS > 2;
    const int cc = tid % CPR, n = n0 + cc * 8, rl0 = tid / CPR;
    const bool nok = n < p.N;
    const unsigned char* const read_base = smem + rl0 * SROW + cc * 32;
    const rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(p.C, (short)0, (int)0xffffffffu, 0x00020000);
    const rsrc_t rc2 = __builtin_amdgcn_make_buffer_rsrc((FLAGS & (EF_GELU2 | EF_RBWD)) ? p.C2 : p.C, (short)0, (int)0xffffffffu, 0x00020000);
    constexpr uint32_t CESZ = (FLAGS & EF_F32) ? 4u : 2u;         // bytes per element of C
    const uint32_t ldcb = (uint32_t)p.ldc * CESZ, ldc2b = (uint32_t)p.ldc2 * 2u, nb = (uint32_t)n * 2u;
    float sq = 0.f;                                              // EF_F32: this thread's share of sum(C^2)
    // operands are read through range-checked descriptors: rows past M (and chunks past N) take the out-of-range offset and read zeros
    // (EF_RMAP: the residual has its own row count -- the host checked that it ends below 2 GiB, and a row without residual takes OOB)
    constexpr bool RMAP = (FLAGS & EF_RMAP) != 0, CMAP = (FLAGS & EF_CMAP) != 0;
    const rsrc_t rr = make_rsrc(HAS_RES ? p.residual : p.C, HAS_RES ? (RMAP ? OOB : (uint32_t)((int64_t)p.M * p.ldr * 2)) : 0u);
    const void* auxp = (FLAGS & (EF_MASK | EF_RBWD)) ? p.mask : p.dact_pre;
    const int64_t lda = (FLAGS & (EF_MASK | EF_RBWD)) ? p.ldm : p.ldd;
    const rsrc_t ra = make_rsrc(HAS_AUX ? auxp : p.C, HAS_AUX ? (CMAP ? OOB : (uint32_t)((int64_t)p.M * lda * 2)) : 0u);
    // (EF_CMAP: the mapped rows run over the whole output, which the host checked to end below 2 GiB)
    auto out_row = [&](int m) __attribute__((always_inline)) { if constexpr (CMAP) return (uint32_t)p.c_rowmap[m]; else return (uint32_t)m; };
    const uint32_t ldrb = (uint32_t)p.ldr * 2u, ldab = (uint32_t)lda * 2u;
    f32x2 sc[4], sh[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { sc[r] = f32x2{1.f, 1.f}; sh[r] = f32x2{0.f, 0.f}; }
    if (nok) {
        if constexpr ((FLAGS & EF_SCALE) != 0) {
            const f32x4 a = load4(p.scale + n), b = load4(p.scale + n + 4);
            sc[0] = f32x2{a[0], a[1]}; sc[1] = f32x2{a[2], a[3]}; sc[2] = f32x2{b[0], b[1]}; sc[3] = f32x2{b[2], b[3]};
        }
        if constexpr ((FLAGS & EF_SHIFT) != 0) {
            const f32x4 a = load4(p.shift + n), b = load4(p.shift + n + 4);
            sh[0] = f32x2{a[0], a[1]}; sh[1] = f32x2{a[2], a[3]}; sh[2] = f32x2{b[0], b[1]}; sh[3] = f32x2{b[2], b[3]};
        }
        if constexpr ((FLAGS & EF_RBWD) != 0) {                  // (sc / sh hold post_scale / post_scale2)
            const f32x4 a = load4(p.post_scale + n), b = load4(p.post_scale + n + 4);
            sc[0] = f32x2{a[0], a[1]}; sc[1] = f32x2{a[2], a[3]}; sc[2] = f32x2{b[0], b[1]}; sc[3] = f32x2{b[2], b[3]};
            if constexpr ((FLAGS & EF_PS2) != 0) {
                const f32x4 c = load4(p.post_scale2 + n), e = load4(p.post_scale2 + n + 4);
                sh[0] = f32x2{c[0], c[1]}; sh[1] = f32x2{c[2], c[3]}; sh[2] = f32x2{e[0], e[1]}; sh[3] = f32x2{e[2], e[3]};
            }
        }
    }
    u32x4 res[HAS_RES ? (ALL ? NCH : ITER) : 1], aux[HAS_AUX ? (ALL ? NCH : ITER) : 1];
    auto request = [&](int h) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int m = m0 + h * PR + rl0 + it * RSTEP;
            const bool ok = m < p.M && nok;
            const int slot = (ALL ? h * ITER : 0) + it;
            if constexpr (HAS_RES) {
                if (ALL && pre_r) { union { bf16x8 x; u32x4 r; } u; u.x = pre_r[h * ITER + it]; res[slot] = u.r; }
                else if constexpr (RMAP) {
                    const int rm = ok ? p.res_rowmap[m] : -1;
                    res[slot] = bload16(rr, rm >= 0 ? (uint32_t)rm * ldrb + nb : OOB);
                } else res[slot] = bload16(rr, ok ? (uint32_t)m * ldrb + nb : OOB);
            }
            if constexpr (HAS_AUX) {
                if (ALL && pre_a) { union { bf16x8 x; u32x4 r; } u; u.x = pre_a[h * ITER + it]; aux[slot] = u.r; }
                else aux[slot] = bload16(ra, ok ? out_row(ok ? m : 0) * ldab + nb : OOB);
            }
        }
    };
    auto chunk = [&](int h, int it, int slot) __attribute__((always_inline)) {
        const int m = m0 + h * PR + rl0 + it * RSTEP;
        if (!(m < p.M && nok)) return;
        const f32x4 a = *reinterpret_cast<const f32x4*>(read_base + it * RSTEP * SROW);
        const f32x4 b = *reinterpret_cast<const f32x4*>(read_base + it * RSTEP * SROW + 16);
        if constexpr ((FLAGS & EF_F32) != 0) {
            union { f32x4 f; u32x4 r; } ua, ub;
            ua.f = a; ub.f = b;
            const uint32_t off = (uint32_t)m * ldcb + (uint32_t)n * 4u;
            // PLAIN stores: the fp32 gradients are read again within the step (norm remainder, AdamW) and a write-through store drops the
            // line from the XCD's L2 -- measured 7.92 (plain) against 8.04 ms (sc1) per step, profiles/r06g_norm_shares_ab.txt
            __builtin_amdgcn_raw_buffer_store_b128(ua.r, rc, off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(ub.r, rc, off + 16u, 0, 0);
            sq += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]) + (b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3]);
            return;
        }
        f32x2 v[4] = {f32x2{a[0], a[1]}, f32x2{a[2], a[3]}, f32x2{b[0], b[1]}, f32x2{b[2], b[3]}};
        if constexpr ((FLAGS & EF_RBWD) != 0) {
            f32x2 t[4];
            if constexpr (HAS_RES) {
                unpack_bf16x8(res[slot], t);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] + t[r];
            }
            unpack_bf16x8(aux[slot], t);
            f32x2 u[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = f32x2{t[r][0] > 0.f ? v[r][0] : 0.f, t[r][1] > 0.f ? v[r][1] : 0.f};
                u[r] = (FLAGS & EF_PS2) != 0 ? v[r] * sh[r] : v[r];
                v[r] = v[r] * sc[r];
            }
            __builtin_amdgcn_raw_buffer_store_b128(pack_bf16x8(u), rc2, (uint32_t)m * ldc2b + nb, 0, 16 /* sc1 */);
            __builtin_amdgcn_raw_buffer_store_b128(pack_bf16x8(v), rc, (uint32_t)m * ldcb + nb, 0, 16 /* sc1 */);
            return;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {                              // (scale and shift together: one fma, as in every path of the library)
            if constexpr ((FLAGS & EF_SCALE) != 0 && (FLAGS & EF_SHIFT) != 0) v[r] = pk_fma(v[r], sc[r], sh[r]);
            else if constexpr ((FLAGS & EF_SCALE) != 0) v[r] = v[r] * sc[r];
            else if constexpr ((FLAGS & EF_SHIFT) != 0) v[r] = v[r] + sh[r];
        }
        if constexpr ((FLAGS & EF_GELU2) != 0) {
            f32x2 dv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) gelu_erf_both2(v[r], v[r], dv[r]);
            __builtin_amdgcn_raw_buffer_store_b128(pack_bf16x8(dv), rc2, (uint32_t)m * ldc2b + nb, 0, 16 /* sc1 */);
        }
        if constexpr ((FLAGS & EF_GELU1) != 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { f32x2 dv; gelu_erf_both2(v[r], v[r], dv); }
        }
        if constexpr ((FLAGS & EF_RELU) != 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = f32x2{fmaxf(v[r][0], 0.f), fmaxf(v[r][1], 0.f)};
        }
        if constexpr ((FLAGS & EF_DROP) != 0) {
            const uint64_t grp = (uint64_t)m * ((p.N + 3) >> 2) + (n >> 2);
            const f32x4 d0 = dropout_mult4(p.seed, grp, p.dropout_p), d1 = dropout_mult4(p.seed, grp + 1, p.dropout_p);
            v[0] = v[0] * f32x2{d0[0], d0[1]}; v[1] = v[1] * f32x2{d0[2], d0[3]};
            v[2] = v[2] * f32x2{d1[0], d1[1]}; v[3] = v[3] * f32x2{d1[2], d1[3]};
        }
        if constexpr (HAS_RES) {
            f32x2 t[4];
            unpack_bf16x8(res[slot], t);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = v[r] + t[r];
        }
        if constexpr ((FLAGS & EF_RELU_AFTER) != 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = f32x2{fmaxf(v[r][0], 0.f), fmaxf(v[r][1], 0.f)};
        }
        if constexpr (HAS_AUX) {
            f32x2 t[4];
            unpack_bf16x8(aux[slot], t);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr ((FLAGS & EF_MASK) != 0) v[r] = f32x2{t[r][0] > 0.f ? v[r][0] : 0.f, t[r][1] > 0.f ? v[r][1] : 0.f};
                else v[r] = v[r] * t[r];
            }
        }
        __builtin_amdgcn_raw_buffer_store_b128(pack_bf16x8(v), rc, out_row(m) * ldcb + nb, 0, 16 /* sc1 */);
    };
    auto pass = [&](int h) __attribute__((always_inline)) {
        if constexpr ((HAS_RES || HAS_AUX) && !ALL) request(h);
        __syncthreads();
        stage(h);
        __syncthreads();
        if constexpr ((FLAGS & (EF_GELU2 | EF_GELU1)) != 0) {
#pragma unroll 1
            for (int it = 0; it < ITER; ++it) chunk(h, it, 0);
        } else {
#pragma unroll
            for (int it = 0; it < ITER; ++it) chunk(h, it, (ALL ? h * ITER : 0) + it);
        }
    };
    if constexpr ((HAS_RES || HAS_AUX) && ALL) {
#pragma unroll
        for (int h = 0; h < NPASS; ++h) request(h);
    }
    if constexpr (ROLL && !((HAS_RES || HAS_AUX) && ALL)) {
#pragma unroll 1
        for (int h = 0; h < NPASS; ++h) pass(h);
    } else {
#pragma unroll
        for (int h = 0; h < NPASS; ++h) pass(h);
    }
    if constexpr ((FLAGS & EF_F32) != 0) {
        if (p.sq_slots) {                                        // (block-uniform) waves added in wave order: a fixed order
            sq = wave_sum(sq);
            __syncthreads();                                     // the staging area is free again
            float* red = reinterpret_cast<float*>(smem);
            if ((tid & 63) == 0) red[tid >> 6] = sq;
            __syncthreads();
            if (tid == 0) {
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < NT / 64; ++w) t += red[w];
                p.sq_slots[tile_lin] = t;
            }
        }
    }
}

// runtime index -> compile-time combination (a wave-uniform switch: the kernel argument lives in SGPRs)
// WG: a weight-gradient kernel (both operands reduction-major): the only combination it ever meets is the stored fp32 C; the other forms
// never meet that one -- neither instantiates what it cannot run.
// FORM: what the kernel's loaders say about the product -- 0 unknown, 1 forward (B k-contiguous), 2 data gradient (B reduction-major).
// fe_in_form: a kernel instantiates only the combinations its form meets in the model (forward: plain, bias, GELU + derivative, bias
// (+ dropout) + residual, the FrozenBN forms; data gradient: plain, x stored derivative, + residual, x scale under a mask, the fused
// ReLU x FrozenBN backward); a call with another combination takes the generic epilogue.  Eight bodies per kernel instead of fifteen:
// 7.718 -> 7.701 ms per step, three alternating pairs (profiles/r06w_epilogue_bodies_per_form.txt) -- and see gemm8_impl.h
// tile_epilogue8w for what ALL of them did to the 256x256 instantiation.
__host__ __device__ constexpr bool fe_in_form(int idx, int form) {
    if (form == 1) return idx == 1 || idx == 2 || idx == 3 || idx == 4 || idx == 5 || idx == 8 || idx == 9 || idx == 10 || idx == 17 || idx == 18;
    if (form == 2) return idx == 1 || idx == 6 || idx == 7 || (idx >= 11 && idx <= 15) || idx == 19 || idx == 20;
    return true;
}
// the row-map bodies (EF_RMAP, EF_CMAP) exist in the 4-wave kernels only (NT == NTHREADS): the 8-wave kernels never meet them (gemm_choose)
__host__ __device__ constexpr bool fe_for_threads(int idx, int nt) { return (FAST_EPI_COMBOS[idx] & (EF_RMAP | EF_CMAP)) == 0 || nt == NTHREADS; }
template <int NT, int BN, int PR, int NPASS, bool WG = false, int FORM = 0, typename StageFn>
__device__ __forceinline__ void fast_epilogue_dispatch(const GP& p, unsigned char* smem, int m0, int n0, int tid, StageFn stage,
                                                       const bf16x8* pre_r = nullptr, const bf16x8* pre_a = nullptr, int tile_lin = 0) {
    if constexpr (WG) {
        fast_epilogue<EF_F32, NT, BN, PR, NPASS>(p, smem, m0, n0, tid, stage, nullptr, nullptr, tile_lin);
        return;
    }
    switch (p.fast_epi) {
#define CB_FE_CASE(I) case I: if constexpr (fe_in_form(I, FORM) && fe_for_threads(I, NT)) fast_epilogue<FAST_EPI_COMBOS[I], NT, BN, PR, NPASS>(p, smem, m0, n0, tid, stage, pre_r, pre_a); break;
        CB_FE_CASE(1) CB_FE_CASE(2) CB_FE_CASE(3) CB_FE_CASE(4) CB_FE_CASE(5) CB_FE_CASE(6) CB_FE_CASE(7) CB_FE_CASE(8) CB_FE_CASE(9) CB_FE_CASE(10)
        CB_FE_CASE(11) CB_FE_CASE(12) CB_FE_CASE(13) CB_FE_CASE(14) CB_FE_CASE(15) CB_FE_CASE(17) CB_FE_CASE(18) CB_FE_CASE(19) CB_FE_CASE(20)
#undef CB_FE_CASE
        default: break;
    }
}
static_assert(FAST_EPI_N == 21 && FAST_EPI_COMBOS[FAST_EPI_F32] == EF_F32, "fast_epilogue_dispatch lists every combination");

// ---------------------------------------------------------------------------------------------
// Epilogue-operand prefetch (row-contiguous bf16 epilogue only).  The epilogue's global READS -- the residual and the ReLU mask
// / GELU pre-activation -- do not depend on the product, so the thread's chunks are requested before the K loop and land while it
// runs: for the short-K 1x1 convolutions of the ResNet (1-4 K tiles, HBM-bound) the block otherwise waits a full HBM round trip
// between its last MFMA and its stores.  Same (row, chunk) map as tile_epilogue's c_vec8 branch.  NCH chunks x 2 operands x 4 VGPR.
// ---------------------------------------------------------------------------------------------
// WITH_R = false: only the second operand (mask / GELU pre-activation) is prefetched -- the 128x128 two-blocks-per-CU tile has 32
// registers to spare, not 64.
template <int BM, int BN, bool WITH_R = true>
struct EpiPre {
    static constexpr int WM = BM / 2, CPR = BN / 8, ITER = WM * CPR / NTHREADS, NCH = 2 * ITER;
    static constexpr bool HAS_R = WITH_R;
    bf16x8 r[WITH_R ? NCH : 1], a[NCH];
};

template <typename T, int BM, int BN, bool WITH_R>
__device__ __forceinline__ void epi_prefetch(const GP& p, EpiPre<BM, BN, WITH_R>& pre, int m0, int n0, int tid) {
    using E = EpiPre<BM, BN, WITH_R>;
    const int cc = tid % E::CPR, n = n0 + cc * 8;
    const void* aux = p.mask ? p.mask : p.dact_pre;
    const int64_t lda = p.mask ? p.ldm : p.ldd;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int it = 0; it < E::ITER; ++it) {
            const int m = m0 + h * E::WM + (tid + it * NTHREADS) / E::CPR;
            bf16x8 z = {};
            if constexpr (WITH_R) pre.r[h * E::ITER + it] = z;
            pre.a[h * E::ITER + it] = z;
            if (m < p.M && n < p.N) {
                const int64_t orow = p.c_rowmap ? (int64_t)p.c_rowmap[m] : (int64_t)m;
                if constexpr (WITH_R) {
                    const int64_t rrow = p.res_rowmap ? (int64_t)p.res_rowmap[m] : orow;          // (-1: the chunk stays zero)
                    if (p.residual && rrow >= 0) pre.r[h * E::ITER + it] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const T*>(p.residual) + rrow * p.ldr + n);
                }
                if (aux) pre.a[h * E::ITER + it] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const T*>(aux) + orow * lda + n);
            }
        }
}

// ---------------------------------------------------------------------------------------------
// Tile epilogue of the 4-wave kernels.  acc[i][j] = 4 consecutive n of row m (swapped MFMA operands).
// ---------------------------------------------------------------------------------------------
// One wave's FM x FN accumulator fragments -> the staging area in tile-row order: fragment (i, j) of lane l lies at row i * 16 + l % 16,
// columns col0 + j * 16 + 4 * (l / 16) .. + 3, rows ROWB bytes apart.  The caller places the barriers around it.
template <int ROWB, int FM, int FN>
__device__ __forceinline__ void stage_acc(unsigned char* smem, const f32x4 (&acc)[FM][FN], int lane, int col0) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
            *reinterpret_cast<f32x4*>(smem + (i * 16 + (lane & 15)) * ROWB + (col0 + j * 16 + 4 * (lane >> 4)) * 4) = acc[i][j];
}

template <typename T, int BM, int BN, int SMEM_BYTES, int EPF = 0, bool WG = false, int FORM = 0>
__device__ __forceinline__ void tile_epilogue(GP& p, f32x4 (&acc)[BM / 32][BN / 32], unsigned char* smem, int m0, int n0, int tid,
                                              const EpiPre<BM, BN, EPF != 1>& pre = EpiPre<BM, BN, EPF != 1>{}, bool use_pre = false, int tile_lin = 0) {
    constexpr int WM = BM / 2, WN = BN / 2, FM = WM / 16, FN = WN / 16;
    constexpr int SROW = BN * 4 + 16;                  // staged row: +16 B staggers consecutive rows across the banks
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    if (p.dropout_p > 0.f && p.seed_ptr) p.seed += *p.seed_ptr;
    const bool fast = p.c_vec && (n0 + BN <= p.N);      // block-uniform
    if constexpr (sizeof(T) == 2) {
        if (p.c_vec8 && p.fast_epi != 0 && (WG == (p.fast_epi == FAST_EPI_F32)) && fe_in_form(p.fast_epi, FORM)) {                    // specialised body for this call's option combination (block-uniform)
            static_assert((BM / 2) * SROW <= SMEM_BYTES, "staging does not fit");
            auto stage = [&](int h) __attribute__((always_inline)) { if (wm == h) stage_acc<SROW>(smem, acc, lane, wn * WN); };
            const bf16x8* pre_r = (EPF == 2 && use_pre) ? pre.r : nullptr;
            const bf16x8* pre_a = (EPF != 0 && use_pre) ? pre.a : nullptr;
            fast_epilogue_dispatch<NTHREADS, BN, BM / 2, 2, WG, FORM>(p, smem, m0, n0, tid, stage, pre_r, pre_a, tile_lin);
            return;
        }
    }
    if (p.c_vec8) {
        // Row-contiguous epilogue: the fp32 accumulators go through LDS (free after the main loop), half the tile
        // rows at a time, so that each thread then owns 8 consecutive columns of one row: residual / mask reads and
        // the stores are 16-byte lane accesses over whole cache lines (the MFMA register layout would touch 16
        // different lines per store instruction -- the dominant cost of the short-K convolutions).
        constexpr int CPR = BN / 8;                    // 8-column chunks per tile row
        constexpr int ITER = WM * CPR / NTHREADS;
        static_assert(WM * SROW <= SMEM_BYTES, "staging does not fit");
        static_assert(WM * CPR % NTHREADS == 0 && NTHREADS % CPR == 0, "chunk map");
        const int cc = tid % CPR, n = n0 + cc * 8;
        const bool nok = n < p.N;                      // N % 8 == 0 (host-checked): chunks are all-in or all-out
        float sc[8], sh[8];
        if (nok) load_scale_shift(p, n, sc, sh);
        // ROLLED pass / chunk loops (round 5): the generic body is ~10 KB of branchy code that a workgroup runs once per chunk; unrolled
        // (2 passes x ITER chunks) it executed out of instruction-cache misses, ~1.1 us per chunk (profiles/r05a_stamps.md).  One copy,
        // warm after the first trip.  The staged accumulator indices do not depend on the pass (a wave stages its whole block in ITS pass);
        // the prefetched epilogue operands (EPF) live in registers and are picked by a compile-time-indexed select chain.
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            __syncthreads();
            if (wm == h) stage_acc<SROW>(smem, acc, lane, wn * WN);
            __syncthreads();
#pragma unroll 1
            for (int it = 0; it < ITER; ++it) {
                const int rl = (tid + it * NTHREADS) / CPR;
                const int m = m0 + h * WM + rl;
                bf16x8 rp = {}, ap = {};
                if constexpr (EPF != 0) {
                    if (use_pre) {
#pragma unroll
                        for (int q = 0; q < 2 * ITER; ++q) {
                            if (q == h * ITER + it) {
                                if constexpr (EPF == 2) rp = pre.r[q];
                                ap = pre.a[q];
                            }
                        }
                    }
                }
                if (m < p.M && nok) {
                    const int64_t orow = p.c_rowmap ? (int64_t)p.c_rowmap[m] : (int64_t)m;
                    const int64_t rrow = p.res_rowmap ? (int64_t)p.res_rowmap[m] : orow;
                    float v[8];
                    load8(reinterpret_cast<const float*>(smem + rl * SROW + cc * 32), v);
                    if (EPF != 0 && use_pre) epilogue_cols<T, 8, EPF, true>(p, v, sc, sh, m, orow, n, rp, ap, rrow);
                    else epilogue_cols<T, 8, 0, true>(p, v, sc, sh, m, orow, n, bf16x8{}, bf16x8{}, rrow);
                }
            }
        }
    } else if (p.split_k > 1 && p.c_vec) {
        // split-K partial sums: fp32 atomics, issued so that a wave instruction covers 64 consecutive floats of one
        // output row (whole cache lines per L2 atomic request instead of 16 rows x 16 B from the MFMA layout).
        static_assert(WM * SROW <= SMEM_BYTES, "staging does not fit");
        float* cbase = reinterpret_cast<float*>(p.C);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            __syncthreads();
            if (wm == h) stage_acc<SROW>(smem, acc, lane, wn * WN);
            __syncthreads();
#pragma unroll 4
            for (int idx = tid; idx < WM * BN; idx += NTHREADS) {
                const int rl = idx / BN, cl = idx % BN;
                const int m = m0 + h * WM + rl, n = n0 + cl;
                if (m < p.M && n < p.N) {
                    const int64_t orow = p.c_rowmap ? (int64_t)p.c_rowmap[m] : (int64_t)m;
                    float x = *reinterpret_cast<const float*>(smem + rl * SROW + cl * 4) * p.alpha;
                    if (p.scale) x *= p.scale[n];
                    atomicAdd(cbase + orow * p.ldc + n, x);
                }
            }
        }
    } else if (fast) {
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const int m = m0 + wm * WM + i * 16 + (lane & 15);
            const bool mok = m < p.M;
            const int64_t orow = (mok && p.c_rowmap) ? (int64_t)p.c_rowmap[m] : (int64_t)m;
            const int64_t rrow = (mok && p.res_rowmap) ? (int64_t)p.res_rowmap[m] : orow;
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                const int nb = n0 + wn * WN + j * 16 + 4 * (lane >> 4);
                if (mok) {
                    float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]}, sc[4], sh[4];
                    load_scale_shift(p, nb, sc, sh);
                    epilogue_cols<T, 4, 0, true>(p, v, sc, sh, m, orow, nb, bf16x8{}, bf16x8{}, rrow);
                }
            }
        }
    } else {
        // ragged N edge or unaligned output: stage the accumulators through LDS (free after the main
        // loop), half the tile rows at a time, then run a plain bounds-checked per-element loop.
        const float* stage = reinterpret_cast<const float*>(smem);
        static_assert(WM * BN * 4 <= SMEM_BYTES, "staging does not fit");
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            __syncthreads();
            if (wm == h) stage_acc<BN * 4>(smem, acc, lane, wn * WN);
            __syncthreads();
            for (int idx = tid; idx < WM * BN; idx += NTHREADS) {
                const int rl = idx / BN, cl = idx % BN;
                const int m = m0 + h * WM + rl, n = n0 + cl;
                if (m < p.M && n < p.N) {
                    const int64_t orow = p.c_rowmap ? (int64_t)p.c_rowmap[m] : (int64_t)m;
                    float v[1] = {stage[idx]}, sc[1], sh[1];
                    load_scale_shift(p, n, sc, sh);
                    epilogue_cols<T, 1, 0, true>(p, v, sc, sh, m, orow, n, bf16x8{}, bf16x8{}, p.res_rowmap ? (int64_t)p.res_rowmap[m] : orow);
                }
            }
        }
    }
}

}  // namespace cbgemm
