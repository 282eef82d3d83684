// GEMM / implicit-GEMM convolution family for gfx950 (MI355X): forward (NT), data-gradient (NN) and
// weight-gradient (TN) forms of Linear and NHWC convolution share one MFMA core.
//
//   C[m,n] (op)= epilogue( sum_k A(m,k) * B(n,k) )           (optionally `batch` problems per launch)
//
// Layout of the sources: gemm_impl.h holds the kernel templates, gemm_inst_*.hip instantiate one tile size each (so the
// tile sizes compile in parallel).  A call goes through three host steps with plain data between them: validate (gemm_prepare, here:
// descriptor -> Prepared), choose (gemm_choose.h: Prepared -> LaunchPlan) and launch (gemm_launch, here); cb_gemm, cb_gemm_plan,
// cb_gemm_workspace_bytes and cb_gemm_group compose them.
//
// * 256 threads = 4 waves (2x2); block tile 128x128 (one block per CU with a 2-stage register ring, or two blocks per CU with
//   one stage and <= 256 registers) / 128x64 / 64x64, K step 64 (bf16) / 32 (fp32).  256-row tiles (256x128, 256x64: one block
//   per CU, ~450 registers) were built and measured in round 2: never the fastest on any shape of the benchmark steps; a 128x128 tile
//   with two register stages AND two blocks per CU (192-242 VGPR, four K tiles in flight per CU) measured equal to the one-stage one.
// * k-contiguous operands: LDS image [rows][128 B], 16-byte segments XOR-swizzled with (row & 7): every ds_read_b128 of an
//   MFMA fragment is conflict-free.  Reduction-major operands (weights in dgrad, both operands in wgrad) keep their
//   natural [k][rows] image in LDS and are read with ds_read_b64_tr_b16 -- no transposed copy anywhere.
// * The addressing mode of each operand is a template parameter (RowkFast / KrowTr / KrowFast; generic guarded loaders
//   for unaligned shapes); loads are buffer-descriptor loads whose range check does all the predication.
// * PF-stage register ring global -> VGPR -> LDS (double-buffered), branch-free steady-state K loop.
// * Convolution operands are gathered through a per-output-pixel table (cb_build_pixel_table): no integer divisions.
// * MFMA operands are swapped (acc = mfma(Bfrag, Afrag)); the epilogue stages the accumulators through LDS so that each
//   thread owns 8 consecutive columns of a row: all epilogue reads and the stores are 16-byte, line-contiguous.
// * Weight gradients: split-K with row-coalesced fp32 atomics, XCD-aware block order, bias gradients as MFMA row sums.
// * bf16: v_mfma_f32_16x16x32_bf16; fp32 parity mode: v_mfma_f32_16x16x4_f32 (exact fp32).
// * Measured bound: L2 -> LDS bandwidth of the tile (profiles/r01_gemm_l2_analysis.md).

#include "gemm8_impl.h"
#include "gemm_stream_impl.h"
#include <stdio.h>
#include <vector>

using namespace cbgemm;

// tile instantiations live in gemm_inst_*.hip
namespace cbgemm {
extern template int launch_gemm<float, 64, 64, 2>(const GP&, bool, hipStream_t);
extern template int launch_gemm<bf16, 128, 128, 2>(const GP&, bool, hipStream_t);
extern template int launch_gemm<bf16, 128, 64, 2>(const GP&, bool, hipStream_t);
extern template int launch_gemm<bf16, 64, 64, 3>(const GP&, bool, hipStream_t);
extern template int launch_gemm<bf16, 128, 128, 1, 2>(const GP&, bool, hipStream_t);
extern template int launch_gemm_group<float, 64, 64, 2, 1>(const GroupArgs&, int, hipStream_t);
extern template int launch_gemm_group<bf16, 64, 64, 3, 1>(const GroupArgs&, int, hipStream_t);
extern template int launch_gemm_group<bf16, 128, 128, 1, 2>(const GroupArgs&, int, hipStream_t);
// 8-wave LDS-DMA structure (gemm8_impl.h), instantiated in gemm8_inst_*.hip
#define CB_G8_DECL(BM, BN, WGM, WGN, NST)                                                             \
    extern template int launch_gemm8_fwd<BM, BN, WGM, WGN, NST>(const GP&, int, float*, hipStream_t);   \
    extern template int launch_gemm8_dgrad<BM, BN, WGM, WGN, NST>(const GP&, int, float*, hipStream_t); \
    extern template int launch_gemm8_wgrad<BM, BN, WGM, WGN, NST>(const GP&, int, float*, hipStream_t);
CB_G8_DECL(256, 256, 2, 4, 2)
CB_G8_DECL(128, 256, 2, 4, 3)
CB_G8_DECL(256, 128, 4, 2, 3)
#undef CB_G8_DECL
// few rows (tile 9, gemm_skinny.hip)
int launch_gemm_skinny(const cb_gemm_desc* d, GP& p, hipStream_t st);
}

// switches, Form / Prepared, the launch-cost model and gemm_choose (validated call -> LaunchPlan)
#include "gemm_choose.h"

// ---- diagnostic build (-DCB_STAMPS, clipbert_amd/lib/libclipbert_hip_stamps.so; tools/stamps_run.py): every stamped launch gets a
// record area in a caller-provided device buffer and a host-side description ----------------------------------------------------
#ifdef CB_STAMPS
#include <string>
namespace {
struct StampState {
    unsigned long long* buf = nullptr;
    int64_t areas = 0;
    std::vector<std::string> desc;
} g_stamps;
void stamp_assign(GP& p, const cb_gemm_desc* d, int tile, int split, int sched, int group_i, int group_n) {
    p.stamps = nullptr;
    if (!g_stamps.buf || (int64_t)g_stamps.desc.size() >= g_stamps.areas) return;
    p.stamps = g_stamps.buf + (int64_t)g_stamps.desc.size() * cbgemm::CB_STAMP_AREA;
    char line[512];
    snprintf(line, sizeof line,
             "{\"M\":%d,\"N\":%d,\"K\":%d,\"a_mode\":%d,\"b_mode\":%d,\"batch\":%d,\"tile\":%d,\"split\":%d,\"sched\":%d,\"taps\":%d,"
             "\"act\":%d,\"c2\":%d,\"residual\":%d,\"dropout\":%d,\"mask\":%d,\"gelu_grad\":%d,\"relu_bwd\":%d,\"c_f32\":%d,\"group_i\":%d,\"group_n\":%d}",
             d->M, d->N, d->K, d->a_mode, d->b_mode, d->batch > 1 ? d->batch : 1, tile, split, sched, (d->R > 0 ? d->R : 1) * (d->S > 0 ? d->S : 1), d->act,
             d->C2 != nullptr, d->residual != nullptr, d->dropout_p > 0.f, d->mask != nullptr, d->gelu_grad_pre != nullptr, d->relu_bwd != 0, d->c_f32, group_i, group_n);
    g_stamps.desc.push_back(line);
}
}  // namespace
// buf: device memory of `bytes` bytes, zero-filled by the caller except word 0 of every area (min start) = ~0; resets the launch list
extern "C" int cb_debug_stamps_begin(void* buf, int64_t bytes) {
    g_stamps.buf = reinterpret_cast<unsigned long long*>(buf);
    g_stamps.areas = buf ? bytes / (8 * (int64_t)cbgemm::CB_STAMP_AREA) : 0;
    g_stamps.desc.clear();
    return 0;
}
extern "C" int64_t cb_debug_stamps_area_words() { return cbgemm::CB_STAMP_AREA; }
extern "C" int64_t cb_debug_stamps_count() { return (int64_t)g_stamps.desc.size(); }
extern "C" int cb_debug_stamps_desc(int64_t i, char* out, int64_t cap) {
    if (i < 0 || i >= (int64_t)g_stamps.desc.size() || cap <= 0) return -1;
    snprintf(out, (size_t)cap, "%s", g_stamps.desc[(size_t)i].c_str());
    return 0;
}
#define CB_STAMP_ASSIGN(p, d, tile, split, sched, gi, gn) stamp_assign(p, d, tile, split, sched, gi, gn)
#else
#define CB_STAMP_ASSIGN(p, d, tile, split, sched, gi, gn) do {} while (0)
#endif

namespace {

__global__ void __launch_bounds__(256) pixel_table_kernel(cb_pixel* tab, int total, int OH, int OW, int stride,
                                                          int pad, int64_t sN, int64_t sH, int64_t sW) {
    int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= total) return;
    int ow = m % OW, t = m / OW;
    int oh = t % OH, n = t / OH;
    int ih0 = oh * stride - pad, iw0 = ow * stride - pad;
    cb_pixel px;
    px.off = (int32_t)((int64_t)n * sN + (int64_t)ih0 * sH + (int64_t)iw0 * sW);
    px.ih0 = (int16_t)ih0;
    px.iw0 = (int16_t)iw0;
    tab[m] = px;
}

// K-split partial products -> result: sums the S slabs of the workspace in index order (deterministic) and applies the epilogue.
__global__ void __launch_bounds__(256) splitk_reduce_kernel(GP p, const float* ws, int S) {
    using T = bf16;
    const int cpr = p.N >> 3;
    const int64_t total = (int64_t)p.M * cpr;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p.batch > 1) {
        const int b = blockIdx.y;
        p.C = reinterpret_cast<unsigned char*>(p.C) + b * p.bs_c;
        ws += (int64_t)b * S * p.M * p.N;
    }
    if (idx >= total) return;
    if (p.dropout_p > 0.f && p.seed_ptr) p.seed += *p.seed_ptr;
    const int m = (int)(idx / cpr), n = (int)(idx - (int64_t)m * cpr) * 8;
    float v[8], t[8], sc[8], sh[8];
    const float* src = ws + (int64_t)m * p.N + n;
    load8(src, v);
    for (int s = 1; s < S; ++s) {
        load8(src + (int64_t)s * p.M * p.N, t);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] += t[r];
    }
    if (p.scale) load8(p.scale + n, sc);
    if (p.shift) load8(p.shift + n, sh);
    const int64_t orow = p.c_rowmap ? (int64_t)p.c_rowmap[m] : (int64_t)m;
    epilogue_cols<T, 8>(p, v, sc, sh, m, orow, n);
}

template <int BM, int BN, int WGM, int WGN, int NST>
int launch8(int form, const GP& p, int mode, float* ws, hipStream_t st) {
    if (form == 1) return launch_gemm8_fwd<BM, BN, WGM, WGN, NST>(p, mode, ws, st);
    if (form == 2) return launch_gemm8_dgrad<BM, BN, WGM, WGN, NST>(p, mode, ws, st);
    return launch_gemm8_wgrad<BM, BN, WGM, WGN, NST>(p, mode, ws, st);
}

// ---- validate: a descriptor is checked and translated into the kernels' parameter block (Prepared, gemm_choose.h)
int gemm_prepare(const cb_gemm_desc* d, Prepared& out) {
    CB_REQUIRE(d != nullptr, "cb_gemm: null descriptor");
    CB_REQUIRE(d->dtype == CB_F32 || d->dtype == CB_BF16, "cb_gemm: bad dtype %d", d->dtype);
    CB_REQUIRE(d->M >= 0 && d->N >= 0 && d->K >= 0, "cb_gemm: negative dims");
    CB_REQUIRE(d->A && d->B && d->C, "cb_gemm: null operand");
    const int esz = d->dtype == CB_BF16 ? 2 : 4;
    const int eps = 16 / esz;
    GP& p = out.p;
    p = GP{};
    p.A = d->A; p.B = d->B; p.C = d->C; p.C2 = d->C2; p.residual = d->residual; p.mask = d->mask;
    p.dact_pre = d->gelu_grad_pre; p.ldd = d->ld_gelu; p.a_rowsum = d->a_rowsum;
    p.relu_bwd = d->relu_bwd != 0; p.post_scale = d->post_scale; p.post_scale2 = d->post_scale2;
    if (p.relu_bwd) {
        CB_REQUIRE(d->mask && (!d->c_f32 || d->dtype == CB_F32) && !d->scale && !d->shift && d->act == CB_ACT_NONE && d->dropout_p <= 0.f && !d->relu_after &&
                   !d->gelu_grad_pre && (d->split_k <= 1),
                   "cb_gemm: relu_bwd needs a mask and excludes scale/shift/act/dropout/relu_after/gelu_grad_pre/split_k and an fp32 C next to bf16 operands");
        CB_REQUIRE((!d->post_scale || aligned16(d->post_scale)) && (!d->post_scale2 || aligned16(d->post_scale2)),
                   "cb_gemm: post_scale vectors must be 16-byte aligned");
    } else {
        CB_REQUIRE(!d->post_scale && !d->post_scale2, "cb_gemm: post_scale / post_scale2 need relu_bwd");
    }
    // (no caller combines them, and the epilogue widths once disagreed on what the pair means: epilogue_cols applies one OR the other)
    CB_REQUIRE(!(d->mask && d->gelu_grad_pre), "cb_gemm: mask and gelu_grad_pre exclude each other");
    p.batch = d->batch > 1 ? d->batch : 1;
    p.bs_a = d->batch_stride_a * esz; p.bs_b = d->batch_stride_b * esz;
    p.bs_c = d->batch_stride_c * (d->c_f32 ? 4 : esz); p.bs_r = d->batch_stride_rowsum;
    if (p.batch > 1) {
        CB_REQUIRE(!d->C2 && !d->residual && !d->mask && !d->gelu_grad_pre && !d->a_tab && !d->b_tab && !d->c_rowmap,
                   "cb_gemm: batch > 1 supports plain operands only (no residual / mask / second output / gather / row map)");
        CB_REQUIRE((d->batch_stride_a * esz) % 16 == 0 && (d->batch_stride_b * esz) % 16 == 0 && (p.bs_c % 16) == 0,
                   "cb_gemm: batch strides must keep 16-byte alignment");
    }
    CB_REQUIRE(!d->a_rowsum || (d->a_mode == CB_KROW && d->b_mode == CB_KROW), "cb_gemm: a_rowsum needs the weight-gradient form (A and B both CB_KROW)");
    p.scale = d->scale; p.shift = d->shift; p.a_tab = d->a_tab; p.b_tab = d->b_tab; p.c_rowmap = d->c_rowmap; p.zfill = d->zero_fill_pitch;
    p.lda = d->lda; p.ldb = d->ldb; p.ldc = d->ldc; p.ldc2 = d->ldc2; p.ldr = d->ldr; p.ldm = d->ldm;
    p.sH = d->sH; p.sW = d->sW;
    p.M = d->M; p.N = d->N; p.K = d->K;
    p.a_mode = d->a_mode; p.b_mode = d->b_mode;
    p.R = d->R > 0 ? d->R : 1; p.S = d->S > 0 ? d->S : 1; p.Ct = d->Cin; p.H = d->H; p.W = d->W; p.flip = d->flip_taps;
    p.res_rowmap = d->res_rowmap;
    if (d->res_rowmap) {
        CB_REQUIRE(d->residual && d->res_rows > 0 && p.batch == 1 && (int64_t)d->res_rows * d->ldr * esz < 0x7fffffffll,
                   "cb_gemm: res_rowmap needs a residual of res_rows > 0 rows that ends below 2 GiB, and one problem per launch");
    }
    if (d->dgrad_s2) {
        CB_REQUIRE(d->a_mode == CB_ROWK_GATHER && d->b_mode == CB_KROW_TAPS && d->R == 3 && d->S == 3 && d->M % 4 == 0 && d->c_rowmap &&
                   d->ldb == (int64_t)9 * d->N && p.batch == 1 && d->split_k <= 1 && !d->zero_fill_pitch,
                   "cb_gemm: dgrad_s2 needs A CB_ROWK_GATHER, B CB_KROW_TAPS with R = S = 3 and ldb = 9 N, M a multiple of 4, c_rowmap, no batch / K split / zero fill");
        p.cls_rows = d->M / 4;
        p.flip = 0;                                   // (each workgroup sets its class's tap base: dgrad_s2_class)
    }
    CB_REQUIRE(d->accumulate >= 0 && d->accumulate <= 2 && (d->accumulate != 2 || d->dtype == CB_BF16), "cb_gemm: bad accumulate %d (2 = first writer: bf16 problems)", d->accumulate);
    p.c_f32 = d->c_f32; p.accumulate = d->accumulate == 1; p.split_k = d->split_k > 0 ? d->split_k : 1;
    p.act = d->act; p.relu_after = d->relu_after;
    p.alpha = d->alpha == 0.f ? 1.f : d->alpha;
    p.dropout_p = d->dropout_p; p.seed = d->dropout_seed; p.seed_ptr = d->dropout_seed_ptr;
    const int bk = d->dtype == CB_BF16 ? Tr<bf16>::BK : Tr<float>::BK;
    p.ktiles = (d->K + bk - 1) / bk;
    {   // write-through (sc1) bf16 epilogue stores (round 5, profiles/r05b_bench_ab_wt.txt: -0.10 ... -0.14 ms per step, four alternating runs):
        // the output leaves for the memory side while the other workgroups still compute, instead of sitting dirty in the XCD's L2 until
        // the end-of-kernel release writes it back in one burst.  CB_GEMM_WT=0 restores plain stores; =3 adds nt on the second output.
        const bool ok = d->dtype == CB_BF16 && !d->c_f32 && (int64_t)d->M * (d->ldc > d->ldc2 ? d->ldc : d->ldc2) * 2 * (p.batch) < 0xffffffffll &&
                        (!d->c_rowmap || d->dgrad_s2);        // (dgrad_s2's row map is a permutation of the M output rows: the same extent)
        p.wt = ok ? switches().wt : 0;
    }
    {   // specialised epilogue (FAST_EPI_COMBOS in gemm_impl.h): the call's option combination, if it is one of the listed ones and the
        // row-contiguous bf16 write-through epilogue applies; CB_GEMM_FAST_EPI=0: the generic epilogue (epilogue_cols) for everything
        const bool fe_off = switches().fast_epi_off;
        p.fast_epi = 0;
        auto rows_ok = [&](const void* q, int64_t ld) { return q == nullptr || (ld % 8 == 0 && aligned16(q) && (int64_t)d->M * ld * 2 < 0x7fffffffll); };
        // weight-gradient forms that STORE an fp32 C (first writer): the lean fp32 epilogue, which also leaves the tile's share of the squared norm
        const bool wg_store = !fe_off && d->dtype == CB_BF16 && d->c_f32 && d->a_mode == CB_KROW && d->accumulate != 1 && p.alpha == 1.f && !d->scale && !d->shift &&
                              d->act == CB_ACT_NONE && !d->C2 && !d->residual && !d->mask && !d->gelu_grad_pre && d->dropout_p <= 0.f && !d->relu_after && !d->c_rowmap &&
                              !d->zero_fill_pitch && !d->relu_bwd && d->N % 8 == 0 && d->ldc % 8 == 0 && aligned16(d->C) && (int64_t)d->M * d->ldc * 4 < 0xffffffffll;
        if (wg_store) p.fast_epi = FAST_EPI_F32;
        p.sq_slots = nullptr;
        if (d->sq_slots) {
            const int64_t need = (int64_t)((d->M + 63) / 64) * ((d->N + 63) / 64) * p.batch;
            CB_REQUIRE(wg_store, "cb_gemm: sq_slots needs a bf16 weight-gradient form storing an aligned fp32 C with a plain epilogue (accumulate 0 / 2)");
            CB_REQUIRE(d->sq_slots_n >= need, "cb_gemm: sq_slots_n %lld < %lld (one slot per 64x64 tile and batch member)", (long long)d->sq_slots_n, (long long)need);
            p.sq_slots = d->sq_slots;
        }
        const bool plain = !wg_store && !fe_off && p.wt == 1 && p.batch == 1 && d->accumulate != 1 && p.alpha == 1.f && !d->zero_fill_pitch && !d->a_rowsum &&
                           d->N % 8 == 0 && d->ldc % 8 == 0 && aligned16(d->C) && (!d->shift || aligned16(d->shift)) && (!d->scale || aligned16(d->scale)) &&
                           (d->res_rowmap ? (d->ldr % 8 == 0 && aligned16(d->residual)) : rows_ok(d->residual, d->ldr)) && rows_ok(d->mask, d->ldm) && rows_ok(d->gelu_grad_pre, d->ld_gelu);
        if (plain && d->relu_bwd) {                                          // (validated above: mask, no scale / shift / act / dropout / relu_after)
            const bool ok = d->C2 && d->post_scale && d->ldc2 % 8 == 0 && aligned16(d->C2) && (int64_t)d->M * d->ldc2 * 2 < 0xffffffffll;
            const int flags = EF_RBWD | (d->residual ? EF_RES : 0) | (d->post_scale2 ? EF_PS2 : 0) | (d->res_rowmap ? EF_RMAP : 0) | (d->dgrad_s2 ? EF_CMAP : 0);
            if (ok)
                for (int i = 1; i < FAST_EPI_N; ++i)
                    if (FAST_EPI_COMBOS[i] == flags) { p.fast_epi = i; break; }
        } else if (plain) {
            int flags = 0;
            bool ok = true;
            if (d->scale) flags |= EF_SCALE;
            if (d->shift) flags |= EF_SHIFT;
            if (d->act == CB_ACT_RELU) flags |= EF_RELU;
            else if (d->act == CB_ACT_GELU_SAVE_GRAD && d->C2) flags |= EF_GELU2;
            else if (d->act == CB_ACT_GELU && !d->C2) flags |= EF_GELU1;
            else if (d->act == CB_ACT_SAVED_GRAD && d->gelu_grad_pre) flags |= EF_MULAUX;
            else if (d->act != CB_ACT_NONE) ok = false;
            if (d->C2 && !(flags & EF_GELU2)) ok = false;                    // (a second output only as the stored derivative)
            if (d->C2) ok = ok && d->ldc2 % 8 == 0 && aligned16(d->C2) && (int64_t)d->M * d->ldc2 * 2 < 0xffffffffll;
            if (d->gelu_grad_pre && !(flags & EF_MULAUX)) ok = false;        // (GELU' evaluated from the pre-activation: generic path)
            if (d->dropout_p > 0.f) flags |= EF_DROP;
            if (d->residual) flags |= EF_RES;
            if (d->res_rowmap) flags |= EF_RMAP;
            if (d->relu_after) flags |= EF_RELU_AFTER;
            if (d->mask) flags |= EF_MASK;
            if (d->dgrad_s2) flags |= EF_CMAP;
            if (ok)
                for (int i = 1; i < FAST_EPI_N; ++i)
                    if (FAST_EPI_COMBOS[i] == flags) { p.fast_epi = i; break; }
        }
    }
    const bool a_krow = d->a_mode == CB_KROW;
    const bool b_krow = d->b_mode == CB_KROW || d->b_mode == CB_KROW_TAPS || d->b_mode == CB_KROW_GATHER;
    CB_REQUIRE(d->a_mode == CB_ROWK || d->a_mode == CB_ROWK_GATHER || d->a_mode == CB_KROW, "cb_gemm: bad a_mode %d", d->a_mode);
    CB_REQUIRE(d->b_mode == CB_ROWK || b_krow, "cb_gemm: bad b_mode %d", d->b_mode);
    const int taps = p.R * p.S;
    const bool tapped = d->a_mode == CB_ROWK_GATHER || d->b_mode == CB_KROW_TAPS || d->b_mode == CB_KROW_GATHER;
    if (tapped) {
        CB_REQUIRE(p.Ct > 0, "cb_gemm: Cin (channels per tap) must be set for conv modes");
        CB_REQUIRE(p.Ct % eps == 0, "cb_gemm: channels per tap (%d) must be a multiple of %d", p.Ct, eps);
    }
    // fast path: 16-byte buffer loads -- every row/tap start 16-byte aligned and operands < 2 GiB
    const int64_t lim = 0x7fffffffll;
    bool fast = d->a_bytes > 0 && d->b_bytes > 0 && d->a_bytes < lim && d->b_bytes < lim && aligned16(d->A) && aligned16(d->B);
    if (d->a_mode == CB_ROWK_GATHER) {
        CB_REQUIRE(d->a_tab, "cb_gemm: a_tab missing");
        CB_REQUIRE(d->K == taps * p.Ct, "cb_gemm: K (%d) != R*S*Cin (%d)", d->K, taps * p.Ct);
        fast = fast && (p.R == 1 || d->sH % eps == 0) && (p.S == 1 || d->sW % eps == 0);
    } else if (d->a_mode == CB_ROWK) {
        fast = fast && (d->lda % eps == 0) && (d->K % eps == 0);
    } else {
        // a 16-byte load that is only partly inside the buffer returns zeros for ALL of it: the last (partial)
        // row block must still lie inside the buffer
        const int64_t need = ((int64_t)(d->K - 1) * d->lda + (d->M + eps - 1) / eps * eps) * esz;
        fast = fast && (d->lda % eps == 0) && (d->M % eps == 0 || need <= d->a_bytes);
    }
    if (d->b_mode == CB_ROWK) {
        fast = fast && (d->ldb % eps == 0) && (d->K % eps == 0);
    } else if (d->b_mode == CB_KROW) {
        const int64_t need = ((int64_t)(d->K - 1) * d->ldb + (d->N + eps - 1) / eps * eps) * esz;
        fast = fast && (d->ldb % eps == 0) && (d->N % eps == 0 || need <= d->b_bytes);
    } else if (d->b_mode == CB_KROW_TAPS) {
        CB_REQUIRE(d->K == taps * p.Ct, "cb_gemm: K (%d) != R*S*Ct (%d)", d->K, taps * p.Ct);
        fast = fast && (d->ldb % eps == 0) && (d->N % eps == 0);
    } else {
        CB_REQUIRE(d->b_tab, "cb_gemm: b_tab missing");
        CB_REQUIRE(d->N == taps * p.Ct, "cb_gemm: N (%d) != R*S*Cin (%d)", d->N, taps * p.Ct);
        fast = fast && (p.R == 1 || d->sH % eps == 0) && (p.S == 1 || d->sW % eps == 0);
    }
    p.a_bytes = (uint32_t)(fast ? d->a_bytes : 0);
    p.b_bytes = (uint32_t)(fast ? d->b_bytes : 0);
    CB_REQUIRE(d->tile >= 0 && d->tile <= 9, "cb_gemm: bad tile %d", d->tile);
    CB_REQUIRE(d->xcd_order >= 0 && d->xcd_order <= 2, "cb_gemm: bad xcd_order %d", d->xcd_order);
    CB_REQUIRE(d->dropout_p >= 0.f && d->dropout_p < 1.f, "cb_gemm: dropout_p out of range");
    // vector epilogue: every touched row pointer must be 16-byte (fp32) / 8-byte (bf16) aligned at n%4==0
    const int cesz = d->c_f32 ? 4 : esz;
    bool cv = (d->ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(d->C) % (4 * cesz)) == 0);
    if (d->C2) cv = cv && (d->ldc2 % 4 == 0) && ((reinterpret_cast<uintptr_t>(d->C2) % (4 * esz)) == 0);
    if (d->residual) cv = cv && (d->ldr % 4 == 0) && ((reinterpret_cast<uintptr_t>(d->residual) % (4 * esz)) == 0);
    if (d->mask) cv = cv && (d->ldm % 4 == 0) && ((reinterpret_cast<uintptr_t>(d->mask) % (4 * esz)) == 0);
    if (d->gelu_grad_pre) cv = cv && (d->ld_gelu % 4 == 0) && ((reinterpret_cast<uintptr_t>(d->gelu_grad_pre) % (4 * esz)) == 0);
    if (d->scale) cv = cv && aligned16(d->scale);
    if (d->shift) cv = cv && aligned16(d->shift);
    p.c_vec = cv;
    // row-contiguous epilogue: 8-wide chunks must be 16-byte aligned everywhere
    bool cv8 = cv && (d->N % 8 == 0) && (d->ldc % 8 == 0) && aligned16(d->C);
    if (d->C2) cv8 = cv8 && (d->ldc2 % 8 == 0) && aligned16(d->C2);
    if (d->residual) cv8 = cv8 && (d->ldr % 8 == 0) && aligned16(d->residual);
    if (d->mask) cv8 = cv8 && (d->ldm % 8 == 0) && aligned16(d->mask);
    if (d->gelu_grad_pre) cv8 = cv8 && (d->ld_gelu % 8 == 0) && aligned16(d->gelu_grad_pre);
    out.fast = fast; out.cv8 = cv8;
    out.form = operand_form(d->a_mode, d->b_mode, taps); out.taps = taps;
    out.epi_scale_only = !d->C2 && !d->residual && !d->mask && !d->gelu_grad_pre && d->act == CB_ACT_NONE && !d->relu_after && !d->shift && d->dropout_p <= 0.f;
    out.atomics_ok = out.epi_scale_only && d->c_f32 && d->accumulate == 1;
    return 0;
}

// The checks every entry point makes first, then gemm_prepare.  empty: M or N is zero -- nothing to compute, and the rest of the descriptor
// is not looked at.
int gemm_validate(const cb_gemm_desc* d, Prepared& pr, bool& empty) {
    empty = false;
    CB_REQUIRE(d != nullptr, "cb_gemm: null descriptor");
    CB_REQUIRE(d->M >= 0 && d->N >= 0 && d->K >= 0, "cb_gemm: negative dims");
    empty = d->M == 0 || d->N == 0;
    return empty ? 0 : gemm_prepare(d, pr);
}

void trace_plan(const cb_gemm_desc* d, const Prepared& pr, const LaunchPlan& lp) {
    if (lp.tile == 9)
        fprintf(stderr, "cb_gemm: M=%d N=%d K=%d modes=%d/%d tile=9 (asked %d) few rows\n", d->M, d->N, d->K, d->a_mode, d->b_mode, d->tile);
    else if (lp.tile == 8)
        fprintf(stderr, "cb_gemm: M=%d N=%d K=%d modes=%d/%d tile=8 (asked %d) stream variant %d\n", d->M, d->N, d->K, d->a_mode, d->b_mode, d->tile, lp.sched);
    else
        fprintf(stderr, "cb_gemm: M=%d N=%d K=%d modes=%d/%d tile=%d (asked %d) form8=%d split=%d ws=%d\n", d->M, d->N, d->K, d->a_mode, d->b_mode,
                lp.picked, d->tile, lp.form8, lp.tile >= 5 ? lp.split_k : pr.p.split_k, (int)lp.slab);
}

// ---- launch: the chosen configuration on the stream
int gemm_launch(const cb_gemm_desc* d, const Prepared& pr, const LaunchPlan& lp, hipStream_t st) {
    GP p = pr.p;
    if (lp.tile == 9) return launch_gemm_skinny(d, p, st);
    p.split_k = lp.split_k;
    p.c_vec8 = lp.c_vec8;
    p.xcd_remap = lp.xcd_remap;
    if (lp.tile == 8) return launch_gemm_stream(p, lp.sched, st);
    if (lp.tile >= 5) {
        float* ws = lp.slab ? reinterpret_cast<float*>(d->splitk_ws) : nullptr;
        CB_STAMP_ASSIGN(p, d, lp.tile, p.split_k, lp.sched, 0, 1);
        int rc;
        if (lp.tile == 5) rc = launch8<256, 256, 2, 4, 2>(lp.form8, p, lp.sched - 1, ws, st);
        else if (lp.tile == 6) rc = launch8<128, 256, 2, 4, 3>(lp.form8, p, lp.sched - 1, ws, st);
        else rc = launch8<256, 128, 4, 2, 3>(lp.form8, p, lp.sched - 1, ws, st);
        if (rc != 0 || !ws) return rc;
        GP q = p;
        q.split_k = 1;
        const int64_t chunks = (int64_t)d->M * (d->N / 8);
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((chunks + 255) / 256), (unsigned)p.batch), dim3(256), 0, st, q, ws, p.split_k);
        return cb_launch_status("cb_gemm (split-K reduce)");
    }
    if (d->dtype == CB_F32) return launch_gemm<float, 64, 64, 2>(p, pr.fast, st);
    CB_STAMP_ASSIGN(p, d, lp.tile, p.split_k, 0, 0, 1);
    if (lp.tile == 4) return launch_gemm<bf16, 128, 128, 1, 2>(p, pr.fast, st);
    if (lp.tile == 1) return launch_gemm<bf16, 128, 128, 2>(p, pr.fast, st);
    if (lp.tile == 3) return launch_gemm<bf16, 128, 64, 2>(p, pr.fast, st);
    return launch_gemm<bf16, 64, 64, 3>(p, pr.fast, st);
}

// cb_gemm for a validated problem (cb_gemm_group's single problems enter here with the Prepared they already have)
int gemm_run(const cb_gemm_desc* d, const Prepared& pr, void* stream) {
    LaunchPlan lp;
    const int rc = gemm_choose(d, pr, true, false, lp);
    if (lp.tile != 0 && switches().trace) trace_plan(d, pr, lp);
    return rc != 0 ? rc : gemm_launch(d, pr, lp, cb_stream(stream));
}
}  // namespace

extern "C" int cb_gemm(const cb_gemm_desc* d, void* stream) {
    Prepared pr;
    bool empty;
    if (int rc = gemm_validate(d, pr, empty)) return rc;
    return empty ? 0 : gemm_run(d, pr, stream);
}

// validate and choose as cb_gemm would, write {tile, split_k, schedule, xcd_order}, launch nothing
extern "C" int cb_gemm_plan(const cb_gemm_desc* d, int32_t use_table, int32_t* out4) {
    CB_REQUIRE(out4 != nullptr, "cb_gemm_plan: null output");
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    Prepared pr;
    LaunchPlan lp;
    bool empty;
    if (int rc = gemm_validate(d, pr, empty)) return rc;
    if (empty) return 0;
    if (int rc = gemm_choose(d, pr, use_table != 0, false, lp)) return rc;
    out4[0] = lp.tile; out4[1] = lp.split_k; out4[2] = lp.sched; out4[3] = lp.xcd_remap ? 1 : 2;
    return 0;
}

// K-split scratch cb_gemm would use for `d` if it were handed an unlimited one: what a caller sizes splitk_ws by.
extern "C" int cb_gemm_workspace_bytes(const cb_gemm_desc* d, int64_t* bytes) {
    CB_REQUIRE(d != nullptr && bytes != nullptr, "cb_gemm_workspace_bytes: null argument");
    *bytes = 0;
    Prepared pr;
    LaunchPlan lp;
    bool empty;
    if (int rc = gemm_validate(d, pr, empty)) return rc;
    if (empty) return 0;
    if (int rc = gemm_choose(d, pr, true, true, lp)) return rc;
    if (lp.slab) *bytes = (int64_t)lp.split_k * pr.p.batch * d->M * d->N * 4 + CB_SPLITK_WS_COUNTER_BYTES;
    return 0;
}

// ---- cb_gemm_group -------------------------------------------------------------------------------------------------------------
namespace {
// kernel class of a prepared problem for the grouped kernels, or -1: launched on its own
int group_class(const cb_gemm_desc* d, const Prepared& pr) {
    if (!pr.fast || d->zero_fill_pitch || d->tile >= 5 || d->tile == 1 || d->tile == 3 || d->res_rowmap || d->dgrad_s2) return -1;
    if (d->batch > 1 || d->a_rowsum) {
        // strided batches and bias row sums: the unsplit bf16 weight-gradient form on the 128x128 two-per-CU tile only (GC_WGRAD_RS: the
        // encoder's four kinds of 12-layer weight gradients share one grid -- their last waves of tiles fill each other's)
        const bool ok = d->dtype == CB_BF16 && pr.form == FORM_WGRAD && d->split_k <= 1 && d->tile != 2 && !d->c_rowmap;
        return ok ? GC_WGRAD_RS : -1;
    }
    return GROUP_CLASS_OF[pr.form];
}

struct GroupItem { const cb_gemm_desc* d; Prepared pr; int cls; };

// The K split of a grouped problem may be chosen freely where its parts can combine.  Unlike cb_gemm's rule (Prepared::atomics_ok) a first
// writer (accumulate == 2) counts here: a group's split problems may combine through the slab scratch, which needs no accumulated-into
// C; group_choose takes such a split back where that scratch cannot be used.
bool group_split_free(const GroupItem& it) { return a_reduction_major(it.pr.form) && it.d->c_f32 && it.d->accumulate != 0 && it.pr.epi_scale_only; }
inline int64_t group_tiles(const cb_gemm_desc* d, int B) { return (int64_t)((d->M + B - 1) / B) * ((d->N + B - 1) / B); }

// Launch configuration of one grouped launch (bf16): tile 2 (64x64) or 4 (128x128, two workgroups per CU) and a K split per problem.
// Cost model (calibrated on the in-step durations of profiles/r03z_train_step.md; tools/group_probe.py re-measures it): a CU retires
// the K tiles of its resident workgroups at a fixed aggregate rate once it holds enough of them -- 0.30 us per 64x64 K tile
// (~445 TF chip-wide), 0.77 us per 128x128 one (~700 TF) -- so a launch costs its fixed part plus (workgroups per CU) x (K tiles
// per workgroup) x that unit, plus the fp32 atomics of the split problems at ~2 TB/s.
double group_cost(const std::vector<GroupItem*>& g, int tile, int s, int* splits) {
    const int B = tile == 4 ? 128 : 64;
    int maxkt = 1;
    for (auto* it : g) maxkt = it->pr.p.ktiles > maxkt ? it->pr.p.ktiles : maxkt;
    const int kt_target = (maxkt + s - 1) / s;
    int64_t W = 0;
    int kt_per_max = 1;
    double atom = 0.0;
    for (size_t i = 0; i < g.size(); ++i) {
        const cb_gemm_desc* d = g[i]->d;
        const int kt = g[i]->pr.p.ktiles;
        int si = g[i]->pr.p.split_k;
        if (group_split_free(*g[i])) {
            si = (kt + kt_target / 2) / kt_target;
            if (si < 1) si = 1;
            while (si > 1 && kt / si < 4) --si;                    // (every split keeps at least four K tiles)
        }
        if (si > kt) si = kt > 0 ? kt : 1;
        splits[i] = si;
        W += group_tiles(d, B) * si;
        const int per = (kt + si - 1) / si;
        kt_per_max = per > kt_per_max ? per : kt_per_max;
        if (si > 1) atom += (double)d->M * d->N * 4.0 * si;
    }
    static const int cus = [] {                    // (the device's CU count; the unit costs below were fitted on an MI355X: 256)
        int dev = 0, n = 0;
        return (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }();
    const int64_t per_cu = (W + cus - 1) / cus;
    double unit;
    if (tile == 4) unit = per_cu <= 1 ? 1.0 : 0.77;
    else unit = per_cu <= 1 ? 0.45 : (per_cu == 2 ? 0.35 : 0.30);
    // workgroups beyond what a CU holds at once (2 / 4) queue behind the first round: their K loops do not overlap
    return 8.0 + (double)per_cu * kt_per_max * unit + atom / 2.0e6;
}

// ---- choose for one grouped launch: the tile, a K split per problem, and whether the split problems combine through the slab scratch
struct GroupPlan {
    int tile = 2;
    int splits[GROUP_MAX];
    float* slab = nullptr;    // the caller's K-split scratch where the slab K split runs, else null: fp32 atomics
    int* cnt = nullptr;       // ... and its arrival counters
};
void group_choose(const std::vector<GroupItem*>& g, int dtype, int cls, GroupPlan& gp) {
    int* splits = gp.splits;
    auto callers_splits = [&] { for (size_t i = 0; i < g.size(); ++i) splits[i] = g[i]->pr.p.split_k; };
    if (dtype == CB_F32) {
        callers_splits();
    } else {
        const int asked = g[0]->d->tile;
        if (cls == GC_WGRAD_RS) {                                    // (one tile, no K split: see group_class)
            gp.tile = 4;
            for (size_t i = 0; i < g.size(); ++i) splits[i] = 1;
        } else if (asked == 2 || asked == 4) {                       // explicit: the caller's tile and splits
            gp.tile = asked;
            callers_splits();
        } else {
            static const int SPLITS[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32};
            bool narrow = false, any_free = false;
            for (auto* it : g) { narrow = narrow || it->d->N <= 64; any_free = any_free || group_split_free(*it); }
            double best = 1e300;
            int tmp[GROUP_MAX];
            for (int t : {2, 4}) {
                if (t == 4 && narrow) continue;
                for (int s : SPLITS) {
                    if (s > 1 && !any_free) break;
                    const double c = group_cost(g, t, s, tmp);
                    if (c < best) { best = c; gp.tile = t; for (size_t i = 0; i < g.size(); ++i) splits[i] = tmp[i]; }
                }
            }
        }
    }
    // ---- slab K split (bf16 weight gradients; gemm_tile): the split problems' partial tiles go to the caller's K-split scratch and the last
    // part of a tile to arrive adds them in part order -- no fp32 atomics, a bit-reproducible sum.  Needs the scratch of the first split
    // problem (the same buffer on every descriptor of a step: ops.splitk_workspace) to hold every part, and its counters.
    // CB_GROUP_SLAB=0 keeps the atomics.
    if (dtype == CB_BF16 && !switches().group_slab_off && (cls == GC_WGRAD || cls == GC_WGRAD_GATHER)) {
        const int B = gp.tile == 4 ? 128 : 64;
        int64_t units = 0, tiles_split = 0;
        const cb_gemm_desc* first = nullptr;
        bool ok = true;
        for (size_t i = 0; i < g.size(); ++i) {
            const cb_gemm_desc* d = g[i]->d;
            const int kt = g[i]->pr.p.ktiles;
            const int si = splits[i] > kt ? (kt > 0 ? kt : 1) : splits[i];
            if (si <= 1) continue;
            units += group_tiles(d, B) * si;
            tiles_split += group_tiles(d, B);
            if (!first) first = d;
            ok = ok && d->splitk_ws == first->splitk_ws && g[i]->pr.p.batch == 1 && !d->a_rowsum && !d->c_rowmap;
        }
        if (first && ok && first->splitk_ws && aligned16(first->splitk_ws) && first->splitk_ws_bytes % 4 == 0 &&
            units * B * B * 4 <= splitk_payload_bytes(first->splitk_ws_bytes) && tiles_split <= GROUP_COUNTERS) {
            for (size_t i = 0; i < g.size(); ++i) ok = ok && (splits[i] <= 1 || g[i]->d->splitk_ws_bytes == first->splitk_ws_bytes);
            gp.cnt = ok ? splitk_counters(first->splitk_ws, first->splitk_ws_bytes) : nullptr;
            if (gp.cnt) gp.slab = reinterpret_cast<float*>(first->splitk_ws);
        }
    }
    if (!gp.slab)                                                   // first writers / norm shares never combine through atomics: unsplit without a scratch
        for (size_t i = 0; i < g.size(); ++i)
            if (g[i]->d->accumulate == 2 || g[i]->d->sq_slots) splits[i] = 1;
}

// ---- launch one group: the problems' parameter blocks with their ranges of workgroups, slab units and counters
int group_launch(const std::vector<GroupItem*>& g, int dtype, int cls, const GroupPlan& gp, hipStream_t st) {
    const Switches& sw = switches();
    const int B = (dtype == CB_BF16 && gp.tile == 4) ? 128 : 64;
    GroupArgs ga{};
    ga.n = (int)g.size();
    ga.slab = gp.slab;
    ga.cnt = gp.slab ? gp.cnt : nullptr;
    int64_t slab_units = 0;
    int cnt_tiles = 0;
    int xcd = 0;
    int64_t acc = 0;
    for (size_t i = 0; i < g.size(); ++i) {
        const cb_gemm_desc* d = g[i]->d;
        const Prepared& pr = g[i]->pr;
        GP p = pr.p;
        p.split_k = gp.splits[i] > p.ktiles ? (p.ktiles > 0 ? p.ktiles : 1) : gp.splits[i];
        if (p.split_k > 1) {
            CB_REQUIRE(d->c_f32 && (d->accumulate == 1 || gp.slab), "cb_gemm_group: split_k > 1 needs an fp32 output accumulated into, or the slab scratch");
            CB_REQUIRE(pr.epi_scale_only, "cb_gemm_group: split_k > 1 supports only scale/alpha in the epilogue");
        }
        p.c_vec8 = pr.cv8 && (p.split_k == 1 || gp.slab);
        const int64_t tiles = group_tiles(d, B);
        if (gp.slab && p.split_k > 1) {
            CB_REQUIRE(slab_units < (1ll << 31), "cb_gemm_group: slab index overflow");
            p.slab_base = (int)slab_units;
            p.cnt_base = cnt_tiles;
            slab_units += tiles * p.split_k;
            cnt_tiles += (int)tiles;
        }
        if (d->xcd_order != 0) xcd = d->xcd_order;
        acc += tiles * p.split_k * (p.batch > 1 ? p.batch : 1);
        CB_REQUIRE(acc < (1ll << 30), "cb_gemm_group: too many workgroups");
        ga.tile_end[i] = (int)acc;
        CB_STAMP_ASSIGN(p, d, gp.tile, p.split_k, 0, (int)i, (int)g.size());
        ga.g[i] = p;
        if (sw.trace) fprintf(stderr, "cb_gemm_group[%zu/%zu]: M=%d N=%d K=%d modes=%d/%d cls=%d tile=%d split=%d%s\n", i, g.size(), d->M, d->N, d->K, d->a_mode,
                              d->b_mode, cls, gp.tile, p.split_k, gp.slab && p.split_k > 1 ? " slab" : "");
    }
    ga.xcd_remap = !sw.no_xcd_remap && xcd != 2;
    if (dtype == CB_F32) return launch_gemm_group<float, 64, 64, 2, 1>(ga, cls, st);
    if (gp.tile == 4) return launch_gemm_group<bf16, 128, 128, 1, 2>(ga, cls, st);
    return launch_gemm_group<bf16, 64, 64, 3, 1>(ga, cls, st);
}
}  // namespace

extern "C" int cb_gemm_group(const cb_gemm_desc* descs, int32_t n, void* stream) {
    CB_REQUIRE(n >= 0 && (n == 0 || descs != nullptr), "cb_gemm_group: bad arguments");
    std::vector<GroupItem> items;
    items.reserve(n);
    for (int i = 0; i < n; ++i) {
        const cb_gemm_desc* d = descs + i;
        CB_REQUIRE(d->M >= 0 && d->N >= 0 && d->K >= 0, "cb_gemm_group: negative dims (problem %d)", i);
        if (d->M == 0 || d->N == 0) continue;
        GroupItem it{d, Prepared{}, -1};
        if (int rc = gemm_prepare(d, it.pr)) return rc;
        it.cls = switches().no_group ? -1 : group_class(d, it.pr);
        items.push_back(it);
    }
    std::vector<char> done(items.size(), 0);
    for (size_t i = 0; i < items.size(); ++i) {
        if (done[i]) continue;
        if (items[i].cls < 0) {                                           // not covered by a grouped kernel
            done[i] = 1;
            if (int rc = gemm_run(items[i].d, items[i].pr, stream)) return rc;
            continue;
        }
        std::vector<GroupItem*> bucket;                                   // same dtype and class (and an explicit tile request in common), caller's order
        for (size_t j = i; j < items.size(); ++j)
            if (!done[j] && items[j].cls == items[i].cls && items[j].d->dtype == items[i].d->dtype && items[j].d->tile == items[i].d->tile) {
                bucket.push_back(&items[j]);
                done[j] = 1;
            }
        if (bucket.size() == 1) {
            if (int rc = gemm_run(bucket[0]->d, bucket[0]->pr, stream)) return rc;
            continue;
        }
        const size_t nchunks = (bucket.size() + GROUP_MAX - 1) / GROUP_MAX;
        const size_t per = (bucket.size() + nchunks - 1) / nchunks;
        for (size_t c = 0; c < bucket.size(); c += per) {
            std::vector<GroupItem*> chunk(bucket.begin() + c, bucket.begin() + (c + per < bucket.size() ? c + per : bucket.size()));
            GroupPlan gp;
            group_choose(chunk, items[i].d->dtype, items[i].cls, gp);
            if (int rc = group_launch(chunk, items[i].d->dtype, items[i].cls, gp, cb_stream(stream))) return rc;
        }
    }
    return 0;
}

extern "C" int cb_build_pixel_table(cb_pixel* tab, int32_t N, int32_t OH, int32_t OW, int32_t stride, int32_t pad,
                                    int64_t sN, int64_t sH, int64_t sW, void* stream) {
    CB_REQUIRE(tab && N > 0 && OH > 0 && OW > 0 && stride > 0, "cb_build_pixel_table: bad arguments");
    int64_t total = (int64_t)N * OH * OW;
    CB_REQUIRE(total < (1ll << 31), "cb_build_pixel_table: too many pixels");
    CB_REQUIRE((int64_t)N * sN < (1ll << 31), "cb_build_pixel_table: image offsets exceed 31 bits");
    hipLaunchKernelGGL(pixel_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, cb_stream(stream), tab,
                       (int)total, OH, OW, stride, pad, sN, sH, sW);
    return cb_launch_status("cb_build_pixel_table");
}
