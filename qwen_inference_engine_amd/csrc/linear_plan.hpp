// linear_plan.hpp — which kernel, in which variant and on which grid, an M <= 16 linear layer
// (qie_linear) launches.  Pure host code (no HIP call): plan_linear() names every choice that
// k_gemv.hip's gemv() then only executes, and launch_geometry() turns a plan into
// (grid, threads, dynamic LDS bytes), so the whole decision can be printed and tested without a
// GPU (tools/plan_dump.cpp, tests/test_linear_plan_cpu.py).  The comments that record measured
// A/B results sit beside the decision they explain.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/qie/qie_ops.h"

namespace qie {

struct PeerPush;   // qie_common.hpp

// ------------------------------------------------------------------ dev knobs
// Every A/B knob of the M <= 16 linear path, with the shipped defaults.  The development build
// fills it from the environment (k_gemv.hip dev_knobs(), one place); the shipped library uses
// the defaults as they stand.  kAuto: the default depends on the shape (see plan_linear).
constexpr int kAuto = INT_MIN;
struct Knobs {
    int epre = 1;             // QIE_GEMV_EPRE
    int mkdiv = 0;            // QIE_GEMV_MKDIV
    int gemv_dbg = 0;         // QIE_GEMV_DBG (M = 1 timing experiments: 1 no norm, 2 no bias)
    int blocks_per_cu = -1;   // QIE_GEMV_BLOCKS_PER_CU
    int xfirst = 1;           // QIE_GEMV_XFIRST
    int xreg = kAuto;         // QIE_GEMV_XREG (default: 1 for vocabulary rows, else 0)
    int xreg4 = 0;            // QIE_GEMV_XREG4
    int xreg4_lm = 0;         // QIE_GEMV_XREG4_LM
    int xreg4_sw = 1;         // QIE_GEMV_XREG4_SW
    int swiglu_bpc = kAuto;   // QIE_GEMV_SWIGLU_BPC
    int lm_bpc = kAuto;       // QIE_GEMV_LM_BPC
    int res_bpc = -1;         // QIE_GEMV_RES_BPC
    int qkv_bpc = kAuto;      // QIE_GEMV_QKV_BPC
    int balanced = 1;         // QIE_GEMV_BALANCED
    int rpw1 = 1;             // QIE_GEMV_RPW1
    int skinny_mfma = 1;      // QIE_SKINNY_MFMA
    int skinny_lds64 = 1;     // QIE_SKINNY_LDS64
    int skinny_xl = -1;       // QIE_SKINNY_XL
    int skinny_dbg = 0;       // QIE_SKINNY_DBG
    int skinny_bpc = 0;       // QIE_SKINNY_BPC
    int dec8 = 1;             // QIE_DEC8
    int dec8_split = 1;       // QIE_DEC8_SPLIT
    int dec8_split_ku = 4;    // QIE_DEC8_SPLIT_KU
    int t16_skinny = 0;       // QIE_T16_SKINNY
};
inline int knob_or(int knob, int dflt) { return knob == kAuto ? dflt : knob; }

// ------------------------------------------------------------------ extras
// What a caller inside the library can pass beside the public argument block.
struct RopeArgs {   // interleaved RoPE in the STORE epilogue (GemvParams::rope_*)
    const int32_t* pos = nullptr;
    const float* cs = nullptr;
    const float* sn = nullptr;
    int hd = 0;
    int64_t rows = 0;
};
struct LinearExtras {
    RopeArgs rope;
    // M = 1, F32 epilogue: push the outputs into the peer backend's tagged exchange slots;
    // *push_taken reports whether the launch did (only gemv_kernel can)
    const PeerPush* push = nullptr;
    bool* push_taken = nullptr;
};

// ------------------------------------------------------------------ the plan
enum class LinearFamily { Dec8, Skinny, Gemm, Gemv, Dec4 };
enum class PlanError { None, TiledShape, NormLds, Fp8K16, NormRouted, Fp4Flags, Fp4Rows, Fp4K, Fp4Shape };

constexpr int kGemvBalancedThreads = 576;   // block size bound of the one-block-per-CU GEMV (9 waves)
constexpr size_t kGemvLdsCap = 96 * 1024;
constexpr size_t kSkinnyLdsCap = 120 * 1024;
constexpr int kDec8MaxTiles = 2048, kDec8MaxParts = 16;   // N <= 32,768 (dec8_plan)

struct LinearPlan {
    LinearFamily family = LinearFamily::Gemv;
    PlanError error = PlanError::None;
    int epi = 0;
    // gemv_kernel<MT, RPW, EPI, U, XCH, WT> / skinny_mfma_kernel<EPI, WT, XL, 4, UO>
    int mt = 1, rpw = 2, xch = 0, uo = 0, wt = 0;
    int xlds = 0;            // x (the M rows) staged in LDS
    int64_t n_tasks = 0;     // GEMV row tasks / skinny column tiles
    // GEMV grid policy: N > 0 a cap of N blocks per CU, -1 / 0 the occupancy-balanced
    // persistent grid, -2 the full-residency grid-stride grid (launch_geometry)
    int bpc = -1;
    // one block per CU with this many waves (0: 4-wave blocks on the bpc grid); the kernel is
    // then the instantiation bounded at 1,024 (rpw 1) or kGemvBalancedThreads threads
    int block_waves = 0;
    int skinny_bpc = 0;      // skinny kernel: cap of blocks per CU (0: all resident)
    size_t lds_bytes = 0;    // dynamic LDS of the launch
    int dbg = 0;             // GemvParams::dbg
    bool t16 = false;        // skinny kernel on 16-row tiled fp8 weights
    bool push = false;       // GemvParams::push taken from the extras
    int dec8_ku = 0, dec8_ks = 0, dec8_parts = 0;   // Dec8: K slice shape; parts >= 2: split-K
    int dec4_ku = 0, dec4_ks = 0, dec4_parts = 0;   // Dec4: the same of the MXFP4 kernel (128-column units)
    bool needs_occupancy() const {
        return family == LinearFamily::Skinny ? skinny_bpc <= 0
                                              : family == LinearFamily::Gemv && block_waves == 0 && bpc <= 0;
    }
    int threads() const { return block_waves ? 64 * block_waves : 256; }
};

struct LaunchGeom {
    unsigned grid;
    int threads;
    size_t lds_bytes;
};

// ------------------------------------------------------------------ fp8 batched decode
// K slice shapes: (units per wave KU, waves KS) with KU * KS * 64 = K.  7 waves x 8 units at
// K = 3,584 (14 x 4 measured the same for QKV and 0.45 µs slower for O at config 4).
// Long K without such a shape (the down projection's 18,944 = 296 units): split-K over
// parts of 8 waves x 4 units (10 parts at 18,944, the last one ragged; 128 VGPRs, two blocks
// per CU), single-segment epilogues without a fused norm only (a norm needs the whole row in
// one block).  Config 4 (fp8, B = 8), same box: the general skinny kernel 2,895 tok/s (down
// 24.9 µs live), split 8 x 8 units 2,990 (23.4), 8 x 4 units 3,010 (23.0); the first form,
// which published each tile's parts as it finished it, stalled every wave on its ticket
// round trip behind the per-tile barrier: 2,760 (31.5).
inline bool dec8_shape(int64_t K, int* ku, int* ks) {
    if (K % 64 != 0) return false;
    const int64_t units = K / 64;
    constexpr int shapes[][2] = {{8, 7}, {8, 8}, {2, 7}, {4, 8}, {8, 4}};
    for (const auto& s : shapes)
        if ((int64_t)s[0] * s[1] == units) {
            *ku = s[0];
            *ks = s[1];
            return true;
        }
    return false;
}
inline int dec8_split_parts(const qie_linear_args& a, const Knobs& k, int* ku) {
    if (a.K % 64 != 0 || a.norm_w || a.epilogue == QIE_EPI_SWIGLU || a.seg_rows[1] > 0) return 0;
    if (a.N > (int64_t)kDec8MaxTiles * 16) return 0;   // the ticket array
    // (tiled weights can be read by this kernel only: the dev switch does not apply to them)
    if (!(a.flags & QIE_LINEAR_FP8_T16) && k.dec8_split == 0) return 0;
    const int64_t units = a.K / 64;
    *ku = k.dec8_split_ku == 8 ? 8 : 4;
    const int64_t parts = (units + 8 * *ku - 1) / (8 * *ku);
    return parts >= 2 && parts <= kDec8MaxParts ? (int)parts : 0;
}
// true when the fp8 batched-decode kernel (k_decode_fp8.hip) takes this projection; then
// (*ku, *ks) is its K slice shape and *parts >= 2 its split-K parts (1: no split)
inline bool dec8_plan(const qie_linear_args& a, const Knobs& k, int* ku, int* ks, int* parts) {
    // tiled weights (QIE_LINEAR_FP8_T16) are read by this kernel only, at any 1 <= M <= 16
    const bool t16 = (a.flags & QIE_LINEAR_FP8_T16) != 0;
    if (!(a.flags & QIE_LINEAR_FP8) || a.M < (t16 ? 1 : 2) || a.M > 16) return false;
    if (t16 && k.t16_skinny != 0) return false;   // dev A/B: tiled projections on the skinny kernel
    if (!t16 && k.dec8 == 0) return false;
    *parts = 1;
    if (!dec8_shape(a.K, ku, ks)) {
        *ks = 8;
        *parts = dec8_split_parts(a, k, ku);
        if (*parts == 0) return false;
    }
    // vocabulary-sized projections (tens of tiles per block) keep the general skinny kernel:
    // its 16 waves per CU keep more bytes in flight than one 7-wave block (lm_head 119 vs 194 µs)
    // (tiled vocabulary projections go to the skinny kernel, which reads the layout too)
    if (a.N <= 0 || a.N > 32768 || a.ldx % 8 != 0 || a.K >= (1 << 20)) return false;
    if (a.epilogue != QIE_EPI_SWIGLU) {
        // column tiles must not straddle segments
        if (a.seg_rows[0] % 16 != 0 || (a.seg_rows[1] > 0 && (a.seg_rows[0] + a.seg_rows[1]) % 16 != 0))
            return false;
    }
    // tiled weights: whole 16-row tiles per segment
    if (t16) {
        if (a.epilogue == QIE_EPI_SWIGLU ? a.N % 16 != 0
                                         : (a.seg_rows[0] % 16 != 0 || a.seg_rows[1] % 16 != 0 || a.seg_rows[2] % 16 != 0))
            return false;
    }
    // every segment's codes + scales must fit a 32-bit buffer range
    for (int s = 0; s < 3; s++)
        if ((int64_t)(a.epilogue == QIE_EPI_SWIGLU ? a.N : a.seg_rows[s]) * (a.K + 4) >= (int64_t)1 << 31)
            return false;
    return true;
}

// ------------------------------------------------------------------ MXFP4 batched decode
// The MXFP4 kernel (k_decode_fp4.hip) is the only reader of fp4 weights: what it does not take is
// refused (a PlanError, -22 from qie_linear), never routed to another kernel.  Units are 128
// columns (one 16-B load per lane = one 32-element MX block = four MFMA operands).  K slice
// shapes: KU units per wave (2, 4 or 8: 16 KU VGPRs of A fragments), KS = ceil(units / KU)
// waves; the last wave's slice may be ragged (its units past K are zero rows and loads out of
// the buffer range).  KU is the smallest of 2 / 4 / 8 with KS <= 4 / 8 / 8, so every K up to 64
// units (8,192) is taken unsplit, fused norm included: 896 = 2 x 4 (7 units), 3,584 = 4 x 7,
// 5,120 = 8 x 5, 8,192 = 8 x 8.  Longer K: split-K over parts of 8 waves x 2 units (2,048
// columns; 18,944 = 10 parts, 17,408 = 9, 29,568 = 15), single-segment epilogues without a norm.
constexpr int kDec4MaxUnits = 64, kDec4SplitKu = 2, kDec4SplitKs = 8;
inline PlanError dec4_plan(const qie_linear_args& a, int* ku, int* ks, int* parts) {
    const bool t16 = (a.flags & QIE_LINEAR_FP4_T16) != 0;
    if (!(a.flags & QIE_LINEAR_FP4) || (a.flags & (QIE_LINEAR_FP8 | QIE_LINEAR_FP8_T16 | QIE_LINEAR_ACT_FP8)))
        return PlanError::Fp4Flags;
    if (a.M < 1 || a.M > 16) return PlanError::Fp4Rows;
    if (a.K <= 0 || a.K % 128 != 0) return PlanError::Fp4K;
    if (a.N <= 0 || a.N > 32768 || a.ldx % 8 != 0 || a.K >= (1 << 20)) return PlanError::Fp4Shape;
    const bool sw = a.epilogue == QIE_EPI_SWIGLU;
    // column tiles must not straddle segments: a segment that another follows is whole tiles (the
    // last one may end in a ragged tile: its rows are clamped); tiled weights: whole tiles everywhere
    if (!sw && ((a.seg_rows[0] % 16 != 0 && (a.seg_rows[1] > 0 || a.seg_rows[2] > 0)) ||
                ((a.seg_rows[0] + a.seg_rows[1]) % 16 != 0 && a.seg_rows[2] > 0)))
        return PlanError::Fp4Shape;
    if (t16 && (sw ? a.N % 16 != 0 : (a.seg_rows[0] % 16 != 0 || a.seg_rows[1] % 16 != 0 || a.seg_rows[2] % 16 != 0)))
        return PlanError::Fp4Shape;
    // every segment's codes + scales must fit a 32-bit buffer range
    for (int s = 0; s < 3; s++)
        if ((int64_t)(sw ? a.N : a.seg_rows[s]) * (a.K / 2 + a.K / 32) >= (int64_t)1 << 31) return PlanError::Fp4Shape;
    const int64_t units = a.K / 128;
    *parts = 1;
    if (units <= kDec4MaxUnits) {
        *ku = units <= 8 ? 2 : (units <= 32 ? 4 : 8);
        *ks = (int)((units + *ku - 1) / *ku);
        return PlanError::None;
    }
    if (a.norm_w || sw || a.seg_rows[1] > 0 || a.N > (int64_t)kDec8MaxTiles * 16) return PlanError::Fp4Shape;
    const int64_t per = kDec4SplitKu * kDec4SplitKs;
    const int64_t np = (units + per - 1) / per;
    if (np > kDec8MaxParts) return PlanError::Fp4Shape;
    *ku = kDec4SplitKu;
    *ks = kDec4SplitKs;
    *parts = (int)np;
    return PlanError::None;
}

// ------------------------------------------------------------------ GEMV pieces
inline bool K_fits(int64_t K, int xch) { return K <= 2048 * (int64_t)xch && K % 8 == 0; }

// One block per CU for mid-sized GEMVs (4..16 row tasks per CU: Qwen2-7B QKV 2,304, O and
// down 1,792): 448 four-wave blocks on 256 CUs left 64 CUs with half the waves, and the
// whole launch waited for the doubly loaded CUs.  Block = ceil(tasks / CUs) waves, so every
// CU streams the same rows.  (SwiGLU and lm_head have > 9 tasks per CU: grid-stride.)
// One row per wave: up to 16 waves per block (Qwen2-7B O / down: 14 one-row waves per CU).
// THE condition: it picks the x-beside-the-weights variant (XCH 1) in plan_linear and the
// block size in launch_geometry.
inline bool one_block_per_cu(int mt, bool fp8, int epi, int bpc, int64_t n_tasks, int rpw, int cus, const Knobs& k) {
    const int64_t max_waves = (rpw == 1 ? 1024 : kGemvBalancedThreads) / 64;
    return mt == 1 && !fp8 && epi != QIE_EPI_SWIGLU && bpc < 0 && n_tasks > 4 * (int64_t)cus &&
           n_tasks <= max_waves * cus && k.balanced != 0;
}

// Chunks in flight per row (UO, 0 = the default 8) sized to K (bf16
// wave-loads per row n), so no load slot re-reads the row's tail: n <= 2 (Qwen2-0.5B, K = 896):
// 2 instead of 8 slots, 6 of them duplicates — lm_head 72.1 -> 47.4 us, gate/up 8.4 -> 6.3,
// decode 1,283 -> 1,471 tok/s; n = 7 (Qwen2-7B, K = 3,584): 7 instead of 8 — gate/up
// 44.2 -> 42.9, QKV 9.67 -> 9.41 us, 349 -> 354 tok/s, but lm_head 166 -> 175 us (25 row tasks
// per wave: there the 8th slot's duplicate costs less than the bytes in flight it drops), so
// the vocabulary projection keeps 8; n = 10 (Qwen3-14B, K = 5,120): 5 per pass, two passes.
// (A slot past K re-reads the row's last 16 B, so at K = 896 the default issued 8 loads per
// row of which 6 were duplicates.)
inline int gemv_uo(int xch, int64_t K, int64_t n_tasks, int rpw) {
    const int64_t n = (K + 511) / 512;   // bf16 wave-loads per row
    const bool vocab = n_tasks * rpw >= 65536;
    const int64_t ub = (n + (n + 7) / 8 - 1) / ((n + 7) / 8);   // balanced slots per pass (<= 8)
    if (xch == 3 || xch == 4)   // fused norm, x in registers: one batch of wave-loads covers a row
        return n <= 2 ? 2 : (n == 7 && !vocab ? 7 : 8);
    if (xch == 2 && n <= 2) return 2;
    if (xch == 2 && n == 7 && !vocab) return 7;
    if (xch == 5 && (n == 9 || n == 10) && !vocab) return 5;
    // K <= 20,480 without a norm (Qwen3-14B O at K = 5,120: 2 x 5; down at K = 17,408: 5 x 7)
    if (xch == 10 && (ub == 5 || ub == 7) && !vocab) return (int)ub;
    if (xch == 1 && n == 7) return 7;
    return 0;
}

// ------------------------------------------------------------------ plan_linear
// allow_dec8 = false: the fp8 batched-decode kernel declined (its split-K workspace cannot be
// made during a graph capture); plan the general kernels.
inline LinearPlan plan_linear(const qie_linear_args& a, const LinearExtras& ex, int cus, const Knobs& k,
                              bool allow_dec8 = true) {
    LinearPlan pl;
    pl.epi = a.epilogue;
    const bool fp8w = (a.flags & QIE_LINEAR_FP8) != 0;
    const bool has_norm = a.norm_w != nullptr;
    const int NB = a.epilogue == QIE_EPI_SWIGLU ? 2 : 1;
    // MXFP4 weights: k_decode_fp4.hip or an error (at any M: qie_linear sends every fp4 launch here)
    if (a.flags & (QIE_LINEAR_FP4 | QIE_LINEAR_FP4_T16)) {
        pl.error = dec4_plan(a, &pl.dec4_ku, &pl.dec4_ks, &pl.dec4_parts);
        pl.family = LinearFamily::Dec4;
        pl.wt = 2;
        pl.n_tasks = (a.N + 15) / 16;
        return pl;
    }
    // fp8 weights, 2..16 rows, K a whole number of per-wave slices (or split-K): k_decode_fp8.hip
    if (allow_dec8 && dec8_plan(a, k, &pl.dec8_ku, &pl.dec8_ks, &pl.dec8_parts)) {
        pl.family = LinearFamily::Dec8;
        pl.wt = 1;
        pl.n_tasks = (a.N + 15) / 16;
        return pl;
    }
    // 16-row tiled fp8 weights the batched-decode kernel did not take (the vocabulary
    // projection): the skinny kernel reads them, at any 1 <= M <= 16 (qie_linear checked the shape)
    pl.t16 = (a.flags & QIE_LINEAR_FP8_T16) != 0;
    if ((a.M >= 2 || pl.t16) && a.M <= 16 && (pl.t16 || k.skinny_mfma != 0)) {
        const int kstep = 64;
        const bool lds_ok = (size_t)a.M * (a.K + 8) * 2 <= kSkinnyLdsCap;
        const bool takes = a.K % kstep == 0 && (lds_ok || !has_norm);
        if (pl.t16 && !(fp8w && takes)) {
            pl.error = PlanError::TiledShape;
            return pl;
        }
        if (takes) {
            pl.family = LinearFamily::Skinny;
            pl.wt = fp8w ? 1 : 0;
            // Stage the M rows in LDS only when the norm is fused (it needs them) or a block
            // serves several column tiles (gate/up, lm_head: the copy is amortised); with
            // about one tile per CU (QKV, O, down) each wave loads its A fragments from L2
            // with its weight steps instead of a 57-KB copy + barrier per block (config 4,
            // fp8: O 9.7 -> 7.8 us, down 26.4 -> 24.6; bf16 O 11.6 -> 10.1, QKV 16.5 -> 15.3)
            pl.n_tasks = (a.N + 15) / 16;
            pl.xlds = lds_ok && (has_norm || pl.n_tasks > 2 * (int64_t)cus) ? 1 : 0;
            // Without a fused norm the staged copy is only an optimisation: keep the launch's
            // dynamic LDS within the default 64 KiB (no raised kernel attribute).  r02's config-4
            // gate/up node (8 rows x 3,592 + two 4-KiB reduction tiles per wave = 65,664 B) was
            // the one decode-graph node above it, and rocprofv3's kernel trace crashed on that
            // graph only; with NW - 1 reduction tiles it is 63,616 B and stays staged.
            const size_t staged = (size_t)a.M * (a.K + 8) * 2 + NB * 3072;
            if (pl.xlds && !has_norm && staged > 65536 && k.skinny_lds64 != 0) pl.xlds = 0;
            if (k.skinny_xl >= 0) pl.xlds = k.skinny_xl && lds_ok ? 1 : 0;
            pl.dbg = k.skinny_dbg;
            // fp8: 7 units per step where a wave's K range is 7 or 14 units (Qwen2-7B, K = 3,584:
            // 2 steps of 7 instead of 4 of 4 / 2 of 8 with two dead units).  Config 4 (fp8, B = 8):
            // gate/up 36.2 -> 35.2, O 8.4 -> 7.45, lm_head 129 -> 122 us, 2,509 -> 2,535 tok/s
            const int64_t uw = (a.K / 64 + 3) / 4;
            pl.uo = fp8w && (uw == 7 || uw == 14) ? 7 : 0;
            // reduction tiles: NW - 1 = 3 partial C tiles per B tile (>= 64 floats for the norm prologue)
            pl.lds_bytes = (pl.xlds ? (size_t)a.M * (a.K + 8) * 2 : 0) + (size_t)3 * NB * 256 * 4;
            // dev A/B: blocks per CU (0: all resident — config 4's tiled lm_head 100.1 µs; caps
            // 1 / 2 / 3 / 6 measured 101.9 / 100.5 / 111.0 / 127.7)
            pl.skinny_bpc = k.skinny_bpc;
            return pl;
        }
    }
    if (a.M > 8) {   // 9..16 rows the skinny kernel could not take
        pl.family = LinearFamily::Gemm;
        return pl;
    }
    pl.family = LinearFamily::Gemv;
    pl.wt = fp8w ? 1 : 0;
    pl.push = ex.push && a.M == 1 && a.epilogue == QIE_EPI_F32;   // every M = 1 launch below is gemv_kernel
    pl.dbg = a.M == 1 ? k.gemv_dbg : 0;
    const int MT = a.M <= 1 ? 1 : a.M <= 2 ? 2 : a.M <= 4 ? 4 : 8;
    pl.mt = MT;
    pl.xlds = ((size_t)MT * a.K * 2 <= kGemvLdsCap) ? 1 : 0;
    if (!pl.xlds && has_norm) {
        pl.error = PlanError::NormLds;
        return pl;
    }
    const int64_t rows = a.epilogue == QIE_EPI_SWIGLU ? 2 * a.N : a.N;
    // Rows per wave: 2, or 1 below.  (4, since removed, measured slower for every Qwen2-7B decode
    // GEMV on MI355X: down 23.7 vs 28.0 us, qkv 9.7 vs 10.9, o 6.6 vs 7.7, gate/up 42.9 vs 43.8;
    // vocabulary rows 165.9 vs 164.8 us, 53.4 vs 48.7 at Qwen2-0.5B.)
    int rpw = 2;
    int64_t n_tasks = (rows + rpw - 1) / rpw;
    // Grid (QIE_GEMV_BLOCKS_PER_CU): default (auto) = one block per CU with ceil(tasks / CUs)
    // waves where 4..9 tasks per CU (Qwen2-7B QKV, O, down), else the occupancy-balanced
    // persistent grid (lm_head 169 vs 183 us, gate/up 43.1 vs 43.5 against a cap of 8 blocks
    // per CU); 0 = always the occupancy grid; N > 0 = cap of N blocks per CU.
    int bpc = k.blocks_per_cu;
    auto finish = [&](int xch) {
        pl.rpw = rpw;
        pl.n_tasks = n_tasks;
        pl.bpc = bpc;
        pl.xch = xch;
        pl.uo = MT == 1 && !fp8w ? gemv_uo(xch, a.K, n_tasks, rpw) : 0;
        pl.lds_bytes = (pl.xlds ? (size_t)MT * a.K * 2 : 0) + 64;
        if (one_block_per_cu(MT, fp8w, a.epilogue, bpc, n_tasks, rpw, cus, k))
            pl.block_waves = (int)((n_tasks + cus - 1) / cus);
        return pl;
    };
    if (fp8w) {
        if (a.K % 16 != 0) {
            pl.error = PlanError::Fp8K16;
            return pl;
        }
        return finish(0);
    }
    // x-first prologue + cross-task weight prefetch (QIE_GEMV_XFIRST, MT = 1).  A first
    // attempt that issued the weights BEFORE x was slower everywhere (qkv 11.4 vs 9.4 us):
    // x then queued behind the weights in the in-order vmcnt.
    int xch = 0;
    // The x-first variants with a fused RMSNorm are XCH 2 and 5 (the norm weights ride along
    // with x); XCH 10 (down, K = 18,944) stages x only — a fused norm there would be dropped,
    // so a normed K > 10,240 takes the generic prologue.
    const bool m1 = MT == 1 && a.M == 1;
    if (m1 && pl.xlds && k.xfirst != 0) {
        if (has_norm) xch = K_fits(a.K, 2) ? 2 : (K_fits(a.K, 5) ? 5 : 0);
        else xch = K_fits(a.K, 2) ? 2 : (K_fits(a.K, 10) ? 10 : 0);
    }
    // Fused norm with a per-wave sum of squares (XCH 3) where one batch of <= 8 wave-loads
    // covers a row (K <= 4,096, K % 8 == 0: Qwen2-7B QKV / gate/up / lm_head at K = 3,584,
    // Qwen2-0.5B at 896): no block reduction, one barrier before the weight stream.
    // Measured (tools/ubench.py, Qwen2-7B): lm_head 175.3 -> 167.4 us; QKV (9.14 vs 9.67) and
    // gate/up (42.7 vs 43.8) are faster with the x-first prologue's one-chunk-per-thread x
    // loads, so only the vocabulary projection takes it.
    const bool vocab_rows = rows >= 65536;
    const bool xreg_ok = m1 && has_norm && a.K % 8 == 0 && a.K <= 4096;
    if (xreg_ok && knob_or(k.xreg, vocab_rows ? 1 : 0) != 0) xch = 3;
    // Normalised x in every wave's registers (XCH 4): no LDS image, no barrier.  Default for
    // gate/up (5 row tasks per wave reuse it): 361.5 -> 362.7 tok/s at Qwen2-7B; the QKV
    // projection (one task per wave) pays the per-wave divisions on its critical path:
    // 9.98 -> 14.6 us (dev knobs QIE_GEMV_XREG4 / _LM / _SW)
    if (xreg_ok && (a.epilogue == QIE_EPI_SWIGLU ? k.xreg4_sw : (vocab_rows ? k.xreg4_lm : k.xreg4)) != 0) {
        xch = 4;
        pl.xlds = 0;
    }
    // gate/up grid: full residency, grid-stride (-2, launch_geometry); QIE_GEMV_SWIGLU_BPC = N > 0
    // caps N blocks per CU, -1 the balanced grid (dev A/B)
    //
    // Round 5, grid caps measured per shape (same box, interleaved, in the graph: tools/ab_decode.py;
    // outputs bit-identical — the grid only changes which wave takes which row task):
    //  * gate/up, Qwen2-7B (K 3,584, 74 row tasks per CU; 198 VGPRs, 2 resident blocks per CU):
    //    6 blocks per CU 42.7 -> 41.3 µs, 361.8 -> 366.7 tok/s — a sharp optimum (5: 357.4,
    //    8: 358.1, 10: 343.2; the full-residency grid, 2 per CU, 361.8);
    //  * gate/up, Qwen2-0.5B (K 896, 19 tasks per CU; 62 VGPRs): 3 per CU 6.48 -> 5.22 µs,
    //    1,484 -> 1,542 tok/s (2: 1,543, 4: 1,511, 5: 1,483);
    //  * lm_head (vocabulary rows, occupancy-balanced grid otherwise): K 896 5 per CU
    //    53.4 -> 48.8 µs; K 3,584 2 per CU 167.3 -> 164.7 µs.
    // Shapes outside those ranges keep the former grids (unmeasured there).
    if (a.epilogue == QIE_EPI_SWIGLU && MT == 1 && bpc < 0) {
        const int64_t tpc = n_tasks / cus;
        int dflt = -2;
        if (a.K <= 1024 && tpc <= 32) dflt = 3;
        else if (a.K >= 3072 && a.K <= 4096 && tpc >= 64 && tpc <= 96) dflt = 6;
        bpc = knob_or(k.swiglu_bpc, dflt);
    }
    if (vocab_rows && MT == 1 && bpc < 0) bpc = knob_or(k.lm_bpc, a.K <= 1024 ? 5 : (a.K <= 4096 ? 2 : -1));
    // The normed STORE projection (QKV), Qwen2-7B (K 3,584, 9 row tasks per CU): 2 blocks of 4
    // waves per CU instead of one 9-wave block, 9.77 -> 9.26 µs, 367.4 -> 369.4 tok/s (1: 357.2,
    // 3: 364.8, 4: 364.8).  The fused norm's sum of squares is then reduced over 256 threads
    // instead of 576 (another fp32 order of the same sum; the parity tests bound it).
    // Qwen2-0.5B's QKV: equal at 1-3 per CU, kept.
    // (dev A/B) residual projections (O, down): caps 3 / 5 / 6 / 8 per CU all ran Qwen2-7B at
    // 363.4-363.5 vs 369.6 tok/s on their one-block-per-CU layout; 0.5B equal
    if (MT == 1 && a.epilogue == QIE_EPI_RESIDUAL && bpc < 0) bpc = k.res_bpc;
    if (!vocab_rows && MT == 1 && has_norm && a.epilogue == QIE_EPI_STORE && bpc < 0) {
        const int64_t tpc = n_tasks / cus;
        bpc = knob_or(k.qkv_bpc, a.K >= 3072 && a.K <= 4096 && tpc >= 6 && tpc <= 12 ? 2 : -1);
    }
    // Batch-1 GEMVs without a fused norm on the one-block-per-CU grid (one row task per
    // wave: Qwen2-7B O, down) read x from L2 beside each weight chunk (XCH = 1) instead of
    // staging it in LDS behind a barrier: Qwen2-7B decode 355 -> 358 tok/s (two A/B rounds),
    // in-graph down 24.5 -> 23.5 us, O 7.3 -> 7.05.  Where a wave walks several row tasks
    // (Qwen3-14B O / down, 10 per CU; Qwen2-0.5B) x would be re-read per task: O 13.1 ->
    // 16.5, down 32.9 -> 39.7 us at 14B, so those keep the staged copy.
    if (m1 && !has_norm && a.K % 8 == 0 && one_block_per_cu(MT, fp8w, a.epilogue, bpc, n_tasks, rpw, cus, k)) {
        xch = 1;
        pl.xlds = 0;
        // one row per wave, up to 16 waves per CU, where x is short (each wave re-reads all of x
        // from L2): Qwen2-7B O 6.68 -> 6.45 us; down (x 37.9 KB, K = 18,944) doubled its L2
        // traffic for x that way (23.3 -> 25.1 us), so it keeps two rows per wave
        if ((a.epilogue == QIE_EPI_RESIDUAL || a.epilogue == QIE_EPI_STORE) && rows <= 16 * (int64_t)cus &&
            a.K <= 4096 && k.rpw1 != 0) {
            rpw = 1;
            n_tasks = rows;
        }
    }
    if (xch == 10 && has_norm) {
        pl.error = PlanError::NormRouted;
        return pl;
    }
    return finish(MT == 1 ? xch : 0);
}

// ------------------------------------------------------------------ launch_geometry
// (grid, threads, dynamic LDS) of a Gemv or Skinny plan on `cus` CUs; resident_blocks: blocks of
// plan.threads() threads and plan.lds_bytes resident per CU (the occupancy query; read only
// where plan.needs_occupancy()).
inline LaunchGeom launch_geometry(const LinearPlan& pl, int cus, int resident_blocks) {
    LaunchGeom g{1, pl.threads(), pl.lds_bytes};
    int64_t grid = 1;
    if (pl.family == LinearFamily::Skinny) {
        // as many blocks as are resident at once (LDS-limited when the M rows are staged)
        grid = std::min<int64_t>(pl.n_tasks, (int64_t)cus * (pl.skinny_bpc > 0 ? pl.skinny_bpc : resident_blocks));
    } else if (pl.block_waves) {
        grid = (pl.n_tasks + pl.block_waves - 1) / pl.block_waves;
    } else if (pl.bpc == -2) {
        // Full-residency grid-stride grid (the SwiGLU default): every CU holds the same number
        // of blocks for the whole launch.  The balanced grid below gives every WAVE the same
        // task count but leaves CUs with 3 and 4 blocks (948 blocks at 4 per CU for Qwen2-7B
        // gate/up): in-graph gate/up 43.0 -> 42.2 us, 358.9 -> 361.5 tok/s (same box, A/B)
        grid = std::min((pl.n_tasks + 3) / 4, (int64_t)cus * resident_blocks);
    } else if (pl.bpc <= 0) {
        // Balanced persistent grid (default): the grid is what fits on the chip at once, and
        // the task count per wave is made (nearly) equal — e.g. gate/up (18,944 tasks) on
        // 768 resident blocks: 7 rounds over 677 blocks instead of 4.6 rounds over 1024
        // blocks, whose last 0.6 round ran the chip at 60 % of its waves.
        const int64_t cap = (int64_t)cus * resident_blocks;
        const int64_t rounds = (pl.n_tasks + 4 * cap - 1) / (4 * cap);
        grid = (pl.n_tasks + 4 * rounds - 1) / (4 * rounds);
    } else {
        grid = std::min((pl.n_tasks + 3) / 4, (int64_t)cus * pl.bpc);
    }
    g.grid = (unsigned)std::max<int64_t>(1, grid);
    return g;
}

}  // namespace qie
