// gemm_plan.hpp — which prefill GEMM kernel, on which tiles, parts and grid, a linear layer
// launches once qie_linear hands it to gemm() (M > 16, 9..16 rows no skinny kernel takes, and
// every M with fp8 activations).  Pure host code (no HIP call), the M > 16 half of
// linear_plan.hpp: plan_gemm() names every choice that k_gemm.hip's gemm() then only executes,
// so the decision can be printed and tested without a GPU (tools/plan_dump.cpp,
// tests/test_gemm_plan_cpu.py).  The comments that record measured A/B results sit beside the
// decision they explain.  gemm() validates the arguments before it plans.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/qie/qie_ops.h"

namespace qie {

// Every A/B knob of the prefill GEMM launch choice, with the shipped defaults.  The development
// build fills it from the environment (k_gemm.hip dev_gemm_knobs(), one place).
struct GemmKnobs {
    int gemm_big = -1;       // QIE_GEMM_BIG: 1 / 2 force the 256x256 / 256x128 LDS-DMA tile, 0 disables both
    int gemm8 = 2;           // QIE_GEMM8: 2 + split-K; 1 full-chip grids only; 0 off; 3 stream-K
    int sk_grid = 0;         // QIE_GEMM8_SK_GRID: stream-K workgroups (0: one per CU)
    int sk_mink = 64;        // QIE_GEMM8_SK_MINK: k-tiles a bf16 split-K part keeps at least (>= 4)
    int mx_splitk_max = 4;   // QIE_MX_SPLITK_MAX: most parts of an fp8-activation split-K
};

enum class GemmFamily {
    Generic,       // gemm_kernel<EPI, 0>: 128x128 tiles, any K % 8 == 0
    GenericFp8,    // gemm_kernel<EPI, 1>: fp8 weights decoded to bf16 on the way into LDS
    Big256,        // gemm_big_kernel<EPI, 256>
    Big128,        // gemm_big_kernel<EPI, 128>
    Gemm8,         // gemm8_kernel<EPI>, splitk parts per tile
    Gemm8StreamK,  // gemm8sk_kernel<EPI>
    Mx,            // gemm8mx_kernel<EPI, false>: fp8 activations, plain fp8 weights
    MxT16,         // gemm8mx_kernel<EPI, true>: 16-row tiled fp8 weights
};

struct GemmPlan {
    GemmFamily family = GemmFamily::Generic;
    int n_mt = 0;        // row tiles (the tiled kernels walk tile = nt * n_mt + mt)
    int tiles = 0;       // block tiles
    int splitk = 1;      // Gemm8 / Mx: parts per tile
    int dp_rounds = 0;   // stream-K: whole-tile rounds
    int chunk = 0;       // stream-K: k-tile units per range
    unsigned grid_x = 1, grid_y = 1;
    int threads = 256;
    size_t lds_bytes = 0;
    // split-K / stream-K workspace: fp32 slabs of one 256x256 tile, tickets (0: none needed)
    int slabs = 0, tickets = 0;
};

constexpr int kGemmTileLds = 2 * (256 + 256) * 64 * 2;   // gemm8 family: two 64-KB k-tile buffers

// parts per tile: the fewest rounds of (tile, part) items over the CUs, in units of a tile
// (112 tiles: 2 parts = one round of half tiles; 144 tiles: 3 parts, two rounds of thirds),
// among 1..max_parts parts of at least min_k_tiles k-tiles each; the fewest parts on a tie.
inline int split_parts(int64_t tiles, int64_t cus, int nk, int min_k_tiles, int max_parts) {
    int best = 1;
    double best_t = 1e30;
    for (int s = 1; s <= max_parts && nk / s >= min_k_tiles; s++) {
        const double t = (double)((tiles * s + cus - 1) / cus) / s;
        if (t < best_t - 1e-9) {
            best_t = t;
            best = s;
        }
    }
    return best;
}

// allow_split = false: the split-K / stream-K workspace cannot be had (it would have to grow
// during a graph capture); plan what needs none.
inline GemmPlan plan_gemm(const qie_linear_args& a, const GemmKnobs& k, int cus_, bool allow_split = true) {
    GemmPlan pl;
    const int64_t cus = cus_;
    const auto cdiv = [](int64_t x, int64_t y) { return (x + y - 1) / y; };
    const bool sw = a.epilogue == QIE_EPI_SWIGLU;
    const int64_t cols = sw ? 2 * a.N : a.N;   // weight rows = tile columns (gate and up interleaved)
    const int64_t n_mt = cdiv(a.M, 256);
    const int64_t t256 = n_mt * cdiv(cols, 256), t128 = n_mt * cdiv(cols, 128);
    auto tiled = [&](GemmFamily f, int64_t tiles, int64_t grid, size_t lds) {
        pl.family = f;
        pl.n_mt = (int)n_mt;
        pl.tiles = (int)tiles;
        pl.grid_x = (unsigned)grid;
        pl.threads = 512;
        pl.lds_bytes = lds;
        return pl;
    };
    auto split = [&](int parts) {   // `parts` slabs and one ticket per tile
        pl.splitk = parts;
        pl.slabs = (int)t256 * parts;
        pl.tickets = (int)t256;
    };

    // QIE_LINEAR_ACT_FP8 (qie_ops.h): every M, one 256x256 kernel; split-K where the tiles do not
    // fill the chip once (the fewest rounds of (tile, part) items; parts of >= 8 k-tiles)
    if (a.flags & QIE_LINEAR_ACT_FP8) {
        // split only below half the chip (r05, same box, 2,048 rows): O (112 tiles) 91.0 unsplit
        // vs 78.0 split 3, down (112) 307 vs 188; QKV (144 tiles) 69.4 unsplit vs 93.9 split 3
        if (allow_split && 2 * t256 <= cus) {
            const int s = split_parts(t256, cus, (int)(a.K / 128), 8, k.mx_splitk_max);
            if (s > 1) split(s);
        }
        return tiled((a.flags & QIE_LINEAR_FP8_T16) ? GemmFamily::MxT16 : GemmFamily::Mx, t256, t256 * pl.splitk,
                     kGemmTileLds);
    }

    if (!(a.flags & QIE_LINEAR_FP8) && a.K % 32 == 0 && a.ldx % 8 == 0) {
        // LDS-DMA kernels: 256x256 tiles when they fill the chip at least once (config 4's
        // O / down at 8,192 rows: 448 tiles; the generic 128x128 kernel took them before), else
        // 256x128 when those fill >= 3/4 of it in one round (Qwen2-7B O and down projections
        // at 2,048 rows: 112 vs 224 tiles on 256 CUs), else 256x256 in one round (below).
        // args.flags QIE_LINEAR_TILE256 / TILE128 force a tile (tests; dev builds also
        // QIE_GEMM_BIG = 1 / 2, 0 disables the kernel for A/B timing).
        const int force = (a.flags & QIE_LINEAR_TILE256) ? 1 : (a.flags & QIE_LINEAR_TILE128) ? 2 : k.gemm_big;
        const bool by_count = force < 0 && a.M >= 256;   // nothing forced: the tile counts decide
        // phase-interleaved 256x256 kernel (K a multiple of 64, >= 4 k-tiles): Qwen2-7B gate/up at 2,048
        // rows 612 -> 488 us, bit-identical to gemm_big; down split-K 2: 309 -> 247 us
        const bool g8ok = a.K % 64 == 0 && a.K >= 4 * 64;
        const int nk = (int)(a.K / 64);
        // stream-K (QIE_GEMM8 = 3; args.flags QIE_LINEAR_STREAMK): any tile count, one workgroup per CU.
        // The first dp_rounds * grid tiles go whole; the k-tile units of the rest are cut into
        // `grid` ranges of `chunk` (workspace: slab [grid][2], tickets [tiles]).
        if (g8ok && ((a.flags & QIE_LINEAR_STREAMK) || (k.gemm8 == 3 && by_count))) {
            const int64_t grid = k.sk_grid > 0 ? k.sk_grid : cus;
            const int64_t dp = t256 / grid, rest = (t256 - dp * grid) * nk;
            if (rest == 0 || allow_split) {
                pl.dp_rounds = (int)dp;
                pl.chunk = (int)std::max<int64_t>(1, (rest + grid - 1) / grid);
                if (rest > 0) {
                    pl.slabs = 2 * (int)grid;
                    pl.tickets = (int)t256;
                }
                return tiled(GemmFamily::Gemm8StreamK, t256, grid, kGemmTileLds);
            }
        }
        if (g8ok && k.gemm8 != 0 && force != 2 && (force == 1 || (by_count && t256 >= cus)))
            return tiled(GemmFamily::Gemm8, t256, t256, kGemmTileLds);
        if (g8ok && k.gemm8 == 2 && by_count && t256 < cus) {
            // (short parts lose: QKV at 3 x 19 and O at 2 x 28 k-tiles measured 108 -> 112 and
            // 71 -> 69 us, the last arriver's serial slab read and the per-part pipeline fill eat
            // the gain; down at 2 x 148: 309 -> 247 us), so a part keeps >= 64 k-tiles
            // (QIE_GEMM8_SK_MINK, dev A/B; K >= 4,096 per part).  Round 5: split-K 2 for the O
            // projection at P = 2,048 (112 tiles -> 224, K = 3,584) ran 94-98 vs 84 µs for the
            // 256x128 kernel; QKV at 3 parts 114 vs 89 — the slab round trip costs more than the
            // idle CUs at this K
            const int s = split_parts(t256, cus, nk, std::max(4, k.sk_mink), 4);
            // unsplit, 256x256 tiles must still cover half the chip: QKV at 144 tiles 101.7 ->
            // 87.8 us, but O at 112 tiles 78 -> 103 us (its 256x128 kernel fills 224 CUs)
            if (s == 1 && 2 * t256 >= cus) return tiled(GemmFamily::Gemm8, t256, t256, kGemmTileLds);
            if (s > 1 && allow_split) {
                split(s);
                return tiled(GemmFamily::Gemm8, t256, t256 * s, kGemmTileLds);
            }
        }
        constexpr size_t big256 = 4 * (size_t)(256 + 256) * 32 * 2, big128 = 4 * (size_t)(256 + 128) * 32 * 2;
        if (force == 1 || (by_count && t256 >= cus)) return tiled(GemmFamily::Big256, t256, t256, big256);
        if (force == 2 || (by_count && t128 >= (3 * cus) / 4 && t128 <= cus))
            return tiled(GemmFamily::Big128, t128, t128, big128);
        // 256-column tiles in ONE round when 128-column ones would take two (Qwen2-7B QKV at
        // 2,048 rows: 144 vs 288 tiles on 256 CUs): 124 -> 99 us against the generic kernel
        if (by_count && t256 >= cus / 2 && t256 <= cus && t128 > cus) return tiled(GemmFamily::Big256, t256, t256, big256);
    }
    // generic 128x128 kernel, blockIdx.x over row tiles; SwiGLU: 64 outputs per tile
    pl.family = (a.flags & QIE_LINEAR_FP8) ? GemmFamily::GenericFp8 : GemmFamily::Generic;
    pl.n_mt = (int)cdiv(a.M, 128);
    pl.grid_x = (unsigned)pl.n_mt;
    pl.grid_y = (unsigned)cdiv(a.N, sw ? 64 : 128);
    pl.tiles = (int)(pl.grid_x * pl.grid_y);
    pl.threads = 256;
    pl.lds_bytes = (size_t)2 * (128 + 128) * 64 * 2;
    return pl;
}

}  // namespace qie
