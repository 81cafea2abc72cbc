// rows64_plan.hpp — the launch of a 17..64-row decode projection (QIE_LINEAR_ROWS64,
// k_decode_rows64.hip).  Pure host code (no HIP call), beside plan_linear / plan_gemm:
// plan_rows64() names the instantiation, the work split and the workspace, so the decision can
// be printed and tested without a GPU (tools/plan_dump.cpp, tests/test_rows64_plan_cpu.py).
//
// The work split:
//   * a column tile is 16 output columns; a workgroup of 4 waves owns a column block of 4 tiles
//     (64 columns; SWIGLU: 64 gate + 64 up rows), wave w the block's tile w, for ALL M rows:
//     MT = ceil(M / 16) = 2, 3 or 4 accumulator tiles of 16 rows per weight fragment;
//   * K is walked in chunks of 256 columns (4 MFMA units of 64); the chunk's M x 256 slice of x
//     is staged once per workgroup in LDS (row stride 528 B) and read by its four waves;
//   * K is split over `parts` workgroups per column block so that about two workgroups per CU are
//     resident: parts = min(2 cus / col_blocks, chunks / 2, 16), at least 1; every part walks
//     cpp = ceil(chunks / parts) chunks (parts is then re-derived as ceil(chunks / cpp), so no
//     part is empty; the last one may be short and its last chunk ragged);
//   * parts >= 2: each wave's fp32 partial tiles go to slab [tile][part] and the last arriving
//     part (one ticket per tile) adds them in part order and runs the epilogue.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/qie/qie_ops.h"

namespace qie {

constexpr int kR64Threads = 256, kR64Waves = 4;
constexpr int kR64ChunkK = 256;            // columns of x staged per step
constexpr int kR64RowStride = 528;         // LDS bytes per staged row: 512 + 16 (bank spread)
constexpr int kR64MaxParts = 16;
constexpr int kR64MaxTiles = 2048;         // N <= 32,768: the ticket array
constexpr int64_t kR64SlabTiles = 8192;    // 16 x 16 fp32 tiles x MT the slab holds (x 4 KiB = 32 MiB)

enum class Rows64Error { None, Rows, Flags, Epilogue, Norm, Keys, K64, Shape, Segments, Range };

struct Rows64Plan {
    Rows64Error error = Rows64Error::None;
    int epi = 0;
    int wt = 0;            // 0 bf16, 1 fp8 plain, 2 fp8 16-row tiled
    int mt = 2;            // 16-row accumulator tiles per weight fragment
    int nb = 1;            // weight tiles per column tile (SWIGLU: gate, up)
    int n_tiles = 0, col_blocks = 0;
    int chunks = 0, parts = 1, cpp = 0;
    unsigned grid = 0;
    int threads = kR64Threads;
    size_t lds_bytes = 0;
    size_t ws_bytes = 0;   // slab bytes this launch uses (0: no split)
};

inline const char* rows64_error_text(Rows64Error e) {
    switch (e) {
        case Rows64Error::Rows: return "17 <= M <= 64 rows";
        case Rows64Error::Flags: return "bf16 or fp8 weights only (no MXFP4, fp8-activation or tile-override flags)";
        case Rows64Error::Epilogue: return "STORE, RESIDUAL and SWIGLU epilogues only";
        case Rows64Error::Norm: return "no fused RMSNorm: norm the rows first";
        case Rows64Error::Keys: return "no arg-max keys, fused RoPE or peer push";
        case Rows64Error::K64: return "K % 64 == 0";
        case Rows64Error::Shape: return "N <= 32768, ldx % 8 == 0, K < 2^20";
        case Rows64Error::Segments: return "a segment that another follows is whole 16-row tiles (tiled fp8: every segment)";
        case Rows64Error::Range: return "every weight segment under 2^31 bytes";
        default: return "";
    }
}

// extras: the caller passed a fused RoPE or a peer push (LinearExtras), which this kernel has not
inline Rows64Plan plan_rows64(const qie_linear_args& a, int cus, bool extras = false) {
    Rows64Plan p;
    p.epi = a.epilogue;
    auto err = [&](Rows64Error e) {
        p.error = e;
        return p;
    };
    if (a.M < 17 || a.M > 64) return err(Rows64Error::Rows);
    const int allowed = QIE_LINEAR_ROWS64 | QIE_LINEAR_FP8 | QIE_LINEAR_FP8_T16;
    if ((a.flags & ~allowed) || ((a.flags & QIE_LINEAR_FP8_T16) && !(a.flags & QIE_LINEAR_FP8))) return err(Rows64Error::Flags);
    if (a.epilogue != QIE_EPI_STORE && a.epilogue != QIE_EPI_RESIDUAL && a.epilogue != QIE_EPI_SWIGLU)
        return err(Rows64Error::Epilogue);
    if (a.norm_w) return err(Rows64Error::Norm);
    if (a.argmax_keys || extras) return err(Rows64Error::Keys);
    if (a.K <= 0 || a.K % 64 != 0) return err(Rows64Error::K64);
    if (a.N <= 0 || a.N > (int64_t)kR64MaxTiles * 16 || a.ldx % 8 != 0 || a.K >= (1 << 20)) return err(Rows64Error::Shape);
    const bool sw = a.epilogue == QIE_EPI_SWIGLU;
    const bool fp8 = (a.flags & QIE_LINEAR_FP8) != 0, t16 = (a.flags & QIE_LINEAR_FP8_T16) != 0;
    // column tiles must not straddle segments; the last segment may end in a ragged tile
    if (!sw && ((a.seg_rows[0] % 16 != 0 && (a.seg_rows[1] > 0 || a.seg_rows[2] > 0)) ||
                ((a.seg_rows[0] + a.seg_rows[1]) % 16 != 0 && a.seg_rows[2] > 0)))
        return err(Rows64Error::Segments);
    if (t16 && (sw ? a.N % 16 != 0 : (a.seg_rows[0] % 16 != 0 || a.seg_rows[1] % 16 != 0 || a.seg_rows[2] % 16 != 0)))
        return err(Rows64Error::Segments);
    for (int s = 0; s < 3; s++) {
        const int64_t rows = sw ? a.N : a.seg_rows[s];
        if (rows * (fp8 ? a.K + 4 : 2 * a.K) >= (int64_t)1 << 31) return err(Rows64Error::Range);
    }
    p.wt = t16 ? 2 : (fp8 ? 1 : 0);
    p.mt = (int)((a.M + 15) / 16);
    p.nb = sw ? 2 : 1;
    p.n_tiles = (int)((a.N + 15) / 16);
    p.col_blocks = (p.n_tiles + kR64Waves - 1) / kR64Waves;
    p.chunks = (int)((a.K + kR64ChunkK - 1) / kR64ChunkK);
    int parts = std::min(std::min(2 * cus / p.col_blocks, p.chunks / 2), kR64MaxParts);
    // the slab holds kR64SlabTiles tiles of MT x 16 rows
    parts = (int)std::min<int64_t>(parts, kR64SlabTiles / ((int64_t)p.n_tiles * p.nb));
    parts = std::max(parts, 1);
    p.cpp = (p.chunks + parts - 1) / parts;
    p.parts = (p.chunks + p.cpp - 1) / p.cpp;
    p.grid = (unsigned)(p.col_blocks * p.parts);
    p.lds_bytes = (size_t)p.mt * 16 * kR64RowStride;
    p.ws_bytes = p.parts >= 2 ? (size_t)p.n_tiles * p.parts * p.nb * p.mt * 1024 : 0;
    return p;
}

}  // namespace qie
