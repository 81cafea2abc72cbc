// k_attn_extend.hip — split-context MFMA attention for a block of new rows over a cached
// prefix (gfx950): flash-decoding generalised from one query row to a tile of rows.
//
// qie_attention has no good form for "a few new rows over a long context": its prefill
// kernel gives one workgroup per (16 row groups, q head) that walks the WHOLE context
// serially (128 rows over 8k keys on Qwen2-7B heads: 28 workgroups on 256 CUs, K/V fetched
// once per q head), its split kernel is VALU with one workgroup per row.  Here:
//   * the query rows of one kv head are the flattened (token, head-in-group) pairs
//     f = token * G + head, packed into 16-row MFMA groups (tail padded by clamping): GQA's
//     G heads share every K/V byte, and a handful of tokens still fills the MFMA tile;
//   * a workgroup is one (sequence, kv head, key split, row block): 4 waves x 2 groups =
//     128 flattened rows per block, each staged 64-key K/V tile serves all 8 groups;
//   * the context is cut into splits of a fixed key count (kExtSplitLong / kExtSplitShort
//     keys, a power of two: whole pages or inside one page, see extend_split; each 64-key
//     tile looks its own page up);
//   * every workgroup leaves fp32 partials (O, running max, sum) in the workspace and a
//     second, ordinary launch merges them — no hand-off inside a launch.
// Arithmetic, LDS images (LDS-DMA staging, XOR chunk swizzles, ds_read_b64_tr_b16 V reads)
// and the per-tile softmax are attn_mfma_walk (attn_mfma_tile.hpp), the walk
// attn_prefill_mfma2_kernel runs from key 0; that header documents the operand layouts.
#include "qie_common.hpp"
#include "../../include/qie/qie_ops.h"
#include "attn_mfma_tile.hpp"

namespace qie {

constexpr int kExtSplitLong = 512;    // keys per split
constexpr int kExtSplitShort = 256;   // ... for calls of <= kExtShortRows rows (more workgroups)
constexpr int kExtShortRows = 32;
constexpr int kExtMaxSplits = 64;     // longer contexts take longer splits
constexpr int kExtBlockRows = 128;    // flattened rows per workgroup (4 waves x 2 groups x 16)

// split length and count for a call of M rows on a max_ctx-key cache; a function of
// (M, max_ctx) only, so the workspace can be sized before the call.  The length is a power of
// two >= 256 and pages are powers of two >= 128 tokens: a split is either a whole number of
// pages or lies inside one page, never part of a page and part of the next.
static void extend_split(int64_t M, int32_t max_ctx, int* len, int* count) {
    int L = M <= kExtShortRows ? kExtSplitShort : kExtSplitLong;
    int n = (max_ctx + L - 1) / L;
    while (n > kExtMaxSplits) {
        L *= 2;
        n = (max_ctx + L - 1) / L;
    }
    *len = L;
    *count = n < 1 ? 1 : n;
}

struct ExtendAttnParams {
    const uint16_t* q;       // [M][nq*HD]
    const int32_t* pos;      // [M]; non-decreasing within each sequence's rows
    int rows_per_seq;
    int64_t M;
    const uint16_t* kc;
    const uint16_t* vc;
    KvMap km;
    int layer, nkv, nq;
    int nsplit, split_len;
    float* part_o;    // [M][nq][nsplit][HD]; merged by attn_combine_kernel<HD, true>
    float* part_ml;   // [M][nq][nsplit][2]: running max (log2 domain), sum
    uint16_t* out;    // [M][nq*HD]
};

// Grid (row blocks, splits, n_seqs * nkv), 256 threads.  Wave w owns the block's 16-row
// groups (w, 7 - w): positions are non-decreasing in the flattened row index, so the pair
// evens out the rows' own causal triangle as in the prefill kernel; the rectangle over the
// prefix is the same for every group.
template <int HD, bool PG>
__global__ __launch_bounds__(256, 2) void attn_extend_kernel(ExtendAttnParams a) {
    constexpr int NW = 4;
    constexpr int KT = 64;
    constexpr int KSTEPS = HD / 32;
    constexpr int DT = HD / 16;
    constexpr int QG = 2;                  // 16-row query groups per wave
    constexpr int NGB = QG * NW;           // groups per block
    static_assert(16 * NGB == kExtBlockRows, "attn_extend: block rows");

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int s = blockIdx.y;
    const int kvh = blockIdx.z % a.nkv, seq = blockIdx.z / a.nkv;
    const int G = a.nq / a.nkv;
    const int64_t row0 = (int64_t)seq * a.rows_per_seq;
    const int R = (int)min((int64_t)a.rows_per_seq, a.M - row0);   // a short last sequence
    const int RG = R * G;                                         // flattened rows of this kv head
    const int f0 = blockIdx.x * kExtBlockRows;
    if (f0 >= RG) return;
    // flattened row f = token f / G, head kvh * G + f % G
    const int64_t ns = a.nsplit;
    auto part_idx = [&](int f) { return ((row0 + f / G) * a.nq + kvh * G + f % G) * ns + s; };

    // the block's last position bounds the keys any of its rows can see
    const int kmax = __builtin_amdgcn_readfirstlane(a.pos[row0 + (min(f0 + kExtBlockRows, RG) - 1) / G]);
    const int k0 = s * a.split_len;
    if (k0 > kmax) {
        // no row of the block sees this split: (-inf, 0) in every slot the combine reads (it
        // skips the O of such a slot); splits >= 1 only, so partials exist
        if (tid < kExtBlockRows && f0 + tid < RG) {
            const int64_t pi = part_idx(f0 + tid);
            a.part_ml[pi * 2] = -INFINITY;
            a.part_ml[pi * 2 + 1] = 0.f;
        }
        return;
    }
    const int nkt = min((k0 + a.split_len) / KT, kmax / KT + 1);   // tiles [k0 / KT, nkt); past kmax: not loaded

    const int64_t head_off = kv_run_off(a.km, (int64_t)a.layer * a.nkv + kvh, HD);
    const uint16_t* kb = a.kc + head_off;
    const uint16_t* vb = a.vc + head_off;

    const int grp[QG] = {wave, NGB - 1 - wave};
    bool gact[QG];
    int qpos[QG], gpos[QG], gmin[QG];
    bf16x8_t qf[QG][KSTEPS];
#pragma unroll
    for (int q = 0; q < QG; q++) {
        gact[q] = f0 + 16 * grp[q] < RG;
        const int fb = gact[q] ? f0 + 16 * grp[q] : f0;
        const int f = min(fb + fr, RG - 1);                 // padded rows repeat the last one
        const int t = f / G, hq = f - t * G;
        qpos[q] = a.pos[row0 + t];
        gpos[q] = __builtin_amdgcn_readfirstlane(gact[q] ? a.pos[row0 + min(fb + 15, RG - 1) / G] : -1);   // -1: no tile
        // the group's first position: a key tile ending at or before it needs no causal mask
        gmin[q] = __builtin_amdgcn_readfirstlane(a.pos[row0 + fb / G]);
        const uint16_t* qp = a.q + (row0 + t) * (int64_t)a.nq * HD + (int64_t)(kvh * G + hq) * HD;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) qf[q][ks] = *reinterpret_cast<const bf16x8_t*>(qp + ks * 32 + g * 8);
    }

    f32x4_t oacc[QG][DT];
    float m_run[QG], l_run[QG];
    attn_mfma_walk<HD, PG, NW, true>(kb, vb, a.km, seq, kmax, k0, nkt, qf, qpos, gpos, gmin, oacc, m_run, l_run);

    // every real row of the block leaves its slot, also the rows this split showed no key
    // ((-inf, 0) and a zero O): the workspace is never assumed initialised
#pragma unroll
    for (int q = 0; q < QG; q++) {
        if (!gact[q]) continue;
        const int fb = f0 + 16 * grp[q];
        if (a.nsplit == 1) {
            float lr[4];
#pragma unroll
            for (int r = 0; r < 4; r++) lr[r] = __shfl(l_run[q], g * 4 + r, 64);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int f = fb + g * 4 + r;
                if (f >= RG) continue;
                uint16_t* orow = a.out + (row0 + f / G) * (int64_t)a.nq * HD + (int64_t)(kvh * G + f % G) * HD;
#pragma unroll
                for (int d = 0; d < DT; d++) orow[16 * d + fr] = f2bf(oacc[q][d][r] / lr[r]);
            }
            continue;
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int f = fb + g * 4 + r;
            if (f >= RG) continue;
            float* prow = a.part_o + part_idx(f) * HD;
#pragma unroll
            for (int d = 0; d < DT; d++) prow[16 * d + fr] = oacc[q][d][r];
        }
        if (g == 0 && fb + fr < RG) {   // lanes of equal fr hold the same row statistics
            const int64_t pi = part_idx(fb + fr);
            a.part_ml[pi * 2] = m_run[q];
            a.part_ml[pi * 2 + 1] = l_run[q];
        }
    }
}

}  // namespace qie

using namespace qie;

extern "C" {

int32_t qie_attention_extend_split_tokens(int64_t M, int32_t max_ctx) {
    int len, count;
    extend_split(M, max_ctx, &len, &count);
    return len;
}

int64_t qie_attention_extend_workspace_bytes(int64_t M, int32_t n_heads, int32_t head_dim, int32_t max_ctx) {
    int len, count;
    extend_split(M, max_ctx, &len, &count);
    if (count == 1) return 0;
    return M * n_heads * (int64_t)count * (head_dim + 2) * 4;
}

int qie_attention_extend(const void* q, int64_t M, const int32_t* pos, int32_t rows_per_seq,
                         const qie_kv_cache* cache, int32_t layer, int32_t n_heads, void* out, void* ws,
                         void* stream) {
    QIE_REQUIRE(q && pos && cache && cache->k && cache->v && out && M >= 0 && rows_per_seq > 0 && n_heads > 0,
                "qie_attention_extend: bad arguments");
    QIE_REQUIRE(cache->head_dim == 64 || cache->head_dim == 128,
                "qie_attention_extend: head_dim must be 64 or 128 (got %d)", cache->head_dim);
    QIE_REQUIRE(cache->n_kv_heads > 0 && n_heads % cache->n_kv_heads == 0 &&
                    n_heads / cache->n_kv_heads <= kMaxGroup,
                "qie_attention_extend: n_heads/n_kv_heads must be an integer <= %d", kMaxGroup);
    QIE_REQUIRE(layer >= 0 && layer < cache->n_layers, "qie_attention_extend: bad layer");
    if (M == 0) return 0;
    ExtendAttnParams a;
    a.q = (const uint16_t*)q;
    a.pos = pos;
    a.rows_per_seq = rows_per_seq;
    a.M = M;
    a.kc = (const uint16_t*)cache->k;
    a.vc = (const uint16_t*)cache->v;
    QIE_TRY(kv_map_make(cache, &a.km, "qie_attention_extend"));
    a.layer = layer;
    a.nkv = cache->n_kv_heads;
    a.nq = n_heads;
    extend_split(M, cache->max_ctx, &a.split_len, &a.nsplit);
    QIE_REQUIRE(a.nsplit == 1 || ws, "qie_attention_extend: workspace required");
    const int64_t part = M * n_heads * (int64_t)a.nsplit;
    a.part_o = (float*)ws;
    a.part_ml = ws ? (float*)ws + part * cache->head_dim : nullptr;
    a.out = (uint16_t*)out;
    const int64_t n_seqs = (M + rows_per_seq - 1) / rows_per_seq;
    const int G = n_heads / cache->n_kv_heads;
    const int64_t nblk = ((int64_t)std::min<int64_t>(rows_per_seq, M) * G + kExtBlockRows - 1) / kExtBlockRows;
    QIE_REQUIRE(n_seqs * a.nkv <= 65535 && nblk <= INT32_MAX && M <= INT32_MAX,
                "qie_attention_extend: %lld sequences x %d kv heads exceed the launch grid", (long long)n_seqs, a.nkv);
    hipStream_t st = (hipStream_t)stream;
    const size_t shm = (size_t)2 * 2 * 64 * cache->head_dim * 2;
    const bool pg = a.km.table != nullptr;
    dim3 grid((unsigned)nblk, (unsigned)a.nsplit, (unsigned)(n_seqs * a.nkv));
    auto k = cache->head_dim == 128 ? (pg ? attn_extend_kernel<128, true> : attn_extend_kernel<128, false>)
                                    : (pg ? attn_extend_kernel<64, true> : attn_extend_kernel<64, false>);
    hipLaunchKernelGGL(k, grid, dim3(256), shm, st, a);
    QIE_LAUNCH_CHECK();
    if (a.nsplit > 1) {
        launch_attn_combine<true>(cache->head_dim, M, n_heads, a.nsplit, a.part_o, a.part_ml, a.out, st);
        QIE_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
