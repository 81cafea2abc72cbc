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
// One workgroup's work is attn_extend_block (attn_extend_block.hpp), shared with the ragged
// form (k_attn_ragged.hip).
// Arithmetic, LDS images (LDS-DMA staging, XOR chunk swizzles, ds_read_b64_tr_b16 V reads)
// and the per-tile softmax are attn_mfma_walk (attn_mfma_tile.hpp), the walk
// attn_prefill_mfma2_kernel runs from key 0; that header documents the operand layouts.
#include "qie_common.hpp"
#include "../../include/qie/qie_ops.h"
#include "attn_extend_block.hpp"

namespace qie {

constexpr int kExtSplitLong = 512;    // keys per split
constexpr int kExtSplitShort = 256;   // ... for calls of <= kExtShortRows rows (more workgroups)
constexpr int kExtShortRows = 32;
constexpr int kExtMaxSplits = 64;     // longer contexts take longer splits

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

// Grid (row blocks, splits, n_seqs * nkv), 256 threads: sequence z owns rows
// [z * rows_per_seq, (z + 1) * rows_per_seq) of the call; the workgroup is attn_extend_block.
template <int HD, bool PG>
__global__ __launch_bounds__(256, 2) void attn_extend_kernel(ExtendAttnParams a) {
    const int kvh = blockIdx.z % a.nkv, seq = blockIdx.z / a.nkv;
    const int64_t row0 = (int64_t)seq * a.rows_per_seq;
    const int R = (int)min((int64_t)a.rows_per_seq, a.M - row0);   // a short last sequence
    attn_extend_block<HD, PG>(a, seq, row0, R, blockIdx.x, blockIdx.y, kvh);
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
