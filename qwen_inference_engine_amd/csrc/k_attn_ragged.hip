// k_attn_ragged.hip — the split-context MFMA attention of k_attn_extend.hip over row segments
// of any lengths: up to QIE_RAGGED_MAX_SEGS runs of rows, each with its own cache sequence.
// The segment table travels by value in the kernel arguments (no device table): grid x is the
// sum of the segments' block counts, and a workgroup finds its segment by comparing its index
// with the at most 8 prefix sums — wave-uniform, on scalars.  From there on a workgroup is
// attn_extend_block (attn_extend_block.hpp) on the segment's rows, and the partial layout, the
// split length and the merge are qie_attention_extend's at M = the total row count.
#include "qie_common.hpp"
#include "../../include/qie/qie_ops.h"
#include "attn_extend_block.hpp"

namespace qie {

struct RaggedAttnParams {
    ExtendAttnParams a;                       // rows_per_seq unused
    qie_row_segs segs;
    int32_t blk0[QIE_RAGGED_MAX_SEGS + 1];    // prefix sums of the segments' block counts
};

// Grid (blk0[n], splits, nkv), 256 threads
template <int HD, bool PG>
__global__ __launch_bounds__(256, 2) void attn_ragged_kernel(RaggedAttnParams p) {
    const int bx = blockIdx.x;
    // constant indices only: the table stays in scalar registers
    int row0 = 0, row1 = p.segs.row0[1], seq = p.segs.seq[0], b0 = 0;
#pragma unroll
    for (int z = 1; z < QIE_RAGGED_MAX_SEGS; z++)
        if (z < p.segs.n && bx >= p.blk0[z]) {
            row0 = p.segs.row0[z];
            row1 = p.segs.row0[z + 1];
            seq = p.segs.seq[z];
            b0 = p.blk0[z];
        }
    attn_extend_block<HD, PG>(p.a, seq, row0, row1 - row0, bx - b0, blockIdx.y, blockIdx.z);
}

}  // namespace qie

using namespace qie;

extern "C" {

int qie_attention_ragged(const void* q, const int32_t* pos, const qie_row_segs* segs, const qie_kv_cache* cache,
                         int32_t layer, int32_t n_heads, void* out, void* ws, void* stream) {
    QIE_REQUIRE(q && pos && segs && cache && cache->k && cache->v && out && n_heads > 0,
                "qie_attention_ragged: bad arguments");
    QIE_REQUIRE(segs->n >= 1 && segs->n <= QIE_RAGGED_MAX_SEGS && row_segs_ok(segs, segs->row0[segs->n]),
                "qie_attention_ragged: malformed segment table (1 .. %d segments, row0 strictly increasing from 0, "
                "distinct sequences)", QIE_RAGGED_MAX_SEGS);
    QIE_REQUIRE(cache->head_dim == 64 || cache->head_dim == 128,
                "qie_attention_ragged: head_dim must be 64 or 128 (got %d)", cache->head_dim);
    QIE_REQUIRE(cache->n_kv_heads > 0 && n_heads % cache->n_kv_heads == 0 &&
                    n_heads / cache->n_kv_heads <= kMaxGroup,
                "qie_attention_ragged: n_heads/n_kv_heads must be an integer <= %d", kMaxGroup);
    QIE_REQUIRE(layer >= 0 && layer < cache->n_layers, "qie_attention_ragged: bad layer");
    const int64_t M = segs->row0[segs->n];
    RaggedAttnParams p;
    ExtendAttnParams& a = p.a;
    a.q = (const uint16_t*)q;
    a.pos = pos;
    a.rows_per_seq = 0;
    a.M = M;
    a.kc = (const uint16_t*)cache->k;
    a.vc = (const uint16_t*)cache->v;
    QIE_TRY(kv_map_make(cache, &a.km, "qie_attention_ragged"));
    a.layer = layer;
    a.nkv = cache->n_kv_heads;
    a.nq = n_heads;
    // qie_attention_extend's split of a call of M rows
    a.split_len = qie_attention_extend_split_tokens(M, cache->max_ctx);
    a.nsplit = std::max(1, (cache->max_ctx + a.split_len - 1) / a.split_len);
    QIE_REQUIRE(a.nsplit == 1 || ws, "qie_attention_ragged: workspace required");
    const int64_t part = M * n_heads * (int64_t)a.nsplit;
    a.part_o = (float*)ws;
    a.part_ml = ws ? (float*)ws + part * cache->head_dim : nullptr;
    a.out = (uint16_t*)out;
    p.segs = *segs;
    const int G = n_heads / cache->n_kv_heads;
    int64_t nblk = 0;
    for (int z = 0; z <= QIE_RAGGED_MAX_SEGS; z++) {
        p.blk0[z] = (int32_t)nblk;
        if (z < segs->n)
            nblk += ((int64_t)(segs->row0[z + 1] - segs->row0[z]) * G + kExtBlockRows - 1) / kExtBlockRows;
    }
    QIE_REQUIRE(a.nkv <= 65535 && a.nsplit <= 65535 && nblk <= INT32_MAX,
                "qie_attention_ragged: %lld row blocks x %d kv heads exceed the launch grid", (long long)nblk, a.nkv);
    hipStream_t st = (hipStream_t)stream;
    const size_t shm = (size_t)2 * 2 * 64 * cache->head_dim * 2;
    const bool pg = a.km.table != nullptr;
    dim3 grid((unsigned)nblk, (unsigned)a.nsplit, (unsigned)a.nkv);
    auto k = cache->head_dim == 128 ? (pg ? attn_ragged_kernel<128, true> : attn_ragged_kernel<128, false>)
                                    : (pg ? attn_ragged_kernel<64, true> : attn_ragged_kernel<64, false>);
    hipLaunchKernelGGL(k, grid, dim3(256), shm, st, p);
    QIE_LAUNCH_CHECK();
    if (a.nsplit > 1) {
        launch_attn_combine<true>(cache->head_dim, M, n_heads, a.nsplit, a.part_o, a.part_ml, a.out, st);
        QIE_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
