// k_kv_fp8.hip — the fp8 KV cache's operator tier around the decode attention (k_attention.hip
// qie_attention_decode_fp8): the prompt writer (qie_qkv_post_fp8), the exact expander into a bf16
// staging cache (qie_kv_dequantize_fp8) and the copy (qie_kv_copy_fp8).  Format: qie_ops.h
// "fp8 KV cache", device form kv_fp8.hpp.  The reference keeps its cache in bf16 only
// (include_cuda.cu:165-279); nothing here restates a reference kernel.
#include "kv_fp8.hpp"
#include "launch_util.hpp"
#include "qkv_post.hpp"

namespace qie {

int kv8_exps_make(const qie_kv_cache_fp8* c, const KvMap& km, Kv8Exps* out, const char* who) {
    QIE_REQUIRE(c->k_exps && c->v_exps, "%s: fp8 KV cache without exponent arrays", who);
    QIE_REQUIRE(c->c.head_dim == 64 || c->c.head_dim == 128, "%s: fp8 KV cache: head_dim must be 64 or 128 (got %d)",
                who, c->c.head_dim);
    QIE_REQUIRE(c->exp_stride >= (int64_t)c->c.n_layers * c->c.n_kv_heads * km.run,
                "%s: fp8 KV cache: exp_stride %lld < layers x kv heads x %d tokens", who, (long long)c->exp_stride,
                km.run);
    QIE_REQUIRE(c->c.seq_stride % 16 == 0 && ((uintptr_t)c->c.k % 16) == 0 && ((uintptr_t)c->c.v % 16) == 0,
                "%s: fp8 KV cache: codes must be 16-byte aligned with seq_stride %% 16 == 0", who);
    out->ke = (uint8_t*)c->k_exps;
    out->ve = (uint8_t*)c->v_exps;
    out->em = km;
    out->em.stride = c->exp_stride;
    return 0;
}

// ------------------------------------------------------------------ writer
// qkv_post_kernel's block (one per row, a wave per head, a lane per RoPE pair, the heads' source
// pairs loaded in batches) with a second stage for the K and V heads: the wave leaves the head's
// bf16 row in its LDS slot, and the row's hd / 8 lanes take it back 8 elements each — the layout in
// which the amax is a DPP reduction within a 16-lane row, the codes leave as one 8-byte store per
// lane and the staging copy as one 16-byte store.  q heads are stored as the bf16 kernel stores them.
struct QkvPost8 {
    uint8_t* k8;
    uint8_t* v8;
    Kv8Exps ex;
    uint16_t* sk;     // staging cache (contiguous bf16, layer 0), or null
    uint16_t* sv;
    KvMap sm;
};

template <bool PG, bool HF, int HD, class Args>
__global__ __launch_bounds__(256) void qkv_post_fp8_kernel(Args a, QkvPost8 f) {
#pragma clang fp contract(off)
    constexpr int LPT = HD / 8;
    __shared__ __attribute__((aligned(16))) uint16_t row_s[4][HD];
    const int64_t m = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int hd = HD, half = HD / 2;
    const int QD = a.nq * hd, KD = a.nkv * hd;
    const int ptot = a.nq + 2 * a.nkv;
    const int p = a.pos[m];
    const int64_t seq = qkv_row_seq(a, m);
    const uint16_t* row = a.qkv + m * (int64_t)(QD + 2 * KD);
    const bool active = lane < half;
    const int i0 = HF ? lane : 2 * lane;
    const int i1 = HF ? lane + half : 2 * lane + 1;
    const float c = active ? a.cs[(int64_t)p * half + lane] : 0.f;
    const float s = active ? a.sn[(int64_t)p * half + lane] : 0.f;
    const int64_t tok = kv_tok<PG>(a.km, seq, p, hd);                // codes: elements = bytes
    const int64_t stok = f.sk ? kv_tok<false>(f.sm, seq, p, hd) : 0;
    for (int h0 = wave; h0 < ptot; h0 += 4 * kQkvBatch) {
        uint32_t raw[kQkvBatch];   // the lane's pair of head h0 + 4 b: element i0 low, i1 high
#pragma unroll
        for (int b = 0; b < kQkvBatch; b++) {
            const int h = h0 + 4 * b;
            raw[b] = 0;
            if (h < ptot && active) {
                const uint16_t* src = row + h * hd;
                raw[b] = HF ? (uint32_t)src[i0] | ((uint32_t)src[i1] << 16)
                            : reinterpret_cast<const uint32_t*>(src)[lane];
            }
        }
#pragma unroll
        for (int b = 0; b < kQkvBatch; b++) {
            const int h = h0 + 4 * b;
            if (h >= ptot) break;   // wave-uniform
            const bool is_q = h < a.nq, is_k = !is_q && h < a.nq + a.nkv;
            float y0, y1;
            qkv_post_pair<HF>(raw[b], active, is_q || is_k, is_q ? a.q_norm : (is_k ? a.k_norm : nullptr), i0, i1, c, s,
                              hd, a.eps, y0, y1);
            if (is_q) {   // wave-uniform
                uint16_t* dst = a.q_out + m * (int64_t)QD + h * hd;
                if (active) {
                    if (HF) {
                        dst[i0] = f2bf(y0);
                        dst[i1] = f2bf(y1);
                    } else {
                        reinterpret_cast<uint32_t*>(dst)[lane] = pack2(y0, y1);
                    }
                }
                continue;
            }
            if (active) {
                row_s[wave][i0] = f2bf(y0);
                row_s[wave][i1] = f2bf(y1);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const bool own = lane < LPT;
            const uint4 bf8 = own ? *reinterpret_cast<const uint4*>(&row_s[wave][lane * 8]) : make_uint4(0, 0, 0, 0);
            const Kv8Row r = kv8_quantize_row<LPT>(bf8);   // every lane runs the reduction
            const int g = is_k ? h - a.nq : h - a.nq - a.nkv;
            const int64_t lg = (int64_t)a.layer * a.nkv + g;
            if (own) {
                uint8_t* codes = (is_k ? f.k8 : f.v8) + kv_run_off(a.km, lg, hd) + tok;
                *reinterpret_cast<uint2*>(codes + lane * 8) = r.codes;
                if (lane == 0) (is_k ? f.ex.ke : f.ex.ve)[kv8_exp_off<PG>(f.ex.em, lg, seq, p)] = (uint8_t)r.e;
                if (f.sk)
                    *reinterpret_cast<uint4*>((is_k ? f.sk : f.sv) + kv_run_off(f.sm, g, hd) + stok + lane * 8) = r.deq;
            }
            __builtin_amdgcn_wave_barrier();   // the slot is free for the wave's next head
        }
    }
}

// ---------------------------------------------------------------- expander
// One layer's rows [pos0, pos0 + n) of every kv head, K and V: thread = one 8-code unit (8 B in,
// the row's exponent byte, 16 B out); consecutive lanes take consecutive units of a row, so a wave
// reads 512 contiguous code bytes and writes 1 KiB.  grid = (units / 256, kv heads, {K, V}).
struct KvDeq8Args {
    const uint8_t *k8, *v8;
    Kv8Exps ex;
    KvMap sm, dm;
    uint16_t *dk, *dv;
    int sseq, dseq, slayer, dlayer, nkv, pos0, units, hd;
};

template <bool PG>
__global__ __launch_bounds__(256) void kv_dequantize_fp8_kernel(const KvDeq8Args a) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= a.units) return;
    const int cpr = a.hd / 8;
    const int tok = a.pos0 + u / cpr, ch = u % cpr;
    const int g = blockIdx.y;
    const bool isv = blockIdx.z != 0;
    const int64_t slg = (int64_t)a.slayer * a.nkv + g, dlg = (int64_t)a.dlayer * a.nkv + g;
    const uint8_t* src = (isv ? a.v8 : a.k8) + kv_run_off(a.sm, slg, a.hd) + kv_tok<PG>(a.sm, a.sseq, tok, a.hd);
    const uint2 codes = *reinterpret_cast<const uint2*>(src + ch * 8);
    const uint32_t e = (isv ? a.ex.ve : a.ex.ke)[kv8_exp_off<PG>(a.ex.em, slg, a.sseq, tok)];
    uint16_t* dst = (isv ? a.dv : a.dk) + kv_run_off(a.dm, dlg, a.hd) + kv_tok<false>(a.dm, a.dseq, tok, a.hd);
    *reinterpret_cast<uint4*>(dst + ch * 8) = fp8x8_to_bf16x8(codes, kv8_scale(e));
}

// -------------------------------------------------------------------- copy
// qie_kv_copy's stream at one byte per element: thread = one 16-byte unit (16 codes) of the range,
// every (layer, kv head) run on grid y, {K, V} on z.  A run has hd / 16 >= 4 units per row, so its
// first n_rows threads also move one exponent byte each (thread u: row u's) — no second launch.
struct KvCopy8Args {
    const uint8_t *sk, *sv;
    uint8_t *dk, *dv;
    Kv8Exps se, de;
    KvMap sm, dm;
    int sseq, dseq, pos0, units, n_rows, cpr, hd;
};

template <bool PG>
__global__ __launch_bounds__(256) void kv_copy_fp8_kernel(const KvCopy8Args a) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= a.units) return;
    const int64_t lg = blockIdx.y;
    const bool isv = blockIdx.z != 0;
    const int row = u / a.cpr, ch = u % a.cpr;
    const uint8_t* s = (isv ? a.sv : a.sk) + kv_run_off(a.sm, lg, a.hd) + kv_tok<PG>(a.sm, a.sseq, a.pos0 + row, a.hd);
    uint8_t* d = (isv ? a.dv : a.dk) + kv_run_off(a.dm, lg, a.hd) + kv_tok<PG>(a.dm, a.dseq, a.pos0 + row, a.hd);
    const uint4 r = *reinterpret_cast<const uint4*>(s + ch * 16);
    uint8_t e = 0;
    if (u < a.n_rows) e = (isv ? a.se.ve : a.se.ke)[kv8_exp_off<PG>(a.se.em, lg, a.sseq, a.pos0 + u)];
    *reinterpret_cast<uint4*>(d + ch * 16) = r;
    if (u < a.n_rows) (isv ? a.de.ve : a.de.ke)[kv8_exp_off<PG>(a.de.em, lg, a.dseq, a.pos0 + u)] = e;
}

template <class Args>
static int qkv_post_fp8_launch(const char* who, Args& a, const void* qkv, int64_t M, const int32_t* pos,
                               const void* q_norm, const void* k_norm, const float* rope_cos, const float* rope_sin,
                               int32_t n_heads, const qie_kv_cache_fp8* cache, const qie_kv_cache* stage, int32_t layer,
                               float eps, int32_t numerics, void* q_out, void* stream) {
    const qie_kv_cache& c = cache->c;
    a.qkv = (const uint16_t*)qkv;
    a.pos = pos;
    a.q_norm = (const uint16_t*)q_norm;
    a.k_norm = (const uint16_t*)k_norm;
    a.cs = rope_cos;
    a.sn = rope_sin;
    a.nq = n_heads;
    a.nkv = c.n_kv_heads;
    a.hd = c.head_dim;
    a.kc = a.vc = nullptr;   // the bf16 kernel's destinations: not used here
    QIE_TRY(kv_map_make(&c, &a.km, who));
    a.layer = layer;
    a.eps = eps;
    a.numerics = numerics;
    a.q_out = (uint16_t*)q_out;
    QkvPost8 f{};
    f.k8 = (uint8_t*)c.k;
    f.v8 = (uint8_t*)c.v;
    QIE_TRY(kv8_exps_make(cache, a.km, &f.ex, who));
    if (stage) {
        QIE_REQUIRE(!stage->block_table && stage->n_kv_heads == c.n_kv_heads && stage->head_dim == c.head_dim &&
                        stage->max_ctx >= c.max_ctx && ((uintptr_t)stage->k % 16) == 0 && ((uintptr_t)stage->v % 16) == 0 &&
                        stage->seq_stride % 8 == 0,
                    "%s: stage must be a contiguous, 16-byte aligned bf16 cache with the fp8 cache's n_kv_heads and "
                    "head_dim and at least its max_ctx", who);
        QIE_TRY(kv_map_make(stage, &f.sm, who));
        f.sk = (uint16_t*)stage->k;
        f.sv = (uint16_t*)stage->v;
    }
    if (M == 0) return 0;
    const bool hf = numerics == QIE_NUMERICS_HF, pg = a.km.table != nullptr;
    void (*fn)(Args, QkvPost8);
    if (c.head_dim == 128)
        fn = pg ? (hf ? qkv_post_fp8_kernel<true, true, 128, Args> : qkv_post_fp8_kernel<true, false, 128, Args>)
                : (hf ? qkv_post_fp8_kernel<false, true, 128, Args> : qkv_post_fp8_kernel<false, false, 128, Args>);
    else
        fn = pg ? (hf ? qkv_post_fp8_kernel<true, true, 64, Args> : qkv_post_fp8_kernel<true, false, 64, Args>)
                : (hf ? qkv_post_fp8_kernel<false, true, 64, Args> : qkv_post_fp8_kernel<false, false, 64, Args>);
    hipLaunchKernelGGL(fn, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, a, f);
    QIE_LAUNCH_CHECK();
    return 0;
}

}  // namespace qie

using namespace qie;

extern "C" {

int qie_qkv_post_fp8(const void* qkv, int64_t M, const int32_t* pos, int32_t rows_per_seq, const qie_row_segs* segs,
                     const void* q_norm, const void* k_norm, const float* rope_cos, const float* rope_sin,
                     int32_t n_heads, const qie_kv_cache_fp8* cache, const qie_kv_cache* stage, int32_t layer, float eps,
                     int32_t numerics, void* q_out, void* stream) {
    QIE_REQUIRE(qkv && pos && cache && cache->c.k && cache->c.v && rope_cos && rope_sin && q_out && M >= 0 &&
                    M <= INT32_MAX && (segs || rows_per_seq > 0) && n_heads > 0 && cache->c.n_kv_heads > 0 &&
                    n_heads % cache->c.n_kv_heads == 0 && layer >= 0 && layer < cache->c.n_layers,
                "qie_qkv_post_fp8: bad arguments");
    if (segs) {
        QIE_REQUIRE(row_segs_ok(segs, M), "qie_qkv_post_fp8: malformed segment table (1 .. %d segments, row0 strictly "
                    "increasing from 0 to M = %lld, distinct sequences)", QIE_RAGGED_MAX_SEGS, (long long)M);
        QkvPostRaggedArgs a;
        a.rows_per_seq = 0;
        a.segs = *segs;
        return qkv_post_fp8_launch("qie_qkv_post_fp8", a, qkv, M, pos, q_norm, k_norm, rope_cos, rope_sin, n_heads,
                                   cache, stage, layer, eps, numerics, q_out, stream);
    }
    QkvPostArgs a;
    a.rows_per_seq = rows_per_seq;
    return qkv_post_fp8_launch("qie_qkv_post_fp8", a, qkv, M, pos, q_norm, k_norm, rope_cos, rope_sin, n_heads, cache,
                               stage, layer, eps, numerics, q_out, stream);
}

int qie_kv_dequantize_fp8(const qie_kv_cache_fp8* src, int32_t src_seq, int32_t layer, int32_t pos0, int32_t n_rows,
                          const qie_kv_cache* dst, int32_t dst_seq, int32_t dst_layer, void* stream) {
    QIE_REQUIRE(src && dst && src_seq >= 0 && dst_seq >= 0 && pos0 >= 0 && n_rows >= 0 && layer >= 0 &&
                    layer < src->c.n_layers && dst_layer >= 0 && dst_layer < dst->n_layers,
                "qie_kv_dequantize_fp8: bad arguments");
    KvDeq8Args a{};
    QIE_TRY(kv_map_make(&src->c, &a.sm, "qie_kv_dequantize_fp8"));
    QIE_TRY(kv_map_make(dst, &a.dm, "qie_kv_dequantize_fp8"));
    QIE_TRY(kv8_exps_make(src, a.sm, &a.ex, "qie_kv_dequantize_fp8"));
    QIE_REQUIRE(!dst->block_table && dst->n_kv_heads == src->c.n_kv_heads && dst->head_dim == src->c.head_dim &&
                    ((uintptr_t)dst->k % 16) == 0 && ((uintptr_t)dst->v % 16) == 0 && dst->seq_stride % 8 == 0,
                "qie_kv_dequantize_fp8: dst must be a contiguous, 16-byte aligned bf16 cache with the source's "
                "n_kv_heads and head_dim");
    QIE_REQUIRE((int64_t)pos0 + n_rows <= src->c.max_ctx && (int64_t)pos0 + n_rows <= dst->max_ctx,
                "qie_kv_dequantize_fp8: positions %d..%lld exceed max_ctx %d / %d", pos0, (long long)pos0 + n_rows - 1,
                src->c.max_ctx, dst->max_ctx);
    if (n_rows == 0) return 0;
    const int hd = src->c.head_dim;
    const int64_t units = (int64_t)n_rows * (hd / 8);
    QIE_REQUIRE(src->c.n_kv_heads <= 65535 && units <= INT32_MAX / 2, "qie_kv_dequantize_fp8: %lld units", (long long)units);
    a.k8 = (const uint8_t*)src->c.k;
    a.v8 = (const uint8_t*)src->c.v;
    a.dk = (uint16_t*)dst->k;
    a.dv = (uint16_t*)dst->v;
    a.sseq = src_seq; a.dseq = dst_seq; a.slayer = layer; a.dlayer = dst_layer;
    a.nkv = src->c.n_kv_heads; a.pos0 = pos0; a.units = (int)units; a.hd = hd;
    const dim3 grid((unsigned)((units + 255) / 256), (unsigned)a.nkv, 2);
    hipLaunchKernelGGL((a.sm.table ? kv_dequantize_fp8_kernel<true> : kv_dequantize_fp8_kernel<false>), grid, dim3(256), 0,
                       (hipStream_t)stream, a);
    QIE_LAUNCH_CHECK();
    return 0;
}

int qie_kv_copy_fp8(const qie_kv_cache_fp8* src, int32_t src_seq, const qie_kv_cache_fp8* dst, int32_t dst_seq,
                    int32_t pos0, int32_t n_rows, void* stream) {
    QIE_REQUIRE(src && dst && src_seq >= 0 && dst_seq >= 0 && pos0 >= 0 && n_rows >= 0, "qie_kv_copy_fp8: bad arguments");
    const qie_kv_cache &s = src->c, &d = dst->c;
    QIE_REQUIRE(!s.block_table == !d.block_table, "qie_kv_copy_fp8: one cache is paged, the other contiguous");
    QIE_REQUIRE(s.n_layers == d.n_layers && s.n_kv_heads == d.n_kv_heads && s.head_dim == d.head_dim &&
                    (!s.block_table || s.page_tokens == d.page_tokens),
                "qie_kv_copy_fp8: the caches differ in n_layers, n_kv_heads, head_dim or page_tokens");
    KvCopy8Args a{};
    QIE_TRY(kv_map_make(&s, &a.sm, "qie_kv_copy_fp8"));
    QIE_TRY(kv_map_make(&d, &a.dm, "qie_kv_copy_fp8"));
    QIE_TRY(kv8_exps_make(src, a.sm, &a.se, "qie_kv_copy_fp8"));
    QIE_TRY(kv8_exps_make(dst, a.dm, &a.de, "qie_kv_copy_fp8"));
    QIE_REQUIRE((int64_t)pos0 + n_rows <= s.max_ctx && (int64_t)pos0 + n_rows <= d.max_ctx,
                "qie_kv_copy_fp8: positions %d..%lld exceed max_ctx %d / %d", pos0, (long long)pos0 + n_rows - 1,
                s.max_ctx, d.max_ctx);
    const bool same = s.block_table ? s.k == d.k && s.block_table + (int64_t)src_seq * s.max_pages ==
                                                        d.block_table + (int64_t)dst_seq * d.max_pages
                                    : (const uint8_t*)s.k + (int64_t)src_seq * s.seq_stride ==
                                          (const uint8_t*)d.k + (int64_t)dst_seq * d.seq_stride;
    QIE_REQUIRE(!same, "qie_kv_copy_fp8: source and destination are the same sequence of the same cache");
    if (n_rows == 0) return 0;
    const int hd = s.head_dim;
    const int64_t lg = (int64_t)s.n_layers * s.n_kv_heads;
    const int64_t units = (int64_t)n_rows * (hd / 16);
    QIE_REQUIRE(lg <= 65535 && units <= INT32_MAX / 2, "qie_kv_copy_fp8: %lld (layer, kv head) runs of %lld units",
                (long long)lg, (long long)units);
    a.sk = (const uint8_t*)s.k; a.sv = (const uint8_t*)s.v;
    a.dk = (uint8_t*)d.k; a.dv = (uint8_t*)d.v;
    a.sseq = src_seq; a.dseq = dst_seq; a.pos0 = pos0; a.units = (int)units; a.n_rows = n_rows;
    a.cpr = hd / 16; a.hd = hd;
    const dim3 grid((unsigned)((units + 255) / 256), (unsigned)lg, 2);
    hipLaunchKernelGGL((a.sm.table ? kv_copy_fp8_kernel<true> : kv_copy_fp8_kernel<false>), grid, dim3(256), 0,
                       (hipStream_t)stream, a);
    QIE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
