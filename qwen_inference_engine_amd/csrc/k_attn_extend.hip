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
// and the per-tile softmax are attn_prefill_mfma2_kernel's (k_attention.hip), which documents
// the operand layouts; differences are marked below.
#include "qie_common.hpp"
#include "../../include/qie/qie_ops.h"
#include "attn_decode.hpp"

#include <type_traits>

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
    float* part_o;    // [M][nq][nsplit][HD]
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
    constexpr int CPR = HD / 8;
    constexpr int KSTEPS = HD / 32;
    constexpr int DT = HD / 16;
    constexpr int QG = 2;                  // 16-row query groups per wave
    constexpr int NGB = QG * NW;           // groups per block
    static_assert(16 * NGB == kExtBlockRows, "attn_extend: block rows");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* Ks = reinterpret_cast<uint16_t*>(smem);
    uint16_t* Vs = reinterpret_cast<uint16_t*>(smem + 2 * KT * HD * 2);
    auto vswz = [](int r) { return 2 * (r & (CPR / 2 - 1)); };

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
    const int kt0 = k0 / KT;
    const int nkt = min((k0 + a.split_len) / KT, kmax / KT + 1);   // tiles [kt0, nkt); past kmax: not loaded

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

    // K/V tiles: buffer loads to LDS on a per-tile resource that ends at row kmax (rows past
    // it read as zeros; their keys are masked), chunk swizzle on the source address
    constexpr int RPI = 512 / HD;                 // key rows per 1 KiB wave-instruction
    constexpr int IPW = KT / RPI / NW;            // wave-instructions per wave per operand
    uint32_t koff[IPW], voff[IPW];
#pragma unroll
    for (int i = 0; i < IPW; i++) {
        const int r = (wave * IPW + i) * RPI + lane / CPR, pch = lane % CPR;
        koff[i] = (uint32_t)(r * HD + (pch ^ (r & (CPR - 1))) * 8) * 2;
        voff[i] = (uint32_t)(r * HD + (pch ^ vswz(r)) * 8) * 2;
    }
    auto issue = [&](int kt, int buf) {
        const int64_t tb = kv_tok<PG>(a.km, seq, kt * KT, HD);
        const int rows = min(KT, kmax + 1 - kt * KT);
        const auto rk = __builtin_amdgcn_make_buffer_rsrc((void*)(kb + tb), (short)0, rows * HD * 2, 0x00020000);
        const auto rv = __builtin_amdgcn_make_buffer_rsrc((void*)(vb + tb), (short)0, rows * HD * 2, 0x00020000);
#pragma unroll
        for (int i = 0; i < IPW; i++) {
            const int inst = wave * IPW + i;
            buf_lds16(rk, Ks + buf * KT * HD + inst * 512, koff[i]);
            buf_lds16(rv, Vs + buf * KT * HD + inst * 512, voff[i]);
        }
    };

    f32x4_t oacc[QG][DT];
#pragma unroll
    for (int q = 0; q < QG; q++)
#pragma unroll
        for (int d = 0; d < DT; d++) oacc[q][d] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m_run[QG], l_run[QG];
#pragma unroll
    for (int q = 0; q < QG; q++) {
        m_run[q] = -INFINITY;
        l_run[q] = 0.f;
    }
    const float sl2 = 1.4426950408889634f / sqrtf((float)HD);   // log2(e) / sqrt(hd)

    issue(kt0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    auto tile = [&](const int kt, const uint16_t* K, const uint16_t* Vt, auto q0c, auto q1c) {
            constexpr bool ON[QG] = {decltype(q0c)::value, decltype(q1c)::value};
            f32x4_t sacc[QG][4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
#pragma unroll
                for (int q = 0; q < QG; q++) sacc[q][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                const int r = t * 16 + fr;
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ks++) {
                    const int ch = ks * 4 + g;
                    const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(K + r * HD + ((ch ^ (r & (CPR - 1))) * 8));
#pragma unroll
                    for (int q = 0; q < QG; q++)
                        if (ON[q]) sacc[q][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[q][ks], sacc[q][t], 0, 0, 0);
                }
            }
            float pv[QG][4][4];
#pragma unroll
            for (int q = 0; q < QG; q++) {
                if (!ON[q]) continue;
                float (&sv)[4][4] = pv[q];
                float mt = -INFINITY;
                if (kt * KT + KT - 1 <= gmin[q]) {   // wave-uniform: no key of the tile is masked
#pragma unroll
                    for (int t = 0; t < 4; t++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const float sc = sacc[q][t][r] * sl2;
                            sv[t][r] = sc;
                            mt = fmaxf(mt, sc);
                        }
                } else {
#pragma unroll
                    for (int t = 0; t < 4; t++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int key = kt * KT + t * 16 + g * 4 + r;
                            const float sc = key <= qpos[q] ? sacc[q][t][r] * sl2 : -INFINITY;
                            sv[t][r] = sc;
                            mt = fmaxf(mt, sc);
                        }
                }
                mt = xor32_max(xor16_max(mt));
                // unlike the prefill kernel's, a split past a row's position shows it no key
                // at all: the running max stays -inf there, and the exponent base must not
                // (-inf - -inf is NaN)
                const float m_new = fmaxf(m_run[q], mt);
                const float m_use = m_new == -INFINITY ? 0.f : m_new;
                const float alpha = __builtin_amdgcn_exp2f(m_run[q] - m_use);
                float ls = 0.f;
#pragma unroll
                for (int t = 0; t < 4; t++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float e = __builtin_amdgcn_exp2f(sv[t][r] - m_use);
                        sv[t][r] = e;
                        ls += e;
                    }
                ls = xor32_sum(xor16_sum(ls));
                l_run[q] = l_run[q] * alpha + ls;
                m_run[q] = m_new;
                // the split's first tile finds O zero; alpha == 1 exactly where no max grew
                if (kt > kt0 && __builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
                    float ar[4];
#pragma unroll
                    for (int r = 0; r < 4; r++) ar[r] = __shfl(alpha, g * 4 + r, 64);
#pragma unroll
                    for (int d = 0; d < DT; d++)
#pragma unroll
                        for (int r = 0; r < 4; r++) oacc[q][d][r] *= ar[r];
                }
            }
            const int q4 = fr >> 2, p4 = fr & 3;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                // P = hi + lo bf16 parts, as the prefill kernel
                bf16x8_t ph[QG], pl[QG];
#pragma unroll
                for (int q = 0; q < QG; q++) {
                    if (!ON[q]) continue;
                    float e8[8];
#pragma unroll
                    for (int jj = 0; jj < 8; jj++) e8[jj] = pv[q][2 * c + (jj >> 2)][jj & 3];
                    uint4 pp[2];
                    split_bf16x8<2>(e8, pp);
                    ph[q] = __builtin_bit_cast(bf16x8_t, pp[0]);
                    pl[q] = __builtin_bit_cast(bf16x8_t, pp[1]);
                }
#pragma unroll
                for (int d = 0; d < DT; d++) {
                    const int vr = 32 * c + 4 * g + q4;
                    const uint16_t* a0 = Vt + vr * HD + (((2 * d + (p4 >> 1)) ^ vswz(vr)) * 8) + (p4 & 1) * 4;
                    const i16x4_t v0 =
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4_t*)(a0));
                    const i16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) i16x4_t*)(a0 + 16 * HD));
                    const bf16x8_t vb8 =
                        __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
                    for (int q = 0; q < QG; q++) {
                        if (!ON[q]) continue;
                        oacc[q][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph[q], vb8, oacc[q][d], 0, 0, 0);
                        oacc[q][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl[q], vb8, oacc[q][d], 0, 0, 0);
                    }
                }
            }
        };
    int kt = kt0;
    auto run = [&](const int kend, auto q0c, auto q1c) {
        for (; kt < kend; kt++) {
            // into the other buffer: every wave finished tile kt-1 before the last barrier
            if (kt + 1 < nkt) issue(kt + 1, cur ^ 1);
            if constexpr (decltype(q0c)::value || decltype(q1c)::value)
                tile(kt, Ks + cur * KT * HD, Vs + cur * KT * HD, q0c, q1c);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMAs of tile kt+1
            __syncthreads();                                     // ... and every other wave's
            cur ^= 1;
        }
    };
    // tiles of this split each group takes: [kt0, gpos / KT] (none when the group's last
    // position lies before the split or the group is padding); group 1 is the later one
    const int nkt0 = gpos[0] >= k0 ? min(nkt, gpos[0] / KT + 1) : kt0;
    const int nkt1 = gpos[1] >= k0 ? min(nkt, gpos[1] / KT + 1) : kt0;
    if (nkt1 > kt0) {
        run(nkt0, std::true_type{}, std::true_type{});
        run(nkt1, std::false_type{}, std::true_type{});
    } else {
        run(nkt0, std::true_type{}, std::false_type{});
    }
    run(nkt, std::false_type{}, std::false_type{});

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

// Merge of the splits of one (row, q head): grid (M, nq), HD threads.  The running maxima
// are in the log2 domain (scores * log2(e) / sqrt(hd)), so the weights are exp2.
template <int HD>
__global__ __launch_bounds__(HD) void attn_extend_combine_kernel(ExtendAttnParams a) {
    const int64_t m = blockIdx.x;
    const int h = blockIdx.y, d = threadIdx.x;
    const int64_t base = (m * a.nq + h) * (int64_t)a.nsplit;
    float mn = -INFINITY;
    for (int s = 0; s < a.nsplit; s++) mn = fmaxf(mn, a.part_ml[(base + s) * 2]);
    float l = 0.f, ov = 0.f;
    for (int s = 0; s < a.nsplit; s++) {
        const float ms = a.part_ml[(base + s) * 2];
        if (ms == -INFINITY) continue;   // no visible key: its O is not read
        const float c = __builtin_amdgcn_exp2f(ms - mn);
        l += a.part_ml[(base + s) * 2 + 1] * c;
        ov += a.part_o[(base + s) * HD + d] * c;
    }
    a.out[m * (int64_t)a.nq * HD + (int64_t)h * HD + d] = f2bf(ov / l);
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
        if (cache->head_dim == 128)
            hipLaunchKernelGGL(attn_extend_combine_kernel<128>, dim3((unsigned)M, (unsigned)n_heads), dim3(128), 0, st, a);
        else
            hipLaunchKernelGGL(attn_extend_combine_kernel<64>, dim3((unsigned)M, (unsigned)n_heads), dim3(64), 0, st, a);
        QIE_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
