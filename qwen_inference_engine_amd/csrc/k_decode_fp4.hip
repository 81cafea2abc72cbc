// k_decode_fp4.hip — the M <= 16 layer projections on MXFP4 weights (1 <= M <= 16 rows), and the
// MXFP4 format's own operators (quantise, dequantise, tile, decode probe).
//
// Replaces matrix_mul (layers/src/matrix_mul.cu:165-288) for decode, verify and short prefill
// steps of a model whose projection weights are MXFP4 (qie_ops.h: e2m1 codes in 32-element
// blocks with one e8m0 scale each), plus the launch_rms in front of QKV and gate/up
// (normalization.cu:5-25).  The structure is dec8_kernel's (k_decode_fp8.hip):
//   * a block of KS waves owns whole 16-column tiles; wave w owns the SAME K slice of every
//     tile, so its A fragments (16 rows x its K slice) are loaded once and stay in registers;
//   * the RMSNorm is fused from the block's joint sum of squares (REF and HF numerics);
//   * weights are non-temporal 16-B buffer loads in half-tile steps, the next step in flight;
//   * the KS partial C tiles meet in double-buffered LDS behind one barrier per tile (or all at
//     the block's end), the epilogue (linear_epilogue.hpp) by a wave that rotates with the tile;
//   * long K by split-K in part order through slabs and tickets.
// What differs:
//   * a unit is 128 columns: one 16-B load per lane is 32 codes = ONE MX block of one row
//     (lane (fr, g): row fr of the tile, columns 128 j + 32 g + [0, 32)) and yields the B
//     operands of four v_mfma_f32_16x16x32_bf16; MFMA i of a unit multiplies columns
//     128 j + 32 g + 8 i + [0, 8), and the A fragments are loaded under the same mapping
//     (4 KU 16-B vectors per lane);
//   * the block scale enters in the conversion: v_cvt_scalef32_pk_bf16_fp4 takes the e8m0 byte
//     shifted into an f32 exponent field as its scale operand — two codes -> two bf16 per VALU
//     op, no separate multiply, and no row scale in the epilogue;
//   * KS is a launch parameter (block size) below the instantiation's bound, and the last
//     wave's slice may be ragged (units past K: zero A rows, loads out of the buffer range), so
//     three slice widths (KU = 2, 4, 8 units) cover every K % 128 == 0 up to 8,192.
// Numerics contract: products of the bf16 activations (after the fused norm's bf16 rounding) and
// the exactly dequantised bf16 weights (every code x 2^k is a bf16) accumulate in fp32 in one fixed
// order: a wave walks its K slice unit by unit, and within a unit MFMA i = 0..3 adds the 32
// products of columns 128 j + 32 g + 8 i + [0, 8), g = 0..3 (the instruction's own order over its
// 32-k step) to the running sum; then the slices in wave order, split parts in part order.  No
// float atomics; two runs are bit-identical; row m's result does not depend on M.  The
// epilogues round exactly as the reference's separate kernels (bf16 after each op).
#include "qie_common.hpp"
#include "launch_util.hpp"
#include "linear_epilogue.hpp"
#include "linear_plan.hpp"
#include "../../include/qie/qie_ops.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>

namespace qie {

typedef unsigned int d4_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 d4_bf16x8 __attribute__((ext_vector_type(8)));
typedef float d4_f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ the format
// e8m0 exponent of a block's scale: the smallest 2^k with amax <= 6 * 2^k, -125 <= k <= 125; k = 0
// for an all-zero block.  Exact: amax = f 2^e with f in [0.5, 1) is <= 1.5 * 2^(k + 2) from
// k = e - 3 on where f <= 0.75, from k = e - 2 on otherwise.  The upper clamp keeps finite input
// finite: 6 * 2^125 = 1.5 * 2^127 is the largest product that is a finite bf16, and at k = 126 the
// nearest code of a maximum in (3.5 * 2^126, 2^128) would be 4 * 2^126 = inf; such a block (maxima
// above 1.5 * 2^127, the top 0.4 octave of bf16) takes k = 125 and its elements beyond 6 * 2^125
// round to code 6, the only place where the quantiser saturates.
__host__ __device__ inline int fp4_block_exp(float amax) {
    if (!(amax > 0.f)) return 127;
    int e;
    const float f = frexpf(amax, &e);
    int k = f <= 0.75f ? e - 3 : e - 2;
    if (k < -125) k = -125;
    if (k > 125) k = 125;
    return k + 127;
}
// q = w / s -> e2m1 code: nearest grid value, ties to the even code index; a magnitude that
// rounds to 0 is code 0
__host__ __device__ inline uint8_t e2m1_encode(float q) {
    const float a = fabsf(q);
    const int idx = a <= 0.25f ? 0 : a < 0.75f ? 1 : a <= 1.25f ? 2 : a < 1.75f ? 3 : a <= 2.5f ? 4 : a < 3.5f ? 5 : a <= 5.f ? 6 : 7;
    return (uint8_t)(idx == 0 ? 0 : (q < 0.f ? 8 | idx : idx));
}
__host__ __device__ inline float e2m1_decode(uint32_t c) {
    const int idx = c & 7;
    const float v = idx < 4 ? 0.5f * (float)idx : (idx < 6 ? (float)(idx - 2) : (idx == 6 ? 4.f : 6.f));
    return (c & 8) ? -v : v;
}
// 32 bf16 (four 16-B vectors) -> 16 code bytes + the block's e8m0 byte
__host__ __device__ inline void fp4_quantize_block(const uint16_t* w, uint8_t* codes, uint8_t* ex) {
    float v[32], amax = 0.f;
    for (int i = 0; i < 32; i++) {
        const uint32_t u = (uint32_t)w[i] << 16;
        memcpy(&v[i], &u, 4);
        amax = fmaxf(amax, fabsf(v[i]));
    }
    const int e = fp4_block_exp(amax);
    const float s = ldexpf(1.f, e - 127);
    for (int i = 0; i < 16; i++)
        codes[i] = (uint8_t)(e2m1_encode(v[2 * i] / s) | (e2m1_encode(v[2 * i + 1] / s) << 4));
    *ex = (uint8_t)e;
}

// eight codes of one MX block -> eight bf16, the kernel's conversion: four
// v_cvt_scalef32_pk_bf16_fp4, byte b of the word = columns 2b (low nibble) and 2b + 1
// (tests/test_gpu_fp4.py checks every code under several exponents: qie_debug_fp4_decode_bf16)
__device__ __forceinline__ d4_u32x4 fp4x8_to_bf16x8(uint32_t w, float sc) {
    const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0);
    const auto p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1);
    const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2);
    const auto p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3);
    return d4_u32x4{__builtin_bit_cast(uint32_t, p0), __builtin_bit_cast(uint32_t, p1), __builtin_bit_cast(uint32_t, p2),
                    __builtin_bit_cast(uint32_t, p3)};
}
// the e8m0 byte as the conversion's scale operand: the f32 with that exponent field
__device__ __forceinline__ float e8m0_scale(uint32_t e) { return __uint_as_float(e << 23); }

struct Dec4Params {
    const uint16_t* x;         // [M][ldx] bf16 activation rows
    int64_t ldx;
    const uint16_t* norm_w;    // fused RMSNorm weights (null: rows used as they are)
    float eps;
    int numerics;
    const uint8_t* w[3];       // segment bases: codes, then e8m0 scales (plain or tiled)
    const uint16_t* bias[3];   // per segment, may be null
    int32_t seg_rows[3];
    int32_t t01[2];            // tiles in segment 0, in segments 0 + 1
    int32_t K, N, M;
    int32_t n_tiles;
    int32_t ks;                // waves per block (K slices)
    uint16_t* y;               // [M][ldy] (fp32 for QIE_EPI_F32)
    int64_t ldy;
    unsigned long long* keys;  // arg-max keys per row (STORE), may be null
    int64_t key_col0;
    // split-K (SPL instantiations): `parts` slices of ks * KU units, block b serves part
    // b % parts; each part's reduced tile goes write-through to slab [tile][part] and the last
    // arriving part (ticket cnt[tile]) sums them in part order
    int parts;
    float* slab;
    unsigned* cnt;
};

// one bf16 pair of the RMSNorm step: dec8_kernel's arithmetic (k_decode_fp8.hip d8_rms_pair), the
// numerics as a launch-uniform select instead of two copies of the prologue (two branches that
// each rewrite every A fragment cost 13 to 30 VGPRs in every instantiation)
__device__ __forceinline__ uint32_t d4_rms_pair(bool hf, uint32_t xv, uint32_t wv, float rr, float inv) {
#pragma clang fp contract(off)
    const float a[2] = {bf_lo(xv), bf_hi(xv)}, w[2] = {bf_lo(wv), bf_hi(wv)};
    float y[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const float q = a[j] * inv;
        y[j] = (hf ? rbf(q) : fmaf(fmaf(-q, rr, a[j]), inv, q)) * w[j];
    }
    return pack2(y[0], y[1]);
}

// partial-tile slots in LDS: RDF slots of KSMAX x NB 16 x 16 fp32 tiles within 48 KiB
template <int KSMAX, int NB>
constexpr int dec4_rdf() {
    return 49152 / (KSMAX * NB * 1024) < 2 ? 2 : 49152 / (KSMAX * NB * 1024);
}

// KSMAX: the block size bound (the launch runs p.ks <= KSMAX waves).  Split-K: two blocks per
// CU (the bound's second argument: 4 waves per SIMD = 128 VGPRs), as dec8_kernel.
template <int EPI, int KU, int KSMAX, bool SPL = false, bool T16 = false>
__global__ __launch_bounds__(KSMAX * 64, SPL ? 4 : 1) void dec4_kernel(Dec4Params p) {
#pragma clang fp contract(off)
    static_assert(!SPL || EPI != QIE_EPI_SWIGLU, "split-K: single-segment epilogues");
    static_assert(KU % 2 == 0, "half-tile steps");
    constexpr int NB = EPI == QIE_EPI_SWIGLU ? 2 : 1;   // B tiles per column tile (gate, up)
    constexpr int kNT = 2;                               // buffer-load policy: nt (streamed once)
    constexpr int RDF = dec4_rdf<KSMAX, NB>();
    constexpr int NWV = (KU * 16 + 63) / 64;             // norm-weight vectors per lane
    __shared__ __attribute__((aligned(16))) float red[RDF][KSMAX][NB][256];
    __shared__ float ssq[KSMAX][16];
    __shared__ __attribute__((aligned(16))) d4_u32x4 nw_s[KSMAX][KU * 16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int M = p.M, K = p.K, T = p.n_tiles, KS = p.ks;
    const int units = K >> 7;
    // block -> (first tile bi, tile stride G, K part); without split: part 0, G = grid
    const int part = SPL ? (int)blockIdx.x % p.parts : 0;
    const int bi = SPL ? (int)blockIdx.x / p.parts : (int)blockIdx.x;
    const int G = SPL ? (int)gridDim.x / p.parts : (int)gridDim.x;
    if (bi >= T || bi >= G) return;   // block-uniform, before any barrier
    const int my = (T - 1 - bi) / G + 1;
    const int arow = fr < M ? fr : M - 1;
    const int ju0 = (part * KS + wave) * KU;   // this wave's first unit
    // units of this wave past K (a ragged last slice): A fragments 0, weight loads out of the
    // buffer range (0) — wave-uniform, and no load sits under a branch
    const int kval = units - ju0;   // valid units (may be <= 0 or > KU)

    // ---- A fragments of this wave's K slice: row arow, k = 128 (ju0 + u) + 32 g + 8 i + [0, 8)
    d4_u32x4 av[KU][4];
    {
        const d4_u32x4* xp = reinterpret_cast<const d4_u32x4*>(p.x + (int64_t)arow * p.ldx + 32 * g);
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int ok = u < kval;
            const int o = ok ? (ju0 + u) * 16 : 0;
            const d4_u32x4 z = d4_u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const d4_u32x4 v = xp[o + i];
                av[u][i] = ok ? v : z;
            }
        }
    }
    // this wave's slice of the norm weights: 16-B vectors v = lane + 64 q (k = 128 ju0 + 8 v),
    // staged in LDS for the apply below
    const bool nrm = p.norm_w != nullptr;   // launch-uniform
    d4_u32x4 nwv[NWV];
#pragma unroll
    for (int q = 0; q < NWV; q++) {
        const int v = lane + 64 * q;
        const int k = ju0 * 128 + 8 * v;
        nwv[q] = *reinterpret_cast<const d4_u32x4*>((nrm ? p.norm_w : p.x) + (nrm && v < KU * 16 && k < K ? k : 0));
    }

    // A step = half a tile's units (KH per B tile) of one column tile; two steps are in
    // flight (double-buffered registers), i.e. one tile of weights per wave ahead
    constexpr int KH = KU / 2;
    struct Step {
        d4_u32x4 wv[NB][KH];
        uint32_t sc[NB][KH];   // the e8m0 byte of each load's MX block
        float ep[4];           // residual values (rows 4 g + r) or the bias (ep[0])
    };
    // loads of step s: every load unconditional (clamped or out of range), none under a branch;
    // hf (which half of the tile) is a constant at every call site: the epilogue operands ride
    // with the second half only
    auto issue = [&](Step& t, int it, int hf) {
        const int tile = bi + it * G;
        const int sg = NB == 2 ? 0 : (tile < p.t01[0] ? 0 : (tile < p.t01[1] ? 1 : 2));
        const int tb0 = sg == 0 ? 0 : (sg == 1 ? p.t01[0] : p.t01[1]);
        const int rows = p.seg_rows[sg];
        int r = (tile - tb0) * 16 + fr;
        r = r < rows ? r : rows - 1;
        const int ju = ju0 + hf * KH;
        // plain layout: lane (fr, g) reads row r, code bytes 64 j + 16 g + [0, 16) and scale byte
        // (r, 4 j + g); tiled (T16, qie_fp4_tile16): bytes 16 lane of unit j's 1-KiB block and
        // byte `lane` of its 64 scale bytes
        constexpr int UST = T16 ? 1024 : 64, SST = T16 ? 64 : 4;
        const int voff = T16 ? ((tile - tb0) * units + ju) * 1024 + lane * 16 : r * (K >> 1) + ju * 64 + 16 * g;
        const int soff = rows * (K >> 1) + (T16 ? ((tile - tb0) * units + ju) * 64 + lane : r * (K >> 5) + ju * 4 + g);
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const uint8_t* base = p.w[NB == 2 ? b : sg];
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), (short)0,
                                                              (int)((int64_t)rows * ((K >> 1) + (K >> 5))), 0x00020000);
#pragma unroll
            for (int u = 0; u < KH; u++) {
                const bool ok = hf * KH + u < kval;
                t.wv[b][u] = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? voff + u * UST : 0x7ffffff0, 0, kNT);
                t.sc[b][u] = __builtin_amdgcn_raw_buffer_load_b8(rs, ok ? soff + u * SST : 0x7ffffff0, 0, kNT);
            }
        }
        if (!hf) return;
        const int n = tile * 16 + fr;
        const int nc = n < p.N ? n : p.N - 1;
        if constexpr (EPI == QIE_EPI_RESIDUAL) {
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int i = 4 * g + rr < M ? 4 * g + rr : M - 1;
                t.ep[rr] = bf2f(p.y[(int64_t)i * p.ldy + nc]);
            }
        } else if constexpr (EPI == QIE_EPI_STORE) {
            const uint16_t* bp = p.bias[sg];
            const float v = bf2f((bp ? bp : p.x)[bp ? r : 0]);
            t.ep[0] = bp ? v : 0.f;
        }
    };

    Step sa, sb;
    issue(sa, 0, 0);
    __builtin_amdgcn_sched_barrier(0);

    // ---- fused RMSNorm: row arow's sum of squares over the whole K (this wave's slice, the 4
    // k groups by lane exchange, the KS slices through LDS), then the fragments are normalised
    // in place (qie_rmsnorm's arithmetic)
    if (nrm) {
        float ss = 0.f;
#pragma unroll
        for (int u = 0; u < KU; u++)
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const uint32_t e4[4] = {av[u][h].x, av[u][h].y, av[u][h].z, av[u][h].w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float l = bf_lo(e4[j]), hh = bf_hi(e4[j]);
                    ss += l * l + hh * hh;
                }
                __builtin_amdgcn_sched_barrier(0);   // (as in the apply below: no hoisted unpacking)
            }
        ss = xor32_sum(xor16_sum(ss));
        if (g == 0) ssq[wave][fr] = ss;
#pragma unroll
        for (int q = 0; q < NWV; q++)
            if (lane + 64 * q < KU * 16) nw_s[wave][lane + 64 * q] = nwv[q];
        __syncthreads();
        float tot = 0.f;
        for (int w = 0; w < KS; w++) tot += ssq[w][fr];
        const float rms = sqrtf((tot / (float)K) + p.eps);
        const float inv = 1.0f / rms;
        const float rr = rms < INFINITY ? rms : 0.f;
        // the fragments as opaque values from here on: the sum of squares above unpacked every
        // element to fp32, and the compiler otherwise keeps those 32 KU floats per lane live for
        // the apply below instead of unpacking again (KU = 8: ~950 B of scratch per lane)
#pragma unroll
        for (int u = 0; u < KU; u++)
#pragma unroll
            for (int h = 0; h < 4; h++) asm volatile("" : "+v"(av[u][h]));
        const bool hfm = p.numerics == QIE_NUMERICS_HF;   // launch-uniform
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < KU; u++) {   // (units past K: zero rows times the clamped weights stay zero)
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const d4_u32x4 nv = nw_s[wave][16 * u + 4 * g + h];   // k = 128 (ju0 + u) + 32 g + 8 h
                av[u][h].x = d4_rms_pair(hfm, av[u][h].x, nv.x, rr, inv);
                av[u][h].y = d4_rms_pair(hfm, av[u][h].y, nv.y, rr, inv);
                av[u][h].z = d4_rms_pair(hfm, av[u][h].z, nv.z, rr, inv);
                av[u][h].w = d4_rms_pair(hfm, av[u][h].w, nv.w, rr, inv);
                // one fragment at a time: the opaque use pins the finished fragment here (the final
                // products otherwise sink below the whole prologue and every fragment is held twice)
                asm volatile("" : "+v"(av[u][h]));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    unsigned long long kbest[4] = {0ull, 0ull, 0ull, 0ull};
    d4_f32x4 acc[NB];
    auto mma = [&](const Step& t, int hf) {
        if (hf == 0) {
#pragma unroll
            for (int b = 0; b < NB; b++) acc[b] = d4_f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < KH; u++) {
            const int ua = hf * KH + u;   // (hf is a compile-time constant at every call)
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const float sc = e8m0_scale(t.sc[b][u]);
                const uint32_t wd[4] = {t.wv[b][u].x, t.wv[b][u].y, t.wv[b][u].z, t.wv[b][u].w};
#pragma unroll
                for (int i = 0; i < 4; i++)
                    acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(d4_bf16x8, av[ua][i]),
                                                                     __builtin_bit_cast(d4_bf16x8, fp4x8_to_bf16x8(wd[i], sc)),
                                                                     acc[b], 0, 0, 0);
            }
            // one unit at a time: left alone the scheduler converts a whole step's codes ahead of
            // its MFMAs (16 VGPRs of B operands per unit and B tile; KU = 8 then spilled 950 B)
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // the epilogue of one output tile from its fp32 sums
    auto emit = [&](int tile, const float (&sum)[NB][4], const float* epv) {
        const int n = tile * 16 + fr;
        emit_tile16<EPI>(sum, epv, p.y, p.ldy, M, p.N, n, g, p.keys, p.key_col0, kbest);
    };
    const bool half = M <= 8;   // rows 0..7: lanes 0..31
    // blocks of one or two tiles keep the per-tile hand-off, longer ones keep every tile's
    // partials and reduce them after one barrier (dec8_kernel's measured rule); split-K defers
    const bool defer = (SPL || my >= 3) && my <= (half ? 2 * RDF : RDF);   // block-uniform
    // where tile it's partial of wave w, B tile b, lives (lane-indexed float4)
    auto slot_at = [&](int it, int w, int b) -> float* {
        if (defer && half) return &red[it >> 1][w][b][(it & 1) * 128 + lane * 4];
        return &red[defer ? it : (it & 1)][w][b][lane * 4];
    };
    // the KS waves' partials of tile it, summed in wave order (the same order either way;
    // lanes past row 7 read another tile's slot in the packed form: their rows are >= M)
    auto reduce = [&](int it, float (&sum)[NB][4]) {
#pragma unroll
        for (int b = 0; b < NB; b++) {
            float4 v4 = *reinterpret_cast<const float4*>(slot_at(it, 0, b));
            for (int w = 1; w < KS; w++) {
                const float4 v = *reinterpret_cast<const float4*>(slot_at(it, w, b));
                v4.x += v.x; v4.y += v.y; v4.z += v.z; v4.w += v.w;
            }
            sum[b][0] = v4.x; sum[b][1] = v4.y; sum[b][2] = v4.z; sum[b][3] = v4.w;
        }
    };
    // the epilogue operands of a tile, reloaded (deferred epilogues and the split tail; the
    // per-tile path has them from the tile's step loads, issue())
    auto load_epi = [&](int tile, float (&epv)[4]) {
        const int sg = NB == 2 ? 0 : (tile < p.t01[0] ? 0 : (tile < p.t01[1] ? 1 : 2));
        const int tb0 = sg == 0 ? 0 : (sg == 1 ? p.t01[0] : p.t01[1]);
        const int rows = p.seg_rows[sg];
        int r = (tile - tb0) * 16 + fr;
        r = r < rows ? r : rows - 1;
        epv[0] = epv[1] = epv[2] = epv[3] = 0.f;
        const int n = tile * 16 + fr;
        const int nc = n < p.N ? n : p.N - 1;
        if constexpr (EPI == QIE_EPI_RESIDUAL) {
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int i = 4 * g + rr < M ? 4 * g + rr : M - 1;
                epv[rr] = bf2f(p.y[(int64_t)i * p.ldy + nc]);
            }
        } else if constexpr (EPI == QIE_EPI_STORE) {
            const uint16_t* bp = p.bias[sg];
            epv[0] = bp ? bf2f(bp[r]) : 0.f;
        }
    };
    // tile end (after its second step): this wave's partial tile -> LDS; deferred: nothing
    // else until the block's last tile; else one barrier and the rotating wave's epilogue
    auto finish = [&](const Step& t, int it) {
        if (!(defer && half) || lane < 32) {
#pragma unroll
            for (int b = 0; b < NB; b++)
                *reinterpret_cast<float4*>(slot_at(it, wave, b)) = make_float4(acc[b][0], acc[b][1], acc[b][2], acc[b][3]);
        }
        if (defer) return;   // block-uniform
        // one barrier per tile: the next write of a slot is two tiles away, behind the next
        // tile's barrier, which the epilogue wave reaches only after its reads
        __syncthreads();
        if constexpr (!SPL) {   // (split-K blocks always defer: dec4_launch caps their tiles)
            if (wave != it % KS) return;   // wave-uniform
            float sum[NB][4];
            reduce(it, sum);
            emit(bi + it * G, sum, t.ep);
        }
    };

    // split-K tail of tile it: publish this part's sums write-through, drain, take the ticket;
    // the last arriver sums every part in part order (independent of arrival order), reloads
    // the epilogue operands, emits
    auto split_tail = [&](int it) {
        const int tile = bi + it * G;
        float* tb = p.slab + (int64_t)tile * p.parts * 256;
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(tb, (short)0, p.parts * 1024, 0x00020000);
        float ks[NB][4];
        reduce(it, ks);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(d4_u32x4, d4_f32x4{ks[0][0], ks[0][1], ks[0][2], ks[0][3]}), rs,
                                               part * 1024 + lane * 16, 0, 16);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned old = 0;
        if (lane == 0) old = __hip_atomic_fetch_add(p.cnt + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        old = __shfl(old, 0, 64);
        if (old != (unsigned)p.parts - 1) return;   // wave-uniform
        float epv[4];
        load_epi(tile, epv);
        float sum[NB][4];
        for (int q = 0; q < p.parts; q++) {
            const d4_f32x4 v = __builtin_bit_cast(d4_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, q * 1024 + lane * 16, 0, 16));
#pragma unroll
            for (int j = 0; j < 4; j++) sum[0][j] = q == 0 ? v[j] : sum[0][j] + v[j];
        }
        if (lane == 0) __hip_atomic_store(p.cnt + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        emit(tile, sum, epv);
    };

    // steps alternate sa (first half of a tile) / sb (second half); the next step is always
    // issued before this one is computed
    __builtin_amdgcn_sched_barrier(0);
    int it = 0;
    for (; it + 1 < my; it++) {
        issue(sb, it, 1);
        mma(sa, 0);
        issue(sa, it + 1, 0);
        mma(sb, 1);
        finish(sb, it);
    }
    issue(sb, it, 1);
    mma(sa, 0);
    mma(sb, 1);
    finish(sb, it);
    if (defer) {   // block-uniform: every wave's partials of every tile are in red[]
        __syncthreads();
        for (int t2 = wave; t2 < my; t2 += KS) {
            if constexpr (SPL) {
                split_tail(t2);
            } else {
                float sum[NB][4], epv[4];
                load_epi(bi + t2 * G, epv);
                reduce(t2, sum);
                emit(bi + t2 * G, sum, epv);
            }
        }
    }
    if constexpr (EPI == QIE_EPI_STORE) {
        if (p.keys) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                unsigned long long v = kbest[r];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {   // max over the 16 columns of row 4 g + r
                    const unsigned long long s = __shfl_xor(v, o, 64);
                    v = s > v ? s : v;
                }
                if (fr == 0 && 4 * g + r < M && v) atomicMax(p.keys + 4 * g + r, v);
            }
        }
    }
}

template <int EPI, int KU, int KSMAX, bool SPL, bool T16>
static int dec4_launch(const Dec4Params& p, hipStream_t st) {
    const void* fn = (const void*)dec4_kernel<EPI, KU, KSMAX, SPL, T16>;
    const int per_cu = resident_blocks_per_cu(fn, p.ks * 64, 0, 1);
    const int64_t slots = (int64_t)device_cu_count() * per_cu;
    int grid;
    if constexpr (SPL) {   // parts x G blocks, G tiles in flight per part (one round if they fit)
        // and at most RDF tiles per block (the kernel keeps every tile's partials in LDS)
        constexpr int RDF = dec4_rdf<KSMAX, 1>();
        const int64_t g = std::max<int64_t>((p.n_tiles + RDF - 1) / RDF, std::min<int64_t>(p.n_tiles, slots / p.parts));
        grid = (int)(g * p.parts);
    } else {
        grid = (int)std::max<int64_t>(1, std::min<int64_t>(p.n_tiles, slots));
    }
    hipLaunchKernelGGL((dec4_kernel<EPI, KU, KSMAX, SPL, T16>), dim3(grid), dim3(p.ks * 64), 0, st, p);
    QIE_LAUNCH_CHECK();
    return 0;
}

// Split-K workspace (slabs + tickets), one per stream, a sibling of the fp8 kernel's: reserved
// by qie_batch_create of an fp4 engine (dec4_reserve) so that a captured step finds it; tickets
// are zero at rest (the last arriver resets its tile's).
namespace {
struct Dec4Ws {
    float* slab = nullptr;
    unsigned* cnt = nullptr;
};
std::mutex g_d4_mu;
std::map<hipStream_t, Dec4Ws> g_d4_ws;
}  // namespace

int dec4_reserve(hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_d4_mu);
    Dec4Ws& w = g_d4_ws[st];
    if (w.slab) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return 1;
    QIE_HIP(hipMalloc((void**)&w.slab, (size_t)kDec8MaxTiles * kDec8MaxParts * 1024));
    QIE_HIP(hipMalloc((void**)&w.cnt, (size_t)kDec8MaxTiles * 4));
    QIE_HIP(hipMemsetAsync(w.cnt, 0, (size_t)kDec8MaxTiles * 4, st));
    QIE_HIP(hipStreamSynchronize(st));
    return 0;
}

template <int KU, int KSMAX, bool T16>
static int dec4_epi(const Dec4Params& p, int epi, hipStream_t st) {
    return dispatch_epi(epi, [&](auto E) { return dec4_launch<decltype(E)::value, KU, KSMAX, false, T16>(p, st); });
}
template <bool T16>
static int dec4_epi_split(const Dec4Params& p, int epi, hipStream_t st) {
    return dispatch_epi<QIE_EPI_RESIDUAL, QIE_EPI_F32, QIE_EPI_STORE>(epi, [&](auto E) {
        return dec4_launch<decltype(E)::value, kDec4SplitKu, kDec4SplitKs, true, T16>(p, st);
    });
}

// The one reader of fp4 weights.  A split-K launch whose workspace cannot be made (the stream is
// capturing and nothing reserved it) is an error: there is no other kernel to run instead.
int dec4_linear(const qie_linear_args* a, const LinearPlan& pl, hipStream_t st) {
    QIE_REQUIRE(pl.family == LinearFamily::Dec4 && pl.error == PlanError::None,
                "qie_linear: internal: fp4 batched-decode path does not apply");
    const bool t16 = (a->flags & QIE_LINEAR_FP4_T16) != 0;
    Dec4Params p;
    p.x = (const uint16_t*)a->x;
    p.ldx = a->ldx;
    p.norm_w = (const uint16_t*)a->norm_w;
    p.eps = a->norm_eps;
    p.numerics = a->numerics;
    p.K = (int32_t)a->K;
    p.N = (int32_t)a->N;
    p.M = (int32_t)a->M;
    p.y = (uint16_t*)a->y;
    p.ldy = a->ldy;
    p.keys = (unsigned long long*)a->argmax_keys;
    p.key_col0 = a->key_col0;
    p.parts = 1;
    p.slab = nullptr;
    p.cnt = nullptr;
    p.ks = pl.dec4_ks;
    p.n_tiles = (int32_t)((a->N + 15) / 16);
    for (int s = 0; s < 3; s++) {
        p.w[s] = (const uint8_t*)a->w[s];
        p.bias[s] = (const uint16_t*)a->bias[s];
    }
    if (a->epilogue == QIE_EPI_SWIGLU) {
        p.seg_rows[0] = p.seg_rows[1] = p.seg_rows[2] = (int32_t)a->N;
        p.t01[0] = p.t01[1] = p.n_tiles;
    } else {
        const int64_t r0 = a->seg_rows[0] > 0 ? a->seg_rows[0] : a->N;
        const int64_t r1 = a->seg_rows[1];
        p.seg_rows[0] = (int32_t)r0;
        p.seg_rows[1] = (int32_t)(r1 > 0 ? r1 : 1);
        p.seg_rows[2] = (int32_t)std::max<int64_t>(1, a->N - r0 - r1);
        p.t01[0] = (int32_t)((r0 + 15) / 16);   // (whole tiles wherever a segment follows: dec4_plan)
        p.t01[1] = (int32_t)((r0 + r1 + 15) / 16);
        QIE_REQUIRE(r0 + r1 <= a->N && (r1 == 0 || a->w[1]) && (r0 + r1 == a->N || a->w[2]) && a->w[0],
                    "qie_linear: segment rows do not match the weights");
    }
    const int ku = pl.dec4_ku;
    if (pl.dec4_parts >= 2) {
        p.parts = pl.dec4_parts;
        if (dec4_reserve(st) != 0)
            return fail(-22, "qie_linear: fp4 split-K (K=%lld) needs its workspace before a graph capture: run one such "
                             "launch, or create the batch, outside the capture", (long long)a->K);
        {
            std::lock_guard<std::mutex> lk(g_d4_mu);
            const Dec4Ws& w = g_d4_ws[st];
            p.slab = w.slab;
            p.cnt = w.cnt;
        }
        return t16 ? dec4_epi_split<true>(p, a->epilogue, st) : dec4_epi_split<false>(p, a->epilogue, st);
    }
    if (t16) {
        if (ku == 2) return dec4_epi<2, 4, true>(p, a->epilogue, st);
        if (ku == 4) return dec4_epi<4, 8, true>(p, a->epilogue, st);
        return dec4_epi<8, 8, true>(p, a->epilogue, st);
    }
    if (ku == 2) return dec4_epi<2, 4, false>(p, a->epilogue, st);
    if (ku == 4) return dec4_epi<4, 8, false>(p, a->epilogue, st);
    return dec4_epi<8, 8, false>(p, a->epilogue, st);
}

// ------------------------------------------------------------------ format operators
// one thread per MX block (32 weights), grid-stride: the quantiser is a load-time pass
__global__ __launch_bounds__(256) void quantize_fp4_kernel(const uint16_t* __restrict__ w, int64_t nblk,
                                                           uint8_t* __restrict__ codes, uint8_t* __restrict__ exps) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nblk; i += (int64_t)gridDim.x * 256) {
        alignas(16) uint16_t v[32];
        const uint4* src = reinterpret_cast<const uint4*>(w + 32 * i);
#pragma unroll
        for (int j = 0; j < 4; j++) *reinterpret_cast<uint4*>(v + 8 * j) = src[j];
        alignas(16) uint8_t c[16];
        uint8_t e;
        fp4_quantize_block(v, c, &e);
        *reinterpret_cast<uint4*>(codes + 16 * i) = *reinterpret_cast<const uint4*>(c);
        exps[i] = e;
    }
}

__global__ __launch_bounds__(256) void dequantize_fp4_kernel(const uint4* __restrict__ codes, const uint8_t* __restrict__ exps,
                                                             int64_t nblk, uint4* __restrict__ out) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nblk; i += (int64_t)gridDim.x * 256) {
        const uint4 q = codes[i];
        const float s = ldexpf(1.f, (int)exps[i] - 127);
        const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t o[4];
#pragma unroll
            for (int b = 0; b < 4; b++)
                o[b] = pack2(e2m1_decode(wd[j] >> (8 * b)) * s, e2m1_decode(wd[j] >> (8 * b + 4)) * s);
            out[4 * i + j] = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

// plain -> 16-row tiled (qie_ops.h): output piece (t, j, l) <- row 16 t + l % 16, MX block
// 4 j + l / 16 of that row — the same index for the 16 code bytes and for the scale byte
__global__ __launch_bounds__(256) void fp4_tile16_kernel(const uint4* __restrict__ in, const uint8_t* __restrict__ sin,
                                                         int64_t blk_per_row, int64_t units, int64_t nblk,
                                                         uint4* __restrict__ out, uint8_t* __restrict__ sout) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nblk; i += (int64_t)gridDim.x * 256) {
        const int64_t l = i & 63, blk = i >> 6;
        const int64_t t = blk / units, j = blk % units;
        const int64_t src = (16 * t + (l & 15)) * blk_per_row + 4 * j + (l >> 4);
        out[i] = in[src];
        sout[i] = sin[src];
    }
}

struct Fp4ProbeArgs {
    uint8_t e[16];
};
__global__ void fp4_decode_probe_kernel(Fp4ProbeArgs a, int n, uint16_t* out) {
    const int i = threadIdx.x;
    if (i >= n) return;
    const float sc = e8m0_scale(a.e[i]);
    const d4_u32x4 lo = fp4x8_to_bf16x8(0x76543210u, sc), hi = fp4x8_to_bf16x8(0xFEDCBA98u, sc);
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    for (int j = 0; j < 8; j++) {
        out[16 * i + 2 * j] = (uint16_t)(w[j] & 0xffff);
        out[16 * i + 2 * j + 1] = (uint16_t)(w[j] >> 16);
    }
}

static unsigned fp4_grid(int64_t nblk) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((nblk + 255) / 256, (int64_t)device_cu_count() * 16));
}

}  // namespace qie

using namespace qie;

extern "C" {

int64_t qie_fp4_weight_bytes(int64_t rows, int64_t cols) { return rows * cols / 2 + rows * cols / 32; }

int qie_quantize_fp4(const void* w_bf16, int64_t rows, int64_t cols, void* out, void* stream) {
    QIE_REQUIRE(w_bf16 && out && rows > 0 && cols > 0 && cols % 32 == 0 && ((uintptr_t)w_bf16 % 16) == 0 &&
                    ((uintptr_t)out % 16) == 0,
                "qie_quantize_fp4: bad arguments (cols %% 32 == 0, 16-B aligned buffers)");
    const int64_t nblk = rows * cols / 32;
    uint8_t* codes = (uint8_t*)out;
    hipLaunchKernelGGL(quantize_fp4_kernel, dim3(fp4_grid(nblk)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)w_bf16,
                       nblk, codes, codes + rows * cols / 2);
    QIE_LAUNCH_CHECK();
    return 0;
}

int qie_quantize_fp4_host(const void* w_bf16, int64_t rows, int64_t cols, void* out) {
    QIE_REQUIRE(w_bf16 && out && rows > 0 && cols > 0 && cols % 32 == 0, "qie_quantize_fp4_host: bad arguments (cols %% 32 == 0)");
    const uint16_t* w = (const uint16_t*)w_bf16;
    uint8_t* codes = (uint8_t*)out;
    uint8_t* exps = codes + rows * cols / 2;
    const int64_t nblk = rows * cols / 32;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < nblk; i++) fp4_quantize_block(w + 32 * i, codes + 16 * i, exps + i);
    return 0;
}

int qie_dequantize_fp4(const void* w_fp4, int64_t rows, int64_t cols, void* out_bf16, void* stream) {
    QIE_REQUIRE(w_fp4 && out_bf16 && rows > 0 && cols > 0 && cols % 32 == 0 && ((uintptr_t)w_fp4 % 16) == 0 &&
                    ((uintptr_t)out_bf16 % 16) == 0,
                "qie_dequantize_fp4: bad arguments (cols %% 32 == 0, 16-B aligned buffers)");
    const int64_t nblk = rows * cols / 32;
    const uint8_t* codes = (const uint8_t*)w_fp4;
    hipLaunchKernelGGL(dequantize_fp4_kernel, dim3(fp4_grid(nblk)), dim3(256), 0, (hipStream_t)stream, (const uint4*)codes,
                       codes + rows * cols / 2, nblk, (uint4*)out_bf16);
    QIE_LAUNCH_CHECK();
    return 0;
}

int qie_fp4_tile16(const void* w_fp4, int64_t rows, int64_t cols, void* out, void* stream) {
    QIE_REQUIRE(w_fp4 && out && w_fp4 != out && rows > 0 && rows % 16 == 0 && cols > 0 && cols % 128 == 0 &&
                    ((uintptr_t)w_fp4 % 16) == 0 && ((uintptr_t)out % 16) == 0,
                "qie_fp4_tile16: bad arguments (rows %% 16 == 0, cols %% 128 == 0, distinct 16-B aligned buffers)");
    const int64_t nblk = rows * cols / 32;
    const uint8_t* in = (const uint8_t*)w_fp4;
    uint8_t* o = (uint8_t*)out;
    hipLaunchKernelGGL(fp4_tile16_kernel, dim3(fp4_grid(nblk)), dim3(256), 0, (hipStream_t)stream, (const uint4*)in,
                       in + rows * cols / 2, cols / 32, cols / 128, nblk, (uint4*)o, o + rows * cols / 2);
    QIE_LAUNCH_CHECK();
    return 0;
}

int qie_debug_fp4_decode_bf16(const uint8_t* exps, int32_t n_exps, uint16_t* out_dev) {
    QIE_REQUIRE(exps && out_dev && n_exps >= 1 && n_exps <= 16, "qie_debug_fp4_decode_bf16: bad arguments (1..16 exponents)");
    Fp4ProbeArgs a;
    memset(&a, 0, sizeof(a));
    memcpy(a.e, exps, (size_t)n_exps);
    hipLaunchKernelGGL(fp4_decode_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)0, a, (int)n_exps, out_dev);
    QIE_LAUNCH_CHECK();
    QIE_HIP(hipDeviceSynchronize());
    return 0;
}

}  // extern "C"
