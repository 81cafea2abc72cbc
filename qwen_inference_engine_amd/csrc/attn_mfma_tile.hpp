// attn_mfma_tile.hpp — the MFMA key-tile walk shared by the causal prefill attention
// (attn_prefill_mfma2_kernel, k_attention.hip) and the split-context extend attention
// (attn_extend_kernel, k_attn_extend.hip), and the merge of split partials both files launch.
// One body: the two kernels differ in how they map rows to a wave's two 16-row query groups
// and in what they do with the result, not in the arithmetic — a row's output depends only
// on which key tiles it sees and on its own masked scores.
//
// Causal flash attention on MFMA (v_mfma_f32_16x16x32_bf16).
// K/V tiles of 64 keys staged in LDS (double-buffered, LDS-DMA prefetch).
//   S^T = K . Q^T  — A = K tile (row = key, k = d) from an XOR-swizzled LDS image,
//                    B = Q^T from registers (lane: q = lane & 15, 8 contiguous d);
//                    so each lane holds 4 keys x 4 key-tiles of ONE query row and
//                    the softmax row statistics need only lanes l, l^16, l^32, l^48.
//   O  += P . V    — A = P straight from the S^T accumulators (bf16), k permuted as
//                    key(j) = 32c + 4g + j (j < 4), 32c + 16 + 4g + (j - 4);
//                    B = V with the SAME key permutation, read by two
//                    ds_read_b64_tr_b16 per fragment from a row-major V image.
// Scores: dot / sqrtf(hd) (fp32), masked keys (> query position) get -inf (the
// reference's -1e9, self_attension.cu:88-92, underflows to the same 0).  They go to the
// log2 domain once (dot * log2(e) / sqrt(hd)) and are exponentiated with v_exp_f32: the
// reference build compiles with -use_fast_math, i.e. __expf / __fdividef.
#pragma once
#include "attn_decode.hpp"

#include <type_traits>

namespace qie {

// A wave (of the NW of its workgroup, all of which must call) walks the key tiles
// [k0 / 64, nkt) of sequence `seq` for its two 16-row query groups q = 0, 1:
//   kb, vb   the (layer, kv head) run of the K / V cache;  kmax: the last key any row of the
//            workgroup sees (rows past it are not loaded);  k0: first key, a multiple of 64;
//   qf       Q fragments (lane: row = lane & 15, d = 32 ks + 8 (lane >> 4) ..+7);
//   qpos     the lane's row position;  gpos: the group's last position (wave-uniform; < k0,
//            e.g. -1: the group takes no tile), gpos[1] >= gpos[0];  gmin: the group's first
//            position (a tile ending at or before it skips the causal mask; -1: always mask).
// Leaves the unnormalised O (C/D layout: row = 4 (lane >> 4) + r, d = 16 dt + (lane & 15)),
// the running max (log2 domain) and the sum of each lane's row (lane & 15).
// Dynamic LDS: 2 operands x 2 buffers x 64 keys x HD bf16.
// SPLIT: the walk may show a row no key at all (see the exponent base below).
template <int HD, bool PG, int NW, bool SPLIT>
__device__ __forceinline__ void attn_mfma_walk(const uint16_t* kb, const uint16_t* vb, const KvMap& km, const int seq,
                                               const int kmax, const int k0, const int nkt,
                                               const bf16x8_t (&qf)[2][HD / 32], const int (&qpos)[2],
                                               const int (&gpos)[2], const int (&gmin)[2], f32x4_t (&oacc)[2][HD / 16],
                                               float (&m_run)[2], float (&l_run)[2]) {
    constexpr int KT = 64;
    constexpr int CPR = HD / 8;
    constexpr int KSTEPS = HD / 32;
    constexpr int DT = HD / 16;
    constexpr int QG = 2;                  // 16-row query groups per wave
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* Ks = reinterpret_cast<uint16_t*>(smem);
    uint16_t* Vs = reinterpret_cast<uint16_t*>(smem + 2 * KT * HD * 2);
    // V image chunk swizzle: the 16-B chunk c of key row r sits at c ^ vswz(r).  A
    // ds_read_b64_tr_b16 half-wave reads 8 rows x 32 B at one column; unswizzled, the rows
    // (a whole number of 256-B bank rows apart) hit the same banks: 8-way conflicts.
    auto vswz = [](int r) { return 2 * (r & (CPR / 2 - 1)); };

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int kt0 = k0 / KT;

    // K/V tiles go global -> LDS by LDS-DMA (global_load_lds_dwordx4): one wave-instruction
    // = 1 KiB = RPI key rows, lane-linear in LDS, the chunk swizzle applied on the SOURCE
    // address (LDS position p of row r holds chunk p ^ swz(r)); no staging registers and no
    // ds_write pass.  A 64-key tile never straddles a page (page_tokens is a multiple of
    // 128); rows past kmax re-read row kmax (same page) and are masked by position.
    constexpr int RPI = 512 / HD;                 // key rows per 1 KiB wave-instruction
    constexpr int IPW = KT / RPI / NW;            // wave-instructions per wave per operand
    // Buffer loads to LDS on a per-tile resource (round 5): the lane byte offsets inside a
    // tile are constants of the launch and the tile base is scalar, so a tile's DMAs cost no
    // VALU (the flat form recomputed 64-bit addresses and the row clamp per tile: ~40 VALU).
    // The resource covers the tile's rows up to kmax only: rows past it read as zeros (their
    // keys are masked, and P = 0 times a zero V row stays 0 whatever the cache holds there).
    uint32_t koff[IPW], voff[IPW];
#pragma unroll
    for (int i = 0; i < IPW; i++) {
        const int r = (wave * IPW + i) * RPI + lane / CPR, pch = lane % CPR;
        koff[i] = (uint32_t)(r * HD + (pch ^ (r & (CPR - 1))) * 8) * 2;
        voff[i] = (uint32_t)(r * HD + (pch ^ vswz(r)) * 8) * 2;
    }
    auto issue = [&](int kt, int buf) {
        const int64_t tb = kv_tok<PG>(km, seq, kt * KT, HD);
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

#pragma unroll
    for (int q = 0; q < QG; q++)
#pragma unroll
        for (int d = 0; d < DT; d++) oacc[q][d] = f32x4_t{0.f, 0.f, 0.f, 0.f};
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
    // which of the wave's two groups take a key tile is a run of tiles per case (positions
    // are non-decreasing, and group 1 is the later one): both groups for tiles [kt0, nkt0),
    // group 1 alone up to nkt1, then barriers only up to the workgroup's nkt.  One loop per
    // case with the tile body instantiated for it: no MFMA sits behind a per-instruction
    // exec-mask branch (the compiler could not prove on[] uniform and wrapped every MFMA in
    // s_and_saveexec / s_cbranch_execz / s_or_b64), and — unlike a three-way branch inside
    // one loop — the accumulators need no register copies where the cases meet.
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
            float pv[QG][4][4];   // this tile's probabilities (fp32), split into bf16 parts at P.V
#pragma unroll
            for (int q = 0; q < QG; q++) {
                if (!ON[q]) continue;
                float (&sv)[4][4] = pv[q];
                float mt = -INFINITY;
                // (an fma form, exp2(fma(s, sl2, -m)), saves 16 VALU per tile but rounds
                // differently: config 2's 128-decision parity run then had a flip at a top-2 gap
                // 0.34 against the oracle's own 0.31 spread — not taken)
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
                // a walk from key 0 leaves m_new finite (tile 0 holds key 0 <= every position).
                // SPLIT, the one difference between the callers: a split past a row's position
                // shows it no key at all, the running max stays -inf there, and the exponent
                // base must not (-inf - -inf is NaN)
                const float m_new = fmaxf(m_run[q], mt);
                const float m_use = SPLIT && m_new == -INFINITY ? 0.f : m_new;
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
                // O *= alpha only where some row's max grew: alpha == 1 exactly otherwise
                // (exp2(0)), and the first tile's O is zero — skipping is bit-identical (a
                // wave-uniform ballot; once the running maxima settle most tiles skip the 32
                // products)
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
            // (Measured and dropped: softmax then P.V per group, so that group 1's softmax
            // could issue beside group 0's MFMAs, V fragments read per group: 76.8 vs 75.3 µs.)
            const int q4 = fr >> 2, p4 = fr & 3;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                // P = hi + lo: two bf16 parts carry 16 of the 24 mantissa bits of each fp32
                // probability; the dropped remainder is < 2^-16 of p, a relative error per
                // P.V product (<= 2^-17) below the fp32 summation-order spread of the
                // reference's own sum over keys
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
                    // rows vr and vr + 16 share vswz: one column offset serves both reads
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
    // tiles each group takes: [kt0, gpos / KT] (none when the group's last position lies
    // before k0: padding, or a split the group does not reach); gpos[1] >= gpos[0]
    const int nkt0 = gpos[0] >= k0 ? min(nkt, gpos[0] / KT + 1) : kt0;
    const int nkt1 = gpos[1] >= k0 ? min(nkt, gpos[1] / KT + 1) : kt0;
    if (nkt1 > kt0) {
        run(nkt0, std::true_type{}, std::true_type{});
        run(nkt1, std::false_type{}, std::true_type{});
    } else {
        run(nkt0, std::true_type{}, std::false_type{});
    }
    run(nkt, std::false_type{}, std::false_type{});
}

// Merge of the split partials of one (row, q head): grid (M, nq), HD threads; partials
// [M][nq][nsplit][HD] + [M][nq][nsplit][2] (running max, sum).  LOG2: the maxima are in the
// log2 domain (attn_mfma_walk's), so the weights are exp2; else natural (attn_split_kernel's).
template <int HD, bool LOG2>
__global__ __launch_bounds__(HD) void attn_combine_kernel(const float* part_o, const float* part_ml, uint16_t* out,
                                                          int nq, int nsplit) {
    const int64_t m = blockIdx.x;
    const int h = blockIdx.y, d = threadIdx.x;
    const int64_t base = (m * nq + h) * (int64_t)nsplit;
    float mn = -INFINITY;
    for (int s = 0; s < nsplit; s++) mn = fmaxf(mn, part_ml[(base + s) * 2]);
    float l = 0.f, ov = 0.f;
    for (int s = 0; s < nsplit; s++) {
        const float ms = part_ml[(base + s) * 2];
        if (ms == -INFINITY) continue;   // no visible key: its O is not read
        const float c = LOG2 ? __builtin_amdgcn_exp2f(ms - mn) : expf(ms - mn);
        l += part_ml[(base + s) * 2 + 1] * c;
        ov += part_o[(base + s) * HD + d] * c;
    }
    out[m * (int64_t)nq * HD + (int64_t)h * HD + d] = f2bf(ov / l);
}

template <bool LOG2>
inline void launch_attn_combine(int hd, int64_t M, int nq, int nsplit, const float* part_o, const float* part_ml,
                                uint16_t* out, hipStream_t st) {
    auto k = hd == 128 ? attn_combine_kernel<128, LOG2> : attn_combine_kernel<64, LOG2>;
    hipLaunchKernelGGL(k, dim3((unsigned)M, (unsigned)nq), dim3(hd), 0, st, part_o, part_ml, out, nq, nsplit);
}

}  // namespace qie
