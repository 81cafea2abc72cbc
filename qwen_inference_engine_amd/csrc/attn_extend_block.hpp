// attn_extend_block.hpp — one workgroup of the split-context MFMA attention (k_attn_extend.hip
// describes the scheme): a block of 128 flattened (token, head-in-group) rows of ONE run of
// rows of one sequence, one key split, one kv head.  attn_extend_kernel finds its run by
// m / rows_per_seq (equal runs), attn_ragged_kernel (k_attn_ragged.hip) in a table of runs of
// any lengths; everything from there on is this function, so a row's result depends only on
// its place inside its run, the key tiles it sees and the split length.
#pragma once
#include "qie_common.hpp"
#include "attn_mfma_tile.hpp"

namespace qie {

constexpr int kExtBlockRows = 128;    // flattened rows per workgroup (4 waves x 2 groups x 16)

struct ExtendAttnParams {
    const uint16_t* q;       // [M][nq*HD]
    const int32_t* pos;      // [M]; non-decreasing within each sequence's rows
    int rows_per_seq;        // (attn_extend_kernel only)
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

// The workgroup of (rows [row0, row0 + R) of the call, which belong to cache sequence seq;
// block blk of their flattened rows; split s; kv head kvh).  256 threads.  Wave w owns the
// block's 16-row groups (w, 7 - w): positions are non-decreasing in the flattened row index, so
// the pair evens out the rows' own causal triangle as in the prefill kernel; the rectangle over
// the prefix is the same for every group.
template <int HD, bool PG>
__device__ __forceinline__ void attn_extend_block(const ExtendAttnParams& a, const int seq, const int64_t row0,
                                                  const int R, const int blk, const int s, const int kvh) {
    constexpr int NW = 4;
    constexpr int KT = 64;
    constexpr int KSTEPS = HD / 32;
    constexpr int DT = HD / 16;
    constexpr int QG = 2;                  // 16-row query groups per wave
    constexpr int NGB = QG * NW;           // groups per block
    static_assert(16 * NGB == kExtBlockRows, "attn_extend: block rows");

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int G = a.nq / a.nkv;
    const int RG = R * G;                                         // flattened rows of this kv head
    const int f0 = blk * kExtBlockRows;
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
