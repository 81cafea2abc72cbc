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
// ... on an fp8 KV cache (attn_extend_fp8_kernel): kc / vc point at e4m3 codes, km counts bytes
struct ExtendAttnParams8 : ExtendAttnParams {
    Kv8Exps ex;
};
// ... for the rows of a draft tree (attn_extend_tree_kernel, k_verify_tree.hip): ONE run of M <= 16
// rows whose K/V sit at cache rows p + i (pos[i] = p + i), row i seeing the prefix [0, p) and the
// rows p + j of its ancestors-or-self j (bit j of anc[i])
struct ExtendTreeParams : ExtendAttnParams {
    const int32_t* anc;   // [M]
};

// attn_mfma_walk's visibility policy of those rows.  Every tile from the one that holds row p on
// is masked, for every group (the walk's gmin = p - 1), and its V fragments are scrubbed.
struct VisTree {
    static constexpr bool kScrubV = true;
    int p;             // the run's first cache row
    uint32_t anc[2];   // the lane's row's mask, per query group
    __device__ __forceinline__ bool sees(int q, int key, int) const {
        return key < p || ((unsigned)(key - p) < 16u && ((anc[q] >> (key - p)) & 1u));
    }
    __device__ __forceinline__ bool scrubs(int last_key) const { return last_key >= p; }
};

// The workgroup of (rows [row0, row0 + R) of the call, which belong to cache sequence seq;
// block blk of their flattened rows; split s; kv head kvh).  256 threads.  Wave w owns the
// block's 16-row groups (w, 7 - w): positions are non-decreasing in the flattened row index, so
// the pair evens out the rows' own causal triangle as in the prefill kernel; the rectangle over
// the prefix is the same for every group.
// KV8 (P = ExtendAttnParams8): the walk reads an fp8 cache (attn_mfma_walk's KV8 form); rows,
// splits, partials and stores are the same code.
// TREE (P = ExtendTreeParams): the run is a draft tree.  Every row walks the tiles up to the run's
// last row p + R - 1 (a sibling's row may lie before an ancestor's), under VisTree; rows, splits,
// partials and stores are the same code, and a chain (anc[i] = bits 0 .. i) gives every row the
// scores, maxima and sums of the causal form: a tile that shows a row no key leaves its running
// statistics and its O as they were.
template <int HD, bool PG, bool KV8 = false, bool TREE = false, class P>
__device__ __forceinline__ void attn_extend_block(const P& a, const int seq, const int64_t row0, const int R,
                                                  const int blk, const int s, const int kvh) {
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
    const int kmax = __builtin_amdgcn_readfirstlane(a.pos[row0 + (TREE ? R - 1 : (min(f0 + kExtBlockRows, RG) - 1) / G)]);
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
    // (KV8: offsets are in elements = bytes)
    const uint16_t* kb = KV8 ? reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(a.kc) + head_off)
                             : a.kc + head_off;
    const uint16_t* vb = KV8 ? reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(a.vc) + head_off)
                             : a.vc + head_off;

    const int grp[QG] = {wave, NGB - 1 - wave};
    bool gact[QG];
    int qpos[QG], gpos[QG], gmin[QG];
    bf16x8_t qf[QG][KSTEPS];
    std::conditional_t<TREE, VisTree, VisCausal> vis{};
    if constexpr (TREE) vis.p = __builtin_amdgcn_readfirstlane(a.pos[row0]);
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
        if constexpr (TREE) {
            gpos[q] = gact[q] ? kmax : -1;
            gmin[q] = __builtin_amdgcn_readfirstlane(a.pos[row0]) - 1;
            vis.anc[q] = (uint32_t)a.anc[row0 + t];
        }
        const uint16_t* qp = a.q + (row0 + t) * (int64_t)a.nq * HD + (int64_t)(kvh * G + hq) * HD;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) qf[q][ks] = *reinterpret_cast<const bf16x8_t*>(qp + ks * 32 + g * 8);
    }

    f32x4_t oacc[QG][DT];
    float m_run[QG], l_run[QG];
    if constexpr (KV8)
        attn_mfma_walk<HD, PG, NW, true, true>(kb, vb, a.km, seq, kmax, k0, nkt, qf, qpos, gpos, gmin, oacc, m_run, l_run,
                                               &a.ex, kv_run_off(a.ex.em, (int64_t)a.layer * a.nkv + kvh, 1));
    else if constexpr (TREE)
        attn_mfma_walk<HD, PG, NW, true, false, VisTree>(kb, vb, a.km, seq, kmax, k0, nkt, qf, qpos, gpos, gmin, oacc, m_run,
                                                         l_run, nullptr, 0, vis);
    else
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
