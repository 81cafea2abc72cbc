// k_attn_shared.hip — decode attention that reads a shared prompt prefix once per group
// (cascade / Hydragen decoding; qie_attention_decode_shared).
//
// qie_attention_decode's contract with one change: keys [0, share[m].n_shared) of row m are read
// from sequence share[m].leader's rows.  Slots that hold the same prompt pages (forks, prefix-cache
// loads) form a group; the group's prefix K/V are read ONCE and meet the stacked q rows of all of
// its members, where qie_attention_decode has every slot walk its whole context by itself.
//
// Two launches.
//   1. attn_shared_kernel, grid (nkv * 2 nj, B), 256 threads.  blockIdx.x = (kv head g, role); the
//      key axis is cut into nj splits of `chunk` keys (a multiple of 128, fixed by max_ctx alone,
//      so the grid is the same for every table and one captured launch serves any of them):
//        role j < nj        PREFIX role of leader blockIdx.y, keys [j chunk, (j + 1) chunk) below the
//                           leader's n_shared, read from the leader's rows, for every member whose
//                           n_shared reaches past j chunk;
//        role nj + j        SUFFIX role of slot blockIdx.y, the keys of split j in
//                           [n_shared[m], pos[m]], read from the slot's own rows; the split that
//                           holds pos[m] appends the slot's new K/V row.
//      A block whose role is empty under the current table (not a leader, a prefix that ends
//      before the split, a split past the context) exits at once.  No block waits on another.
//   2. attn_shared_merge_kernel, grid (B, nq), head_dim threads: one log-sum-exp merge of all the
//      partials of a row; which slots of a row hold a partial follows from (share, pos) alone, so
//      the workspace is never cleared and needs no initialisation.
//
// Operand layouts of a block step (128 keys; the decode kernel's, attn_decode.hpp, with the M
// dimension widened from one slot's G = nq / nkv heads to members x G rows):
//   rows     row r = mi * G + h: head h of the group's mi-th member (ascending slot), up to 64 rows
//            = RT <= 4 MFMA row tiles of 16; the rows past members x G are zero q rows, never stored.
//            The prologue norms and rotates q of every member (dec_pro_issue / dec_pro_finish: the
//            decode kernel's arithmetic, bit for bit) into q_s [64][HD] bf16.
//   S^T      = K . Q^T: A = K rows straight from HBM into the registers of the wave that owns the
//            keys (wave w: keys 32 w .. 32 w + 31; lane: key l & 15, 8 contiguous d) — each K element
//            is loaded once per block and its fragment feeds every row tile from registers, so an
//            LDS image would add a round trip and no reuse; B = Q^T from q_s.  Raw dots / sqrt(hd)
//            go to s_s [64][128 + 4] fp32, and after one barrier every wave holds all the scores.
//   O += P.V : each wave owns HD / 4 output dims.  Its V slice of the step (128 keys x HD / 4) goes
//            global -> LDS by LDS-DMA (global_load_lds_dwordx4, lane-linear: chunk c = lane + 64 i
//            is key c / CPW, 16-byte piece c % CPW), double-buffered: the next step's slice lands
//            while this step's is read; ds_read_b64_tr_b16 fragments feed all row tiles.  P = three
//            bf16 parts of the fp32 probability, as in the decode kernel.
//   mask     shared lengths are multiples of the step, so a member whose n_shared ends before a
//            step loses the whole step (its rows' scores are -inf, P = 0: alpha = 1, nothing
//            moves); only the suffix role's last step masks single keys (past pos[m]).
// LDS: q_s 64 HD 2 + kv_new 4 HD + V 2 x 128 x HD x 2 + s_s 64 x 132 x 4 bytes = 113.6 KiB at hd 128,
// 73.3 KiB at hd 64.
//
// Workspace (qie_attention_decode_shared_workspace_bytes; fp32, no initialisation needed):
//   part_o  [B][nq][2 nj][HD]   unnormalised O of (row, head, partial slot)
//   part_ml [B][nq][2 nj][2]    running max (natural log domain) and sum
//   partial slot j < nj: prefix split j; slot nj + j: suffix split j.  Row m holds a prefix partial j
//   iff j chunk < n_shared[m], a suffix partial j iff split j meets [n_shared[m], pos[m]].
//
// The share table is device data and is sanitised where it is read (share_of): a leader outside
// [0, m], a leader that is not its own leader, or a length past a position degrade to a plain slot
// or a shorter prefix, never to a read outside [0, pos] of a live sequence.
#include "attn_decode.hpp"

#include <algorithm>
#include <climits>

namespace qie {

constexpr int kShStep = 128;      // keys per block step (4 waves x 32)
constexpr int kShSplits = 64;     // splits per phase at most: chunk = 128 ceil(steps / 64)
constexpr int kShRows = 64;       // stacked rows at most (kMaxGroup heads x 8 members)
constexpr int kMaxBatchShare = 8; // rows (slots) of a call at most

struct SharedAttnParams {
    DecodeAttnParams d;           // the decode kernel's fields (qkv, pos, norms, RoPE, cache, out)
    const qie_prefix_share* share;
    int B, nj, chunk;
};

struct ShareEnt {
    int leader, ns;
};
// entry m as the kernels use it: leader in [0, m] that leads itself, ns a multiple of 128 with
// ns <= pos[m], ns <= the leader's own sanitised length; ns == 0 <=> leader == m shares nothing
__device__ __forceinline__ ShareEnt share_of(const SharedAttnParams& a, int m) {
    int L = a.share[m].leader, ns = a.share[m].n_shared;
    int cap = a.d.pos[m];
    if (L < 0 || L > m) L = m;
    if (L != m) {
        const qie_prefix_share le = a.share[L];
        if (le.leader != L) return ShareEnt{m, 0};
        cap = min(cap, min(le.n_shared, a.d.pos[L]));
    }
    ns = max(min(ns, cap), 0) & ~(kShStep - 1);
    return ShareEnt{ns == 0 ? m : L, ns};
}

// The key walk of one block: keys [t0, t1) of cache sequence `seq` for nrows stacked rows (row r
// belongs to slot mem_s[r / G] and sees the keys below ns_s[r / G]); p_new >= 0: the key at p_new
// is the row appended by this block (its K / V come from kv_new, and the V rows from p_new on are
// past the context).  Writes the partials of slot `pslot` of every row.
template <int HD, bool PG, int RT>
__device__ __forceinline__ void shared_walk(const SharedAttnParams& a, const int g, const int seq, const int t0,
                                            const int t1, const int p_new, const int nrows, const int minlim,
                                            const int pslot, uint16_t (*q_s)[HD], uint16_t (*kv_new)[HD],
                                            uint16_t* v_s, float (*s_s)[kShStep + 4], const int* mem_s,
                                            const int* ns_s) {
#pragma clang fp contract(off)
    constexpr int KS = kShStep, NWA = 4;
    constexpr int KSTEPS = HD / 32;      // MFMA k-steps over d for S
    constexpr int DW = HD / NWA;         // output dims per wave
    constexpr int DTW = DW / 16;         // output d tiles per wave
    constexpr int CPW = DW / 8;          // 16-byte chunks of a V row per wave
    constexpr int VCH = KS * CPW / 64;   // V chunks per lane per step
    constexpr int TPW = KS / (16 * NWA); // 16-key S tiles per wave per step
    const DecodeAttnParams& d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, gq = lane >> 4;
    const int G = d.nq / d.nkv;
    const int nrt = (nrows + 15) / 16;   // row tiles in use (uniform)
    const int64_t head_off = kv_run_off(d.km, (int64_t)d.layer * d.nkv + g, HD);
    const uint16_t* kb = d.kc + head_off;
    const uint16_t* vb = d.vc + head_off;
    const int last = t1 - 1;
    uint4 kf[TPW][KSTEPS];
    // a 128-key step never straddles a page (steps start at multiples of 128, pages are powers of
    // two >= 128); rows past `last` re-read row `last`
    auto load_k = [&](int kb0) {
        const int64_t so = kv_tok<PG>(d.km, seq, kb0, HD);
#pragma unroll
        for (int t = 0; t < TPW; t++) {
            const int key = min(kb0 + 16 * TPW * wave + 16 * t + fr, last);
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ks++)
                kf[t][ks] = *reinterpret_cast<const uint4*>(kb + so + (int64_t)(key - kb0) * HD + 32 * ks + 8 * gq);
        }
    };
    // this wave's V slice of the step -> its slot of buffer `buf` (lane-linear: chunk c at 16 c bytes)
    auto dma_v = [&](int kb0, int buf) {
        const int64_t so = kv_tok<PG>(d.km, seq, kb0, HD);
        uint16_t* vw = v_s + (buf * NWA + wave) * (KS * DW);
#pragma unroll
        for (int i = 0; i < VCH; i++) {
            const int c = lane + 64 * i;
            const int key = min(kb0 + c / CPW, last);
            dma16(vb + so + (int64_t)(key - kb0) * HD + wave * DW + (c % CPW) * 8, vw + 512 * i);
        }
    };
    load_k(t0);
    dma_v(t0, 0);

    // this lane's row of each tile (S^T B operand and softmax: row 16 rt + fr) and its key limit
    bf16x8_t qb[RT][KSTEPS];
    int rlim[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        const int r = 16 * rt + fr;
        rlim[rt] = r < nrows ? ns_s[r / G] : INT_MAX;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++)
            qb[rt][ks] = *reinterpret_cast<const bf16x8_t*>(&q_s[rt < nrt ? r : fr][32 * ks + 8 * gq]);
    }
    uint4 knew[KSTEPS];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++) knew[ks] = *reinterpret_cast<const uint4*>(&kv_new[0][32 * ks + 8 * gq]);
    const float scale = sqrtf((float)HD);
    const float inv_scale = 1.0f / scale;
    // dot / sqrt(hd), correctly rounded (attn_decode.hpp qdiv)
    auto qdiv = [&](float x) {
        const float q = x * inv_scale;
        if constexpr (HD == 64) return q;
        else return fmaf(fmaf(-q, scale, x), inv_scale, q);
    };
    float m_run[RT], l_run[RT];
    f32x4_t oacc[RT][DTW];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        m_run[rt] = -INFINITY;
        l_run[rt] = 0.f;
#pragma unroll
        for (int dt = 0; dt < DTW; dt++) oacc[rt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const int q4 = fr >> 2, p4 = fr & 3;
    const int nstep = (t1 - t0 + KS - 1) / KS;

    for (int st = 0; st < nstep; st++) {
        const int kb0 = t0 + st * KS;
        uint16_t* vw = v_s + ((st & 1) * NWA + wave) * (KS * DW);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this step's K fragments and V slice
        const bool hasp = p_new >= kb0 && p_new < kb0 + KS;
        if (hasp) {
#pragma unroll
            for (int t = 0; t < TPW; t++) {
                const bool nw = kb0 + 16 * TPW * wave + 16 * t + fr == p_new;
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ks++) kf[t][ks] = sel4(nw, knew[ks], kf[t][ks]);
            }
            // the V rows from p_new on re-read cache row p_new, loaded before this launch's append
            // lands — any bits (NaN bits gave 0 * NaN in P.V).  They take the new row: P = 0 past it
#pragma unroll
            for (int i = 0; i < VCH; i++) {
                const int c = lane + 64 * i;
                if (kb0 + c / CPW >= p_new)
                    *reinterpret_cast<uint4*>(vw + c * 8) =
                        *reinterpret_cast<const uint4*>(&kv_new[1][wave * DW + (c % CPW) * 8]);
            }
        }
        // ---- S^T of this wave's 32 keys against every row tile -> LDS
#pragma unroll
        for (int t = 0; t < TPW; t++) {
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                if (rt >= nrt) continue;
                f32x4_t sacc = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ks++)
                    sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kf[t][ks]), qb[rt][ks],
                                                                   sacc, 0, 0, 0);
                // C map: col = row fr of the tile, rows = keys 4 gq + r of the key tile
                *reinterpret_cast<float4*>(&s_s[16 * rt + fr][16 * TPW * wave + 16 * t + 4 * gq]) =
                    make_float4(qdiv(sacc[0]), qdiv(sacc[1]), qdiv(sacc[2]), qdiv(sacc[3]));
            }
        }
        if (st + 1 < nstep) {   // into the other V buffer: its readers passed the last barrier
            load_k(kb0 + KS);
            dma_v(kb0 + KS, (st + 1) & 1);
        }
        __syncthreads();   // scores visible
        const bool full = kb0 + KS <= minlim;   // uniform: every row sees every key of the step
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
            if (rt >= nrt) continue;
            // online softmax of row 16 rt + fr over the step's keys 32 c + 8 gq + j
            float e[KS / 32][8];
#pragma unroll
            for (int c = 0; c < KS / 32; c++) {
                const float4 lo = *reinterpret_cast<const float4*>(&s_s[16 * rt + fr][32 * c + 8 * gq]);
                const float4 hi = *reinterpret_cast<const float4*>(&s_s[16 * rt + fr][32 * c + 8 * gq + 4]);
                e[c][0] = lo.x; e[c][1] = lo.y; e[c][2] = lo.z; e[c][3] = lo.w;
                e[c][4] = hi.x; e[c][5] = hi.y; e[c][6] = hi.z; e[c][7] = hi.w;
            }
            if (!full) {
#pragma unroll
                for (int c = 0; c < KS / 32; c++)
#pragma unroll
                    for (int j = 0; j < 8; j++)
                        if (kb0 + 32 * c + 8 * gq + j >= rlim[rt]) e[c][j] = -INFINITY;
            }
            float mt = -INFINITY;
#pragma unroll
            for (int c = 0; c < KS / 32; c++)
#pragma unroll
                for (int j = 0; j < 8; j++) mt = fmaxf(mt, e[c][j]);
            mt = xor32_max(xor16_max(mt));
            const float m_new = fmaxf(m_run[rt], mt);
            const float m_use = m_new == -INFINITY ? 0.f : m_new;
            const float alpha = __expf(m_run[rt] - m_use);
            float ls = 0.f;
#pragma unroll
            for (int c = 0; c < KS / 32; c++)
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    e[c][j] = __expf(e[c][j] - m_use);
                    ls += e[c][j];
                }
            ls = xor32_sum(xor16_sum(ls));
            l_run[rt] = l_run[rt] * alpha + ls;
            m_run[rt] = m_new;
            // alpha == 1 exactly where no row's max grew, and step 0's O is zero: skipping is bit-identical
            if (st > 0 && __builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
                float ar[4];
#pragma unroll
                for (int r = 0; r < 4; r++) ar[r] = __shfl(alpha, gq * 4 + r, 64);
#pragma unroll
                for (int dt = 0; dt < DTW; dt++)
#pragma unroll
                    for (int r = 0; r < 4; r++) oacc[rt][dt][r] *= ar[r];
            }
            // O[rows of the tile][this wave's dims] += P . V, P = hi + mid + lo (all 24 bits)
#pragma unroll
            for (int c = 0; c < KS / 32; c++) {
                uint4 pp[3];
                split_bf16x8<3>(e[c], pp);
                const bf16x8_t ph = __builtin_bit_cast(bf16x8_t, pp[0]), pm = __builtin_bit_cast(bf16x8_t, pp[1]),
                               pl = __builtin_bit_cast(bf16x8_t, pp[2]);
#pragma unroll
                for (int dt = 0; dt < DTW; dt++) {
                    const uint16_t* a0 = vw + (32 * c + 8 * gq + q4) * DW + 16 * dt + 4 * p4;
                    const i16x4_t v0 =
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4_t*)(a0));
                    const i16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) i16x4_t*)(a0 + 4 * DW));
                    const bf16x8_t vb8 =
                        __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
                    oacc[rt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, vb8, oacc[rt][dt], 0, 0, 0);
                    oacc[rt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pm, vb8, oacc[rt][dt], 0, 0, 0);
                    oacc[rt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl, vb8, oacc[rt][dt], 0, 0, 0);
                }
            }
        }
        __syncthreads();   // scores free for the next step
    }

    // ---- the partials of slot pslot: O rows 4 gq + r of each tile, this wave's dims; (m, l) by wave 0
    const int n2 = 2 * a.nj;
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        if (rt >= nrt) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 16 * rt + 4 * gq + r;
            if (row >= nrows) continue;
            const int64_t pi = ((int64_t)mem_s[row / G] * d.nq + g * G + row % G) * n2 + pslot;
#pragma unroll
            for (int dt = 0; dt < DTW; dt++) d.part_o[pi * HD + wave * DW + 16 * dt + fr] = oacc[rt][dt][r];
        }
        const int row = 16 * rt + fr;
        if (wave == 0 && gq == 0 && row < nrows) {
            const int64_t pi = ((int64_t)mem_s[row / G] * d.nq + g * G + row % G) * n2 + pslot;
            d.part_ml[pi * 2] = m_run[rt];
            d.part_ml[pi * 2 + 1] = l_run[rt];
        }
    }
}

template <int HD, bool PG, bool PR>
__global__ __launch_bounds__(256) void attn_shared_kernel(SharedAttnParams a) {
    constexpr int KS = kShStep, NWA = 4;
    constexpr int LPT = HD / 8;          // prologue: lanes per head row
    constexpr int GP = 256 / LPT;        // head rows per prologue pass
    constexpr int CPR = HD / 8;
    __shared__ __attribute__((aligned(16))) uint16_t q_s[kShRows][HD];
    __shared__ __attribute__((aligned(16))) uint16_t kv_new[2][HD];
    __shared__ __attribute__((aligned(16))) uint16_t v_s[2 * NWA * KS * (HD / NWA)];
    __shared__ __attribute__((aligned(16))) float s_s[kShRows][KS + 4];
    __shared__ int mem_s[kMaxBatchShare], ns_s[kMaxBatchShare], nmem_s;

    const DecodeAttnParams& d = a.d;
    const int nj = a.nj;
    const int g = blockIdx.x / (2 * nj), role = blockIdx.x % (2 * nj);
    const int by = blockIdx.y;
    const bool prefix = role < nj;
    const int j = prefix ? role : role - nj;
    const int G = d.nq / d.nkv;
    const int tid = threadIdx.x;
    const int grp = tid / LPT, dl = tid % LPT;
    const int QKVD = (d.nq + 2 * d.nkv) * HD;
    const ShareEnt me = share_of(a, by);
    const int p = d.pos[by];
    const int64_t head_off = kv_run_off(d.km, (int64_t)d.layer * d.nkv + g, HD);

    int t0, t1, p_new = -1, nrows, minlim;
    if (prefix) {
        // ---------------- prefix role: the members of leader `by` that reach split j
        t0 = j * a.chunk;
        if (me.leader != by || me.ns <= t0) return;
        t1 = min(t0 + a.chunk, me.ns);
        if (tid == 0) {
            int n = 0;
            for (int m = by; m < a.B; m++) {
                const ShareEnt e = share_of(a, m);
                if (e.leader == by && e.ns > t0) {
                    mem_s[n] = m;
                    ns_s[n] = e.ns;
                    n++;
                }
            }
            nmem_s = n;
        }
        __syncthreads();
        const int nmem = nmem_s;
        nrows = nmem * G;
        minlim = INT_MAX;
        for (int i = 0; i < nmem; i++) minlim = min(minlim, ns_s[i]);
        // q of every member, normed and rotated at ITS position: GP head rows per pass
        for (int r0 = 0; r0 < nrows; r0 += GP) {
            const int r = r0 + grp;
            const bool on = r < nrows;
            const int mi = on ? r / G : 0;
            const int slot = mem_s[mi];
            const int ps = d.pos[slot];
            DecPro pr = dec_pro_issue<HD, PR>(d, d.qkv + slot * (int64_t)QKVD, g, G, on ? r % G : G + 2, dl,
                                              d.cs + (int64_t)ps * (HD / 2), d.sn + (int64_t)ps * (HD / 2), false);
            dec_pro_finish<HD, PR>(d, pr, dl, on ? r % G : G + 2, 0, nullptr, nullptr, q_s + mi * G, kv_new);
        }
    } else {
        // ---------------- suffix role: split j of slot `by` within [n_shared, pos]
        t0 = max(j * a.chunk, me.ns);
        t1 = min((j + 1) * a.chunk, p + 1);
        if (t0 >= t1) return;
        const bool has_new = t1 == p + 1;
        if (has_new) p_new = p;
        if (tid == 0) {
            mem_s[0] = by;
            ns_s[0] = t1;
            nmem_s = 1;
        }
        nrows = G;
        minlim = t1;
        uint16_t* kb = d.kc + head_off;
        uint16_t* vb = d.vc + head_off;
        DecPro pr = dec_pro_issue<HD, PR>(d, d.qkv + by * (int64_t)QKVD, g, G, grp, dl, d.cs + (int64_t)p * (HD / 2),
                                          d.sn + (int64_t)p * (HD / 2), has_new);
        dec_pro_finish<HD, PR>(d, pr, dl, grp, kv_tok<PG>(d.km, by, p, HD), kb, vb, q_s, kv_new);
    }
    const int npad = ((nrows + 15) / 16) * 16 - nrows;   // zero q rows up to the last tile in use
    for (int idx = tid; idx < npad * CPR; idx += 256)
        *reinterpret_cast<uint4*>(&q_s[nrows + idx / CPR][(idx % CPR) * 8]) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const int seq = by;   // the prefix role reads the leader's rows, the suffix role the slot's own
    const int pslot = prefix ? j : nj + j;
    if (nrows <= 16)
        shared_walk<HD, PG, 1>(a, g, seq, t0, t1, p_new, nrows, minlim, pslot, q_s, kv_new, v_s, s_s, mem_s, ns_s);
    else
        shared_walk<HD, PG, 4>(a, g, seq, t0, t1, p_new, nrows, minlim, pslot, q_s, kv_new, v_s, s_s, mem_s, ns_s);
}

// One log-sum-exp merge of every partial of (row m, head h): grid (B, nq), HD threads.
template <int HD>
__global__ __launch_bounds__(HD) void attn_shared_merge_kernel(SharedAttnParams a) {
    __shared__ float m_s[2 * kShSplits], l_s[2 * kShSplits];
    const DecodeAttnParams& d = a.d;
    const int m = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const int nj = a.nj, n2 = 2 * nj;
    const ShareEnt me = share_of(a, m);
    const int p = d.pos[m];
    const int64_t base = ((int64_t)m * d.nq + h) * n2;
    for (int s = t; s < n2; s += HD) {
        const int j = s < nj ? s : s - nj;
        const bool on = s < nj ? j * a.chunk < me.ns : max(j * a.chunk, me.ns) < min((j + 1) * a.chunk, p + 1);
        m_s[s] = on ? d.part_ml[(base + s) * 2] : -INFINITY;
        l_s[s] = on ? d.part_ml[(base + s) * 2 + 1] : 0.f;
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int s = 0; s < n2; s++) mx = fmaxf(mx, m_s[s]);
    float ls = 0.f, acc = 0.f;
    for (int s = 0; s < n2; s++) {
        if (m_s[s] == -INFINITY) continue;   // no partial there (uniform)
        const float c = __expf(m_s[s] - mx);
        ls = fmaf(l_s[s], c, ls);
        acc = fmaf(c, d.part_o[(base + s) * HD + t], acc);
    }
    // divided (not multiplied by 1 / l): the softmax normalisation's one rounding
    d.out[(int64_t)m * d.nq * HD + (int64_t)h * HD + t] = f2bf(acc / ls);
}

// the split of the key axis: `chunk` keys per split (a function of max_ctx alone), nj splits
static void shared_split(int max_ctx, int* chunk, int* nj) {
    const int steps = (max_ctx + kShStep - 1) / kShStep;
    const int per = (steps + kShSplits - 1) / kShSplits;
    *chunk = kShStep * per;
    *nj = (steps + per - 1) / per;
}

}  // namespace qie

using namespace qie;

extern "C" {

int64_t qie_attention_decode_shared_workspace_bytes(int64_t B, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim,
                                                    int32_t max_ctx) {
    (void)n_kv_heads;
    if (B <= 0 || n_heads <= 0 || head_dim <= 0 || max_ctx <= 0) return 0;
    int chunk, nj;
    shared_split(max_ctx, &chunk, &nj);
    return ((B * n_heads * 2 * nj * (int64_t)(head_dim + 2) * 4 + 255) / 256) * 256;
}

int qie_attention_decode_shared(const void* qkv, int64_t B, const int32_t* pos, const qie_prefix_share* share,
                                const void* q_norm, const void* k_norm, const float* rope_cos, const float* rope_sin,
                                int32_t n_heads, const qie_kv_cache* cache, int32_t layer, float eps, int32_t numerics,
                                void* out, void* ws, void* stream) {
    const char* who = "qie_attention_decode_shared";
    QIE_REQUIRE(qkv && pos && share && cache && cache->k && cache->v && rope_cos && rope_sin && out, "%s: bad arguments",
                who);
    QIE_REQUIRE(ws, "%s: needs a workspace of qie_attention_decode_shared_workspace_bytes()", who);
    QIE_REQUIRE(B >= 1 && B <= kMaxBatchShare, "%s: B must be in [1, %d] (got %lld)", who, kMaxBatchShare, (long long)B);
    QIE_REQUIRE(cache->head_dim == 64 || cache->head_dim == 128, "%s: head_dim must be 64 or 128 (got %d)", who,
                cache->head_dim);
    QIE_REQUIRE(cache->n_kv_heads > 0 && n_heads > 0 && n_heads % cache->n_kv_heads == 0 &&
                    n_heads / cache->n_kv_heads <= kMaxGroup,
                "%s: n_heads/n_kv_heads must be an integer <= %d", who, kMaxGroup);
    QIE_REQUIRE(layer >= 0 && layer < cache->n_layers, "%s: bad layer", who);
    SharedAttnParams a{};
    DecodeAttnParams& d = a.d;
    d.qkv = (const uint16_t*)qkv;
    d.pos = pos;
    d.q_norm = (const uint16_t*)q_norm;
    d.k_norm = (const uint16_t*)k_norm;
    d.cs = rope_cos;
    d.sn = rope_sin;
    d.kc = (uint16_t*)cache->k;
    d.vc = (uint16_t*)cache->v;
    QIE_TRY(kv_map_make(cache, &d.km, who));
    d.layer = layer;
    d.nkv = cache->n_kv_heads;
    d.nq = n_heads;
    d.max_ctx = cache->max_ctx;
    d.eps = eps;
    d.numerics = numerics & QIE_NUMERICS_MASK;
    d.pre_roped = (numerics & QIE_ATTN_PREROPED) != 0;
    QIE_REQUIRE(!d.pre_roped || (q_norm == nullptr && k_norm == nullptr && d.numerics == QIE_NUMERICS_REF),
                "%s: QIE_ATTN_PREROPED needs REF numerics without qk-norm", who);
    a.share = share;
    a.B = (int)B;
    shared_split(cache->max_ctx, &a.chunk, &a.nj);
    d.part_o = (float*)ws;
    d.part_ml = d.part_o + B * n_heads * 2 * a.nj * (int64_t)cache->head_dim;
    d.out = (uint16_t*)out;
    const bool pg = d.km.table != nullptr, pr = d.pre_roped != 0;
    auto k = cache->head_dim == 128
                 ? (pr ? (pg ? attn_shared_kernel<128, true, true> : attn_shared_kernel<128, false, true>)
                       : (pg ? attn_shared_kernel<128, true, false> : attn_shared_kernel<128, false, false>))
                 : (pr ? (pg ? attn_shared_kernel<64, true, true> : attn_shared_kernel<64, false, true>)
                       : (pg ? attn_shared_kernel<64, true, false> : attn_shared_kernel<64, false, false>));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k, dim3((unsigned)(d.nkv * 2 * a.nj), (unsigned)B), dim3(256), 0, st, a);
    QIE_LAUNCH_CHECK();
    auto km = cache->head_dim == 128 ? attn_shared_merge_kernel<128> : attn_shared_merge_kernel<64>;
    hipLaunchKernelGGL(km, dim3((unsigned)B, (unsigned)n_heads), dim3(cache->head_dim), 0, st, a);
    QIE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
