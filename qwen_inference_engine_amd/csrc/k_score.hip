// k_score.hip — per-token log-probabilities of the vocabulary head (qie_ops.h "scoring").
//
// The reference has no scoring path: its head (qwen_main.cu:224-241) samples one token from the
// last row.  Contract: a row's logits l[j] are the head's bf16 logits; everything
// after is fp32 on those values,
//     lse = m + logf(sum_j expf(l[j] - m)),  m = max_j l[j],   logprob(t) = l[t] - lse,
// the row's greedy id is the maximum sel_key (the reference tie rule), partial sums are merged in
// a fixed index order (no float atomics: two runs are bit-identical) and no kernel waits on
// another workgroup (the merge of the fused form is a second launch).
//   qie_logprob_rows   over materialised bf16 logit rows, one workgroup per row
//   qie_score_rows     fused: the 256x256 tile pipeline of gemm8_tile.hpp over x [M, K] . W [V, K]^T
//                      whose epilogue reduces each tile row to {max, sum exp, key} instead of
//                      storing it (score_tile_kernel), then one wave per row merging the column
//                      tiles' partials (score_merge_kernel).  Nothing of size M x V is written.
#include "qie_common.hpp"
#include "launch_util.hpp"
#include "gemm8_tile.hpp"
#include "../../include/qie/qie_ops.h"

namespace qie {

// sel_key in halves: the high word orders by value (0: NaN / -inf, never selected), the low
// word breaks ties (bitrev8(idx mod 256), then the smaller idx); never 0 for idx < 2^24 - 1
__device__ __forceinline__ uint32_t key_ord(float v) {
    if (!(v > -INFINITY)) return 0u;
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t key_low(uint32_t idx) {
    return ((__builtin_bitreverse32(idx & 0xffu) >> 24) << 24) | ((~idx) & 0xffffffu);
}
__device__ __forceinline__ float ord_val(uint32_t ord) {
    return ord ? __uint_as_float((ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord) : -INFINITY;
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// max over the aligned 16-lane row (qie_common.hpp group_max, on unsigned words)
__device__ __forceinline__ uint32_t row16_max_u(uint32_t v) {
    v = max(v, dpp_u<0xB1>(v));
    v = max(v, dpp_u<0x4E>(v));
    v = max(v, dpp_u<0x141>(v));
    v = max(v, dpp_u<0x140>(v));
    return v;
}

// ------------------------------------------------------------------ materialised rows
// One workgroup per row (1,024 threads: the callers have at most 16 rows, and a row is 300 KB at
// Qwen2's vocabulary): pass 1 the maximum key (its value is the row maximum), pass 2 the sum of
// expf(l - m), each thread over its elements in index order, then the fixed wave / block tree.
constexpr int kLpThreads = 1024, kLpWaves = kLpThreads / 64;
__global__ __launch_bounds__(kLpThreads) void logprob_rows_kernel(const uint16_t* __restrict__ logits, int64_t V, int64_t ld,
                                                           const int32_t* __restrict__ targets,
                                                           float* __restrict__ logprobs, int32_t* __restrict__ ids) {
#pragma clang fp contract(off)
    __shared__ unsigned long long kred[kLpWaves];
    __shared__ float sred[kLpWaves];
    const int64_t m = blockIdx.x;
    const uint16_t* row = logits + m * ld;
    const int tid = threadIdx.x;
    const bool vec = (ld % 8 == 0) && ((uintptr_t)logits % 16 == 0);   // uniform
    const int64_t V8 = vec ? V / 8 : 0;

    unsigned long long best = 0ull;
    for (int64_t c = tid; c < V8; c += kLpThreads) {
        const uint4 q = *reinterpret_cast<const uint4*>(row + c * 8);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned long long k0 = sel_key(bf_lo(w[j]), (uint32_t)(c * 8 + 2 * j));
            const unsigned long long k1 = sel_key(bf_hi(w[j]), (uint32_t)(c * 8 + 2 * j + 1));
            best = k0 > best ? k0 : best;
            best = k1 > best ? k1 : best;
        }
    }
    for (int64_t i = V8 * 8 + tid; i < V; i += kLpThreads) {
        const unsigned long long k = sel_key(bf2f(row[i]), (uint32_t)i);
        best = k > best ? k : best;
    }
    best = wave_max(best);
    if ((tid & 63) == 0) kred[tid >> 6] = best;
    __syncthreads();
    best = kred[0];
#pragma unroll
    for (int w = 1; w < kLpWaves; w++) best = kred[w] > best ? kred[w] : best;
    const float mx = best ? key_val(best) : -INFINITY;

    float s = 0.f;
    if (best) {
        for (int64_t c = tid; c < V8; c += kLpThreads) {
            const uint4 q = *reinterpret_cast<const uint4*>(row + c * 8);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s += expf(bf_lo(w[j]) - mx);
                s += expf(bf_hi(w[j]) - mx);
            }
        }
        for (int64_t i = V8 * 8 + tid; i < V; i += kLpThreads) s += expf(bf2f(row[i]) - mx);
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) sred[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        float S = sred[0];
        for (int w = 1; w < kLpWaves; w++) S += sred[w];   // wave order
        const int32_t t = targets[m];
        logprobs[m] = (t < 0 || t >= V) ? 0.0f : bf2f(row[t]) - (mx + logf(S));
        if (ids) ids[m] = key_idx(best);
    }
}

// ------------------------------------------------------------------ fused form
// Workspace of qie_score_rows: keys [n_nt][M] u64, {m, s} [n_nt][M] float2, tgt [M] float
struct ScoreWs {
    unsigned long long* keys;
    float2* ms;
    float* tgt;
};
__host__ __device__ inline int64_t score_n_nt(int64_t V) { return (V + g8::BN - 1) / g8::BN; }

struct ScoreParams {
    const uint16_t* x;
    int64_t ldx;
    const uint16_t* W;
    int64_t M, K, V;
    const int32_t* targets;
    ScoreWs ws;
};

// one (wave, row) partial of the cross-wave merge in LDS
struct ScorePart {
    uint32_t ord, low;
    float s;
};

__global__ __launch_bounds__(512) void score_tile_kernel(ScoreParams p, int n_mt) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const G8Lane l = g8_lane();
    const int wid = xcd_major_wid();
    const int64_t mt = wid % n_mt, nt = wid / n_mt;
    const int64_t m0 = mt * g8::BM, n0 = nt * g8::BN;

    G8Bf16 op;
    op.map(l, [&](int u, int i, int r, int cs) {
        if (u == 0 || u == 3) {
            int64_t ar = m0 + r;
            ar = ar < p.M ? ar : p.M - 1;   // rows past M: re-read row M-1, never used
            op.src[u][i] = p.x + ar * p.ldx + cs * 8;
        } else {
            int64_t wr = n0 + r;
            wr = wr < p.V ? wr : p.V - 1;   // weight rows past V: re-read row V-1, masked below
            op.src[u][i] = p.W + wr * p.K + cs * 8;
        }
    });
    f32x4 acc[8][4];
    g8_pipeline<false>(op, l, smem, (int)(p.K / g8::BK), acc);   // K >= 256: nk >= 4

    // Every wave is past the pipeline's last barrier and every DMA has landed: the staging
    // buffers are free.  acc[i][j][r] = row 128 wm + 16 i + 4 g + r, column 64 wn + 16 j + fr.
    ScorePart* part = reinterpret_cast<ScorePart*>(smem);   // [256 rows][4 column waves]
    uint32_t low[4];
    bool cv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t col = n0 + 64 * l.wn + 16 * j + l.fr;
        cv[j] = col < p.V;
        low[j] = key_low((uint32_t)col);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int trow = 128 * l.wm + 16 * i + 4 * l.g + r;
            const int64_t row = m0 + trow;
            const int32_t t = p.targets[row < p.M ? row : p.M - 1];
            float v[4];
            uint32_t o[4], mo = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                v[j] = rbf(acc[i][j][r]);
                o[j] = cv[j] ? key_ord(v[j]) : 0u;
                mo = max(mo, o[j]);
                if (row < p.M && cv[j] && (int64_t)t == n0 + 64 * l.wn + 16 * j + l.fr) p.ws.tgt[row] = v[j];
            }
            mo = row16_max_u(mo);
            const float mx = ord_val(mo);
            uint32_t lo = 0u;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (o[j] == mo) lo = max(lo, low[j]);
                s += cv[j] && mo ? expf(v[j] - mx) : 0.f;
            }
            lo = mo ? row16_max_u(lo) : 0u;
            s = group_sum<16>(s);
            if (l.fr == 0) part[trow * 4 + l.wn] = ScorePart{mo, lo, s};
        }
    }
    __syncthreads();
    if (l.tid < g8::BM && m0 + l.tid < p.M) {   // the four column waves of row tid, in wave order
        const ScorePart* q = part + l.tid * 4;
        unsigned long long key = 0ull;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const unsigned long long k = ((unsigned long long)q[w].ord << 32) | q[w].low;
            key = k > key ? k : key;
        }
        const float mx = ord_val((uint32_t)(key >> 32));
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 4; w++) s += q[w].ord ? q[w].s * expf(ord_val(q[w].ord) - mx) : 0.f;
        const int64_t o = nt * p.M + m0 + l.tid;
        p.ws.keys[o] = key;
        p.ws.ms[o] = make_float2(mx, s);
    }
}

// one wave per row: the n_nt column-tile partials, each lane over its tiles in index order
__global__ __launch_bounds__(256) void score_merge_kernel(ScoreWs ws, int64_t M, int64_t V, int n_nt,
                                                          const int32_t* __restrict__ targets,
                                                          float* __restrict__ logprobs, int32_t* __restrict__ ids) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;   // wave-uniform
    unsigned long long key = 0ull;
    for (int i = lane; i < n_nt; i += 64) {
        const unsigned long long k = ws.keys[(int64_t)i * M + m];
        key = k > key ? k : key;
    }
    key = wave_max(key);
    const float mx = key ? key_val(key) : -INFINITY;
    float s = 0.f;
    if (key)
        for (int i = lane; i < n_nt; i += 64) {
            const float2 q = ws.ms[(int64_t)i * M + m];
            s += q.y > 0.f ? q.y * expf(q.x - mx) : 0.f;
        }
    s = wave_sum(s);
    if (lane == 0) {
        const int32_t t = targets[m];
        logprobs[m] = (t < 0 || t >= V) ? 0.0f : ws.tgt[m] - (mx + logf(s));
        if (ids) ids[m] = key_idx(key);
    }
}

static ScoreWs score_ws(void* ws, int64_t M, int64_t V) {
    const int64_t n = score_n_nt(V) * M;
    char* b = (char*)ws;
    return ScoreWs{(unsigned long long*)b, (float2*)(b + n * 8), (float*)(b + n * 16)};
}

}  // namespace qie

using namespace qie;

extern "C" {

int qie_logprob_rows(const void* logits, int64_t M, int64_t V, int64_t ld, const int32_t* targets_dev,
                     float* logprobs_dev, int32_t* ids_dev, void* stream) {
    QIE_REQUIRE(logits && targets_dev && logprobs_dev && M >= 1 && V >= 1 && V < (1 << 24) && ld >= V,
                "qie_logprob_rows: bad arguments (M >= 1, 1 <= V < 2^24, ld >= V)");
    hipLaunchKernelGGL(logprob_rows_kernel, dim3((unsigned)M), dim3(kLpThreads), 0, (hipStream_t)stream,
                       (const uint16_t*)logits, V, ld, targets_dev, logprobs_dev, ids_dev);
    QIE_LAUNCH_CHECK();
    return 0;
}

int64_t qie_score_rows_workspace_bytes(int64_t M, int64_t V) {
    if (M < 1 || V < 1) return 0;
    return score_n_nt(V) * M * 16 + M * 4;
}

int qie_score_rows(const void* x, int64_t ldx, const void* W, int64_t M, int64_t K, int64_t V,
                   const int32_t* targets_dev, float* logprobs_dev, int32_t* ids_dev, void* ws, void* stream) {
    QIE_REQUIRE(x && W && targets_dev && logprobs_dev && ws, "qie_score_rows: null argument");
    QIE_REQUIRE(M >= 1 && V >= 1 && V < (1 << 24), "qie_score_rows: needs M >= 1 and 1 <= V < 2^24");
    QIE_REQUIRE(K >= 256 && K % g8::BK == 0, "qie_score_rows: needs K %% 64 == 0 and K >= 256 (K = %lld)", (long long)K);
    QIE_REQUIRE(ldx >= K && ldx % 8 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)W % 16 == 0 && (uintptr_t)ws % 8 == 0,
                "qie_score_rows: x and W must be 16-byte aligned with ldx %% 8 == 0, ldx >= K");
    const int64_t n_mt = (M + g8::BM - 1) / g8::BM, n_nt = score_n_nt(V);
    QIE_REQUIRE(n_mt * n_nt <= INT32_MAX, "qie_score_rows: %lld x %lld tiles", (long long)n_mt, (long long)n_nt);
    hipStream_t st = (hipStream_t)stream;
    const ScoreParams p{(const uint16_t*)x, ldx, (const uint16_t*)W, M, K, V, targets_dev, score_ws(ws, M, V)};
    constexpr size_t lds = 2 * g8::BUF;
    QIE_TRY(raise_dynamic_lds((const void*)score_tile_kernel, lds));
    hipLaunchKernelGGL(score_tile_kernel, dim3((unsigned)(n_mt * n_nt)), dim3(512), lds, st, p, (int)n_mt);
    QIE_LAUNCH_CHECK();
    hipLaunchKernelGGL(score_merge_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, p.ws, M, V, (int)n_nt,
                       targets_dev, logprobs_dev, ids_dev);
    QIE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
