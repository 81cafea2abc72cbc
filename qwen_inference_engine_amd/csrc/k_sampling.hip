// k_sampling.hip — greedy arg-max and top-k / temperature / top-p sampling.
//
// Replaces topk_temperature_softmax_sampling_kernel_bf16 + blockArgMax/better
// (layers/src/logit_decode.cu:15-33, 149-274) and sample_topk_bf16
// (helpers.cuh:157-166).  The reference runs ONE 256-thread block that makes k
// full sweeps over V with an O(k) membership scan per element.  Here:
//   * every logit maps to a 64-bit selection key whose order IS the reference's
//     selection order (value, then bitrev8(idx mod 256), then -idx; see
//     qie_common.hpp sel_key) — greedy is a parallel max over keys (also fused
//     into the lm_head GEMV epilogue, k_gemv.hip);
//   * top-k = per-4096-slice bitonic sort (LDS) + a merge sort of the slice
//     winners; the sorted keys reproduce the reference's k rounds exactly;
//   * softmax + draw on one lane with the reference's sequential order and a
//     cuRAND-XORWOW restatement (curand_init(seed, 0, 0); curand_uniform).
//   * qie_sample_rows: the same two launches with every row under its own entry of a device
//     table (penalties over a window of the slot's token history, logit bias, min-p;
//     DESIGN.md §19) — the reference has one host-side parameter set per call.
#include "qie_common.hpp"
#include "launch_util.hpp"
#include "../../include/qie/qie_ops.h"

namespace qie {

constexpr int kSlice = 4096;
constexpr int kMaxTopK = 256;
constexpr int kMaxTail = 256;   // qie_sample_rows: ids a row may carry beside its history

__global__ __launch_bounds__(256) void argmax_keys_kernel(const uint16_t* __restrict__ logits,
                                                          int64_t V, int64_t ld,
                                                          unsigned long long* keys) {
    __shared__ unsigned long long red[4];
    const int64_t m = blockIdx.y;
    const uint16_t* row = logits + m * ld;
    unsigned long long best = 0ull;
    const int64_t per = (V + gridDim.x - 1) / gridDim.x;
    const int64_t lo = blockIdx.x * per, hi = min(V, lo + per);
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        unsigned long long k = sel_key(bf2f(row[i]), (uint32_t)i);
        best = k > best ? k : best;
    }
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = red[0];
        for (int w = 1; w < 4; w++) b = red[w] > b ? red[w] : b;
        if (b) atomicMax(keys + m, b);
    }
}

__global__ void keys_to_ids_kernel(const unsigned long long* keys, int64_t M, int32_t* ids) {
    const int64_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < M) ids[m] = key_idx(keys[m]);
}

// Bitonic sort, descending, of n (power of two) keys in LDS.
__device__ void bitonic_desc(unsigned long long* k, int n) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int j = threadIdx.x; j < n / 2; j += blockDim.x) {
                const int i = (j / stride) * 2 * stride + (j % stride);
                const int q = i + stride;
                const bool desc = (i & size) == 0;
                unsigned long long a = k[i], b = k[q];
                if (desc ? (a < b) : (a > b)) {
                    k[i] = b;
                    k[q] = a;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void topk_slice_kernel(const uint16_t* __restrict__ logits, int64_t V,
                                                         int64_t ld, int k,
                                                         unsigned long long* __restrict__ cand) {
    __shared__ unsigned long long keys[kSlice];
    const int64_t m = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * kSlice;
    const uint16_t* row = logits + m * ld;
    for (int i = threadIdx.x; i < kSlice; i += 256) {
        const int64_t idx = base + i;
        keys[i] = idx < V ? sel_key(bf2f(row[idx]), (uint32_t)idx) : 0ull;
    }
    __syncthreads();
    bitonic_desc(keys, kSlice);
    unsigned long long* out = cand + (m * gridDim.x + blockIdx.x) * (int64_t)k;
    for (int i = threadIdx.x; i < k; i += 256) out[i] = keys[i];
}

// cuRAND XORWOW, curand_init(seed, subsequence = 0, offset = 0) (no skip-ahead)
// and curand_uniform — restated from the published curand_kernel.h.
__device__ __forceinline__ float xorwow_uniform_first(uint64_t seed) {
    uint32_t s0 = (uint32_t)seed ^ 0xaad26b49u;
    uint32_t s1 = (uint32_t)(seed >> 32) ^ 0xf7dcefddu;
    uint32_t t0 = 1099087573u * s0;
    uint32_t t1 = 2591861531u * s1;
    uint32_t d = 6615241u + t1 + t0;
    uint32_t v0 = 123456789u + t0, v4 = 5783321u + t0;
    uint32_t t = v0 ^ (v0 >> 2);
    uint32_t nv4 = (v4 ^ (v4 << 4)) ^ (t ^ (t << 1));
    d += 362437u;
    uint32_t x = nv4 + d;
    return x * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
}

// Softmax at temperature T over the k largest keys sk[0..k) (sorted descending), the optional
// min-p and top-p cuts, one draw from seed sd: logit_decode.cu:225-272 (thread 0).  One lane.
__device__ __forceinline__ int32_t draw_sorted(const unsigned long long* sk, int k, float temperature, float top_p,
                                               float min_p, uint64_t sd) {
#pragma clang fp contract(off)
    int n = 0;
    while (n < k && sk[n] != 0ull) n++;
    if (n == 0) return -1;
    float vals[kMaxTopK];
    float T = temperature > 0.0f ? temperature : 1.0f;
    float max_val = key_val(sk[0]) / T;
    for (int i = 1; i < n; i++) {
        float v = key_val(sk[i]) / T;
        if (v > max_val) max_val = v;
        vals[i] = v;
    }
    vals[0] = key_val(sk[0]) / T;
    float sum = 0.0f;
    for (int i = 0; i < n; i++) {
        vals[i] = expf(vals[i] - max_val);
        sum += vals[i];
    }
    if (min_p > 0.0f && min_p <= 1.0f) {   // the leading entries at least min_p of the best (entry 0 stays)
        int keep = 1;
        while (keep < n && vals[keep] >= min_p) keep++;
        if (keep < n) {
            n = keep;
            sum = 0.0f;
            for (int i = 0; i < n; i++) sum += vals[i];
        }
    }
    if (top_p > 0.0f && top_p < 1.0f) {
        float cum = 0.0f;
        int keep = n;
        for (int i = 0; i < n; i++) {
            cum += vals[i];
            if (cum >= top_p * sum) { keep = i + 1; break; }
        }
        n = keep;
        sum = 0.0f;
        for (int i = 0; i < n; i++) sum += vals[i];
    }
    float u = xorwow_uniform_first(sd) * sum;
    float cum = 0.0f;
    int picked = key_idx(sk[n - 1]);
    for (int i = 0; i < n; i++) {
        cum += vals[i];
        if (u <= cum) { picked = key_idx(sk[i]); break; }
    }
    return picked;
}

__global__ __launch_bounds__(256) void topk_merge_sample_kernel(const unsigned long long* __restrict__ cand,
                                                                int nb, int k, int n2, float temperature,
                                                                float top_p, uint64_t seed,
                                                                const int32_t* step, int32_t* ids) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];
    const int64_t m = blockIdx.x;
    const int total = nb * k;
    for (int i = threadIdx.x; i < n2; i += 256) sk[i] = i < total ? cand[m * total + i] : 0ull;
    __syncthreads();
    bitonic_desc(sk, n2);
    if (threadIdx.x != 0) return;
    const uint64_t sd = seed + (step ? (uint64_t)(int64_t)step[m] : 0ull);
    ids[m] = draw_sorted(sk, k, temperature, top_p, 0.0f, sd);
}

// ------------------------------------------------------------ per-row entries (qie_sample_rows)
// What a row runs under: its slot's table entry, or (n_bias < 0: none) a neutral entry with the
// call's four values.  Uniform per block.
struct RowParams {
    int k;   // candidates per slice and in the draw: 1 = greedy
    float T, top_p, min_p;
    uint64_t seed;
    float rep, pres, freq;
    int start, last_n, n_bias;
    bool pen;
};
struct RowsArgs {
    const uint16_t* logits;
    int64_t V, ld;
    const qie_slot_sampling* table;
    int slot0, slot_stride;
    qie_sampling fb;
    const int32_t* hist;
    int64_t hist_stride;
    const int32_t *q, *tail, *tail_len, *step;
    int32_t* ids;
    unsigned long long* cand;   // [M][nb][kMaxTopK] (a row's slices packed at its own k)
    int nb;
    // qie_sample_rows_mapped (the MAPPED kernels only): row m's slot and where its tail begins
    const int32_t *row_slot, *tail_off;
};
// Row m's slot, and its tail's first word.  MAPPED is a template parameter of the two kernels, so
// the strided form's code is what it was before the mapped form existed.
template <bool MAPPED>
__device__ __forceinline__ int row_slot_of(const RowsArgs& a, int64_t m) {
    if (MAPPED) return a.row_slot[m];
    return a.slot0 + (int)m * a.slot_stride;
}
template <bool MAPPED>
__device__ __forceinline__ const int32_t* row_tail_of(const RowsArgs& a, int64_t m) {
    if (MAPPED) return a.tail ? a.tail + a.tail_off[m] : nullptr;
    return a.tail;
}

__device__ __forceinline__ RowParams row_params(const qie_slot_sampling* e, const qie_sampling& fb, int64_t V) {
    RowParams p;
    p.n_bias = e->n_bias;
    int top_k;
    if (p.n_bias < 0) {
        top_k = fb.top_k, p.T = fb.temperature, p.top_p = fb.top_p, p.min_p = 0.f, p.seed = fb.seed;
        p.rep = 1.f, p.pres = 0.f, p.freq = 0.f, p.start = 0, p.last_n = 0, p.n_bias = 0;
    } else {
        top_k = e->top_k, p.T = e->temperature, p.top_p = e->top_p, p.min_p = e->min_p, p.seed = e->seed;
        p.rep = e->repetition_penalty, p.pres = e->presence_penalty, p.freq = e->frequency_penalty;
        p.start = e->penalty_start, p.last_n = e->penalty_last_n;
        if (p.n_bias > QIE_SLOT_BIAS_MAX) p.n_bias = QIE_SLOT_BIAS_MAX;
    }
    const bool greedy = top_k <= 1 || !(p.T > 0.f);
    p.k = greedy ? 1 : (int)min((int64_t)min(top_k, kMaxTopK), V);
    p.pen = p.rep != 1.f || p.pres != 0.f || p.freq != 0.f;
    return p;
}

// the contract's penalty step on an id seen c > 0 times (qie_ops.h)
__device__ __forceinline__ float penalise(float v, int c, const RowParams& p) {
#pragma clang fp contract(off)
    if (p.rep != 1.f) v = v > 0.f ? v / p.rep : v * p.rep;
    float t = p.freq * (float)c;
    t = p.pres + t;
    return v - t;
}

__device__ __forceinline__ unsigned long long block_max_key(unsigned long long best, unsigned long long* red) {
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    unsigned long long b = red[0];
    for (int w = 1; w < 4; w++) b = red[w] > b ? red[w] : b;
    return b;
}

// Block (slice, row): counts the window's ids that fall in its 4096-id slice (integer LDS
// atomics: order-independent), builds the keys of the processed bf16 values, and leaves the
// slice's k best (sorted; greedy: its one maximum) in cand.
template <bool MAPPED>
__global__ __launch_bounds__(256) void rows_slice_kernel(RowsArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned long long keys[kSlice];
    __shared__ int cnt[kSlice];
    __shared__ unsigned long long red[4];
    const int64_t m = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * kSlice;
    const int slot = row_slot_of<MAPPED>(a, m);
    const qie_slot_sampling* e = a.table + slot;
    const RowParams p = row_params(e, a.fb, a.V);
    const uint16_t* row = a.logits + m * a.ld;
    if (p.pen) {
        for (int i = threadIdx.x; i < kSlice; i += 256) cnt[i] = 0;
        __syncthreads();
        const int64_t q = a.q[m];
        const int32_t* tail = row_tail_of<MAPPED>(a, m);
        int64_t tl = tail && a.tail_len ? a.tail_len[m] : 0;
        tl = tl < 0 ? 0 : (tl > kMaxTail ? kMaxTail : tl);
        int64_t lo = p.last_n > 0 ? q + 1 - p.last_n : 0;
        lo = lo > p.start ? lo : p.start;
        lo = lo > 0 ? lo : 0;
        const int64_t hh = min(q - tl, a.hist_stride - 1);   // last position read from the history
        const int32_t* h = a.hist + (int64_t)slot * a.hist_stride;
        for (int64_t pos = lo + threadIdx.x; pos <= hh; pos += 256) {
            const int64_t d = (int64_t)h[pos] - base;
            if (d >= 0 && d < kSlice && base + d < a.V) atomicAdd(&cnt[d], 1);
        }
        // tail word t sits at position q - tl + 1 + t
        const int64_t t0 = lo - (q - tl + 1);
        for (int64_t t = (t0 > 0 ? t0 : 0) + threadIdx.x; t < tl; t += 256) {
            const int64_t d = (int64_t)tail[t] - base;
            if (d >= 0 && d < kSlice && base + d < a.V) atomicAdd(&cnt[d], 1);
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < kSlice; i += 256) {
        const int64_t idx = base + i;
        unsigned long long key = 0ull;
        if (idx < a.V) {
            uint16_t bits = row[idx];
            const int c = p.pen ? cnt[i] : 0;
            if (c > 0) bits = f2bf(penalise(bf2f(bits), c, p));
            key = sel_key(bf2f(bits), (uint32_t)idx);
        }
        keys[i] = key;
    }
    if (p.n_bias > 0) {   // at most 32 ids: each redone from the logit, after the sweep
        __syncthreads();
        if ((int)threadIdx.x < p.n_bias) {
            const int64_t id = e->bias_ids[threadIdx.x];
            const int64_t d = id - base;
            if (d >= 0 && d < kSlice && id < a.V) {
                float v = bf2f(row[id]);
                const int c = p.pen ? cnt[d] : 0;
                if (c > 0) v = penalise(v, c, p);
                v = v + e->bias[threadIdx.x];
                keys[d] = sel_key(bf2f(f2bf(v)), (uint32_t)id);
            }
        }
    }
    __syncthreads();
    unsigned long long* out = a.cand + (m * a.nb * kMaxTopK) + (int64_t)blockIdx.x * p.k;
    if (p.k == 1) {   // a max-reduce, not the sort (the branch is uniform per block)
        unsigned long long best = 0ull;
        for (int i = threadIdx.x; i < kSlice; i += 256) best = keys[i] > best ? keys[i] : best;
        best = block_max_key(best, red);
        if (threadIdx.x == 0) out[0] = best;
        return;
    }
    bitonic_desc(keys, kSlice);
    for (int i = threadIdx.x; i < p.k; i += 256) out[i] = keys[i];
}

// Block m: merges row m's nb * k slice winners and draws under the row's own parameters.
// Dynamic LDS is sized for k = kMaxTopK; the sort runs over the row's own count.
template <bool MAPPED>
__global__ __launch_bounds__(256) void rows_merge_sample_kernel(RowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];   // all of the kernel's LDS (up to 160 KiB)
    const int64_t m = blockIdx.x;
    const int slot = row_slot_of<MAPPED>(a, m);
    const RowParams p = row_params(a.table + slot, a.fb, a.V);
    const unsigned long long* cand = a.cand + m * a.nb * kMaxTopK;
    const int total = a.nb * p.k;
    if (p.k == 1) {
        unsigned long long best = 0ull;
        for (int i = threadIdx.x; i < total; i += 256) best = cand[i] > best ? cand[i] : best;
        best = block_max_key(best, sk);   // (the sort's LDS is free on this path; at least 4 words)
        if (threadIdx.x == 0) a.ids[m] = key_idx(best);
        return;
    }
    int n2 = 1;
    while (n2 < total) n2 <<= 1;
    for (int i = threadIdx.x; i < n2; i += 256) sk[i] = i < total ? cand[i] : 0ull;
    __syncthreads();
    bitonic_desc(sk, n2);
    if (threadIdx.x != 0) return;
    const uint64_t sd = p.seed + (a.step ? (uint64_t)(int64_t)a.step[m] : 0ull);
    a.ids[m] = draw_sorted(sk, p.k, p.T, p.top_p, p.min_p, sd);
}

static int pow2_at_least(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace qie

using namespace qie;

extern "C" {

int64_t qie_sample_workspace_bytes(int64_t M, int64_t V) {
    const int64_t nb = (V + kSlice - 1) / kSlice;
    return M * nb * kMaxTopK * 8 + M * 8 + 64;
}

int qie_keys_to_ids(const uint64_t* keys, int64_t M, int32_t* out_ids, void* stream) {
    QIE_REQUIRE(keys && out_ids && M >= 0, "qie_keys_to_ids: bad arguments");
    if (M == 0) return 0;
    hipLaunchKernelGGL(keys_to_ids_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0,
                       (hipStream_t)stream, (const unsigned long long*)keys, M, out_ids);
    QIE_LAUNCH_CHECK();
    return 0;
}

int qie_sample(const void* logits, int64_t M, int64_t V, int64_t ld, const qie_sampling* s,
               const int32_t* step_dev, int32_t* out_ids, void* ws, void* stream) {
    QIE_REQUIRE(logits && s && out_ids && ws && M >= 0 && V > 0 && V < (1 << 24) && ld >= V,
                "qie_sample: bad arguments");
    if (M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (s->top_k <= 1) {
        unsigned long long* keys = (unsigned long long*)ws;
        QIE_HIP(hipMemsetAsync(keys, 0, M * 8, st));
        hipLaunchKernelGGL(argmax_keys_kernel, dim3(64, (unsigned)M), dim3(256), 0, st,
                           (const uint16_t*)logits, V, ld, keys);
        QIE_LAUNCH_CHECK();
        return qie_keys_to_ids((const uint64_t*)keys, M, out_ids, stream);
    }
    int k = s->top_k;
    if (k > V) k = (int)V;
    if (k > kMaxTopK) k = kMaxTopK;
    const int nb = (int)((V + kSlice - 1) / kSlice);
    unsigned long long* cand = (unsigned long long*)ws;
    hipLaunchKernelGGL(topk_slice_kernel, dim3(nb, (unsigned)M), dim3(256), 0, st,
                       (const uint16_t*)logits, V, ld, k, cand);
    QIE_LAUNCH_CHECK();
    const int n2 = pow2_at_least(nb * k);
    const size_t shm = (size_t)n2 * 8;
    QIE_REQUIRE(shm <= 160 * 1024, "qie_sample: top-k merge exceeds LDS (V=%lld k=%d)", (long long)V, k);
    if (shm > 65536) QIE_TRY(raise_dynamic_lds((const void*)topk_merge_sample_kernel, 160 * 1024));
    hipLaunchKernelGGL(topk_merge_sample_kernel, dim3((unsigned)M), dim3(256), shm, st, cand, nb, k, n2,
                       s->temperature, s->top_p, (uint64_t)s->seed, step_dev, out_ids);
    QIE_LAUNCH_CHECK();
    return 0;
}

int64_t qie_sample_rows_workspace_bytes(int64_t M, int64_t V) {
    const int64_t nb = (V + kSlice - 1) / kSlice;
    return M * nb * kMaxTopK * 8 + 64;
}

}  // extern "C"

// qie_sample_rows and its mapped form: the same two launches, MAPPED reading row_slot / tail_off
template <bool MAPPED>
static int sample_rows(const qie_sample_rows_args* a, const int32_t* row_slot, const int32_t* tail_off, void* stream,
                       const char* who) {
    QIE_REQUIRE(a && a->logits && a->table && a->hist && a->q_dev && a->out_ids && a->ws && a->M >= 0 && a->V > 0 &&
                    a->ld >= a->V && a->hist_stride > 0 && a->slot0 >= 0 && a->slot_stride >= 0,
                "%s: bad arguments", who);
    const int64_t V = a->V;
    const int nb = (int)((V + kSlice - 1) / kSlice);
    // the merge sorts up to nb * 256 keys in LDS
    QIE_REQUIRE(nb <= 64, "%s: V %lld exceeds %d ids", who, (long long)V, 64 * kSlice);
    if (a->M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    RowsArgs r{};
    r.logits = (const uint16_t*)a->logits, r.V = V, r.ld = a->ld;
    r.table = a->table, r.slot0 = a->slot0, r.slot_stride = a->slot_stride;
    r.fb = a->fallback ? *a->fallback : qie_sampling{1, 0.f, 1.f, 0};
    r.hist = a->hist, r.hist_stride = a->hist_stride;
    r.q = a->q_dev, r.tail = a->tail_dev, r.tail_len = a->tail_len_dev, r.step = a->step_dev;
    r.ids = a->out_ids, r.cand = (unsigned long long*)a->ws, r.nb = nb;
    r.row_slot = row_slot, r.tail_off = tail_off;
    hipLaunchKernelGGL(rows_slice_kernel<MAPPED>, dim3(nb, (unsigned)a->M), dim3(256), 0, st, r);
    QIE_LAUNCH_CHECK();
    const size_t shm = (size_t)std::max(4, pow2_at_least(nb * (int)std::min<int64_t>(kMaxTopK, V))) * 8;
    if (shm > 65536) QIE_TRY(raise_dynamic_lds((const void*)rows_merge_sample_kernel<MAPPED>, 160 * 1024));
    hipLaunchKernelGGL(rows_merge_sample_kernel<MAPPED>, dim3((unsigned)a->M), dim3(256), shm, st, r);
    QIE_LAUNCH_CHECK();
    return 0;
}

extern "C" {

int qie_sample_rows(const qie_sample_rows_args* a, void* stream) {
    return sample_rows<false>(a, nullptr, nullptr, stream, "qie_sample_rows");
}

int qie_sample_rows_mapped(const qie_sample_rows_args* a, const int32_t* row_slot_dev, const int32_t* tail_off_dev,
                           void* stream) {
    QIE_REQUIRE(row_slot_dev && (tail_off_dev || !(a && a->tail_dev)), "qie_sample_rows_mapped: bad arguments");
    return sample_rows<true>(a, row_slot_dev, tail_off_dev, stream, "qie_sample_rows_mapped");
}

}  // extern "C"
