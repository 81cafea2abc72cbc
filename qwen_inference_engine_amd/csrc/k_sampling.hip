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
    bool all;   // top_k == QIE_TOP_K_ALL and sampled: the whole-vocabulary kernels' row
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
    p.n_bias = e ? e->n_bias : -1;   // (no table: qie_sample's ALL mode)
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
    p.all = top_k == QIE_TOP_K_ALL && p.T > 0.f;
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

// Row m's window ids that fall in the slice [base, base + 4096), counted into cnt (zeroed by the
// caller; integer LDS atomics: order-independent) by a block of NT threads.
template <bool MAPPED, int NT>
__device__ __forceinline__ void count_window(const RowsArgs& a, int64_t m, int slot, const RowParams& p, int64_t base,
                                             int* cnt) {
    const int64_t q = a.q[m];
    const int32_t* tail = row_tail_of<MAPPED>(a, m);
    int64_t tl = tail && a.tail_len ? a.tail_len[m] : 0;
    tl = tl < 0 ? 0 : (tl > kMaxTail ? kMaxTail : tl);
    int64_t lo = p.last_n > 0 ? q + 1 - p.last_n : 0;
    lo = lo > p.start ? lo : p.start;
    lo = lo > 0 ? lo : 0;
    const int64_t hh = min(q - tl, a.hist_stride - 1);   // last position read from the history
    const int32_t* h = a.hist + (int64_t)slot * a.hist_stride;
    for (int64_t pos = lo + threadIdx.x; pos <= hh; pos += NT) {
        const int64_t d = (int64_t)h[pos] - base;
        if (d >= 0 && d < kSlice && base + d < a.V) atomicAdd(&cnt[d], 1);
    }
    // tail word t sits at position q - tl + 1 + t
    const int64_t t0 = lo - (q - tl + 1);
    for (int64_t t = (t0 > 0 ? t0 : 0) + threadIdx.x; t < tl; t += NT) {
        const int64_t d = (int64_t)tail[t] - base;
        if (d >= 0 && d < kSlice && base + d < a.V) atomicAdd(&cnt[d], 1);
    }
}

// Block (slice, row): counts the window's ids that fall in its 4096-id slice (integer LDS
// atomics: order-independent), builds the keys of the processed bf16 values, and leaves the
// slice's k best (sorted; greedy: its one maximum) in cand.  A row in ALL mode is not its work.
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
    if (p.all) return;
    const uint16_t* row = a.logits + m * a.ld;
    if (p.pen) {
        for (int i = threadIdx.x; i < kSlice; i += 256) cnt[i] = 0;
        __syncthreads();
        count_window<MAPPED, 256>(a, m, slot, p, base, cnt);
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
    if (p.all) return;
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

// ------------------------------------------------------------ the whole vocabulary (top_k == QIE_TOP_K_ALL)
// A row is bf16, so its candidates fall into at most 65,536 exact bins: no sort of V keys.  The
// 16-bit bin key is the top half of sel_key's value order (0: not selectable), a bin's members
// share one weight, and a bin's mass is count * weight.  Two launches (contract: qie_ops.h):
//   all_count_kernel  grid (2, M) x 1024: workgroup `half` owns keys [half * 32768, + 32768) as
//       u32 LDS counters (128 KiB).  Both stream the whole row (16-byte loads; a row with
//       penalties or bias goes slice by slice through count_window and leaves its processed
//       words in the workspace), so both know the row's maximum without waiting for each other;
//       then one thread per 256-key group sums count * weight in descending key order.
//   all_draw_kernel   grid M x 1024: scans the 256 group sums, re-scans the group of the top-p
//       cut and the group of the draw from the bin counts, then finds the drawn member of the
//       bin: a 256-bucket count over bitrev8(idx & 255), then index order inside the bucket.
// Integer atomics only; every float sum runs in one lane in a fixed order.
constexpr int kAllThreads = 1024;
constexpr int kHalfBins = 32768;
constexpr size_t kAllCountLds = kHalfBins * 4 + kSlice * 4 + kSlice * 2;

struct AllWs {   // per row: counts u32[65536], group mass f32[256], group count u32[256], top key u32[16], words u16[vpad]
    char* base;
    int64_t row_bytes;
    __host__ __device__ static int64_t bytes_per_row(int64_t V) { return 65536 * 4 + 256 * 4 + 256 * 4 + 64 + ((V + 7) / 8) * 16; }
    __device__ uint32_t* counts(int64_t m) const { return (uint32_t*)(base + m * row_bytes); }
    __device__ float* gmass(int64_t m) const { return (float*)(counts(m) + 65536); }
    __device__ uint32_t* gcnt(int64_t m) const { return counts(m) + 65536 + 256; }
    __device__ uint32_t* top(int64_t m) const { return counts(m) + 65536 + 512; }
    __device__ uint16_t* words(int64_t m) const { return (uint16_t*)(counts(m) + 65536 + 512 + 16); }
};

__device__ __forceinline__ uint32_t key16(uint32_t bits) {
    if (!(bf2f(bits) > -INFINITY)) return 0u;
    return (bits & 0x8000u) ? (~bits & 0xffffu) : (bits | 0x8000u);
}
__device__ __forceinline__ float key16_val(uint32_t k) { return bf2f((k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu)); }
// w(b) of the contract; mx = (the row's largest value) / T
__device__ __forceinline__ float bin_weight(uint32_t k, float T, float mx) {
#pragma clang fp contract(off)
    const float v = key16_val(k) / T;
    return expf(v - mx);
}
// does the bin of key k survive min_p?  (the top bin always)
__device__ __forceinline__ bool bin_kept(float w, uint32_t k, uint32_t ktop, float min_p) {
    return !(min_p > 0.f && min_p <= 1.f) || w >= min_p || k == ktop;
}
// counter k of a half sits at a rotated place inside its group of 256, so that one thread per
// group walking its group hits 64 different banks
__device__ __forceinline__ int bin_slot(int k) { return (k & ~255) | ((k + (k >> 8)) & 255); }

// f(bits, idx) for every word of row[0, V): 16-byte loads between the unaligned ends
template <class F>
__device__ __forceinline__ void for_each_word(const uint16_t* row, int64_t V, F&& f) {
    int64_t head = (int64_t)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 1);
    head = head < V ? head : V;
    for (int64_t i = threadIdx.x; i < head; i += kAllThreads) f((uint32_t)row[i], i);
    const int64_t nvec = (V - head) / 8;
    const uint4* rv = (const uint4*)(row + head);
    for (int64_t i = threadIdx.x; i < nvec; i += kAllThreads) {
        const uint4 q = rv[i];
        const int64_t i0 = head + i * 8;
        f(q.x & 0xffffu, i0), f(q.x >> 16, i0 + 1), f(q.y & 0xffffu, i0 + 2), f(q.y >> 16, i0 + 3);
        f(q.z & 0xffffu, i0 + 4), f(q.z >> 16, i0 + 5), f(q.w & 0xffffu, i0 + 6), f(q.w >> 16, i0 + 7);
    }
    for (int64_t i = head + nvec * 8 + threadIdx.x; i < V; i += kAllThreads) f((uint32_t)row[i], i);
}

template <bool MAPPED>
__global__ __launch_bounds__(kAllThreads) void all_count_kernel(RowsArgs a, AllWs w) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) uint32_t bins[];   // [kHalfBins], then cnt, vals
    int* cnt = (int*)(bins + kHalfBins);
    uint16_t* vals = (uint16_t*)(cnt + kSlice);
    __shared__ uint32_t red[kAllThreads / 64];
    const int64_t m = blockIdx.y;
    const uint32_t half = blockIdx.x;
    const int slot = a.table ? row_slot_of<MAPPED>(a, m) : 0;
    const qie_slot_sampling* e = a.table ? a.table + slot : nullptr;
    const RowParams p = row_params(e, a.fb, a.V);
    if (!p.all) return;
    for (int i = threadIdx.x; i < kHalfBins; i += kAllThreads) bins[i] = 0u;
    __syncthreads();
    const uint16_t* row = a.logits + m * a.ld;
    uint32_t ktop = 0u;
    auto add = [&](uint32_t bits, int64_t) {
        const uint32_t k = key16(bits);
        ktop = k > ktop ? k : ktop;
        if (k && (k >> 15) == half) atomicAdd(&bins[bin_slot((int)(k & 32767u))], 1u);
    };
    if (!p.pen && p.n_bias <= 0) {
        for_each_word(row, a.V, add);
    } else {   // the processed words l'[j], a 4096-id slice at a time (rows_slice_kernel's steps)
        uint16_t* out = w.words(m);
        for (int64_t base = 0; base < a.V; base += kSlice) {
            if (p.pen) {
                for (int i = threadIdx.x; i < kSlice; i += kAllThreads) cnt[i] = 0;
                __syncthreads();
                count_window<MAPPED, kAllThreads>(a, m, slot, p, base, cnt);
                __syncthreads();
            }
            for (int i = threadIdx.x; i < kSlice; i += kAllThreads) {
                const int64_t idx = base + i;
                if (idx >= a.V) break;
                uint16_t bits = row[idx];
                const int c = p.pen ? cnt[i] : 0;
                if (c > 0) bits = f2bf(penalise(bf2f(bits), c, p));
                vals[i] = bits;
            }
            if (p.n_bias > 0) {
                __syncthreads();
                if ((int)threadIdx.x < p.n_bias) {
                    const int64_t id = e->bias_ids[threadIdx.x];
                    const int64_t d = id - base;
                    if (d >= 0 && d < kSlice && id < a.V) {
                        float v = bf2f(row[id]);
                        const int c = p.pen ? cnt[d] : 0;
                        if (c > 0) v = penalise(v, c, p);
                        v = v + e->bias[threadIdx.x];
                        vals[d] = f2bf(v);
                    }
                }
            }
            __syncthreads();
            for (int i = threadIdx.x; i < kSlice; i += kAllThreads) {
                const int64_t idx = base + i;
                if (idx >= a.V) break;
                add(vals[i], idx);
                if (half == 0) out[idx] = vals[i];
            }
            __syncthreads();
        }
    }
    // the row's largest key: every thread has seen every word
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t t = __shfl_xor(ktop, o, 64);
        ktop = t > ktop ? t : ktop;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ktop;
    __syncthreads();   // (also: every count of this half is in)
    for (int i = 0; i < kAllThreads / 64; i++) ktop = red[i] > ktop ? red[i] : ktop;
    if (half == 0 && threadIdx.x == 0) w.top(m)[0] = ktop;
    if (ktop == 0u) return;
    if (threadIdx.x < kHalfBins / 256) {   // one group of 256 keys per thread, descending
        const int g = threadIdx.x;
        const float mx = key16_val(ktop) / p.T;
        float mass = 0.f;
        uint32_t n = 0u;
        for (int i = 255; i >= 0; i--) {
            const uint32_t c = bins[bin_slot(g * 256 + i)];
            if (c == 0u) continue;
            const uint32_t k = half * kHalfBins + g * 256 + i;
            const float wt = bin_weight(k, p.T, mx);
            if (!bin_kept(wt, k, ktop, p.min_p)) continue;
            mass += (float)c * wt;
            n += c;
        }
        w.gmass(m)[half * (kHalfBins / 256) + g] = mass;
        w.gcnt(m)[half * (kHalfBins / 256) + g] = n;
    }
    uint32_t* counts = w.counts(m) + half * kHalfBins;
    for (int i = threadIdx.x; i < kHalfBins; i += kAllThreads) counts[i] = bins[bin_slot(i)];
}

template <bool MAPPED>
__global__ __launch_bounds__(kAllThreads) void all_draw_kernel(RowsArgs a, AllWs w) {
#pragma clang fp contract(off)
    __shared__ float gm[256];
    __shared__ uint32_t gc[256], bc[256];
    __shared__ int bucket[256];
    __shared__ int wtot[kAllThreads / 64];
    __shared__ int s_g[2];        // the groups of the top-p cut and of the draw
    __shared__ float s_before[2];
    __shared__ float s_u;
    __shared__ uint32_t s_key;
    __shared__ int s_r, s_lane;
    const int64_t m = blockIdx.x;
    const int tid = threadIdx.x;
    const int slot = a.table ? row_slot_of<MAPPED>(a, m) : 0;
    const RowParams p = row_params(a.table ? a.table + slot : nullptr, a.fb, a.V);
    if (!p.all) return;
    const uint32_t ktop = w.top(m)[0];
    if (ktop == 0u) {
        if (tid == 0) a.ids[m] = -1;
        return;
    }
    const float mx = key16_val(ktop) / p.T;
    const uint32_t* counts = w.counts(m);
    if (tid < 256) gm[tid] = w.gmass(m)[tid], gc[tid] = w.gcnt(m)[tid];
    __syncthreads();
    const bool cut = p.top_p > 0.f && p.top_p < 1.f;
    float thr = 0.f;
    if (tid == 0) {   // the group in which the cumulative mass reaches top_p * total
        float total = 0.f;
        for (int g = 255; g >= 0; g--) total += gm[g];
        thr = p.top_p * total;
        float cum = 0.f;
        int g = 255;
        if (cut) {
            for (; g > 0; g--) {
                if (gc[g] && cum + gm[g] >= thr) break;
                cum += gm[g];
            }
        }
        s_g[0] = g, s_before[0] = cum;
        s_u = total;   // the kept total, when nothing is cut
    }
    // the prefix sums of group g's live bins: calls f(key, count, weight, prefix before, prefix with)
    // in descending key order until it returns true
    auto scan_group = [&](int g, auto&& f) {
        float pre = 0.f;
        for (int i = 255; i >= 0; i--) {
            const uint32_t c = bc[i];
            if (c == 0u) continue;
            const uint32_t k = (uint32_t)(g * 256 + i);
            const float wt = bin_weight(k, p.T, mx);
            if (!bin_kept(wt, k, ktop, p.min_p)) continue;
            const float with = pre + (float)c * wt;
            if (f(k, c, wt, pre, with)) return;
            pre = with;
        }
    };
    if (cut) {   // (uniform: an entry value)
        __syncthreads();
        if (tid < 256) bc[tid] = counts[s_g[0] * 256 + tid];
        __syncthreads();
        if (tid == 0) {
            const float before = s_before[0];
            float kept = before + gm[s_g[0]];
            scan_group(s_g[0], [&](uint32_t, uint32_t, float, float, float with) {
                if (before + with >= thr) { kept = before + with; return true; }
                return false;
            });
            s_u = kept;   // the cut bin stays whole
        }
    }
    if (tid == 0) {   // the draw, and its group
        const uint64_t sd = p.seed + (a.step ? (uint64_t)(int64_t)a.step[m] : 0ull);
        const float u = xorwow_uniform_first(sd) * s_u;
        float cum = 0.f;
        int g = 255;
        for (; g > 0; g--) {
            if (gc[g] && cum + gm[g] >= u) break;
            cum += gm[g];
        }
        // (rounding can leave u above every sum only if the masses are not finite: the lowest
        // live group then)
        while (g < 255 && !gc[g]) g++;
        s_g[1] = g, s_before[1] = cum, s_u = u;
    }
    __syncthreads();
    if (tid < 256) bc[tid] = counts[s_g[1] * 256 + tid], bucket[tid] = 0;
    __syncthreads();
    if (tid == 0) {   // the bin, and the member's rank inside it
        const float before = s_before[1], u = s_u;
        uint32_t key = 0u, cnt = 0u;
        float wt = 0.f, cb = 0.f;
        scan_group(s_g[1], [&](uint32_t k, uint32_t c, float w_, float pre, float with) {
            key = k, cnt = c, wt = w_, cb = pre == 0.f ? before : before + pre;   // (the last live bin stays if none reaches u)
            return before + with >= u;
        });
        uint32_t lo = 0u, hi = cnt ? cnt - 1u : 0u;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (u <= cb + (float)(mid + 1u) * wt) hi = mid;
            else lo = mid + 1u;
        }
        s_key = key, s_r = (int)lo;
    }
    __syncthreads();
    const uint32_t key = s_key;
    const uint16_t* src = (p.pen || p.n_bias > 0) ? w.words(m) : a.logits + m * a.ld;
    for_each_word(src, a.V, [&](uint32_t bits, int64_t idx) {
        if (key16(bits) == key) atomicAdd(&bucket[__builtin_bitreverse32((uint32_t)idx & 0xffu) >> 24], 1);
    });
    __syncthreads();
    if (tid == 0) {   // descending sel_key inside a bin: bitrev8(idx & 255) down, then idx up
        int r = s_r, br = 255;
        for (; br > 0; br--) {
            if (r < bucket[br]) break;
            r -= bucket[br];
        }
        s_r = r, s_lane = (int)(__builtin_bitreverse32((uint32_t)br) >> 24);
        a.ids[m] = -1;   // (overwritten below: the bin's count says that the member exists)
    }
    __syncthreads();
    const int r = s_r, x = s_lane;
    const int64_t J = a.V > x ? (a.V - x + 255) / 256 : 0;
    int seen = 0;
    for (int64_t j0 = 0; j0 < J && seen <= r; j0 += kAllThreads) {   // (uniform bounds)
        const int64_t j = j0 + tid;
        const bool hit = j < J && key16(src[x + 256 * j]) == key;
        const unsigned long long bal = __ballot(hit);
        if ((tid & 63) == 0) wtot[tid >> 6] = __popcll(bal);
        __syncthreads();
        int mine = seen + __popcll(bal & ((1ull << (tid & 63)) - 1ull)), all = 0;
        for (int i = 0; i < kAllThreads / 64; i++) {
            if (i < (tid >> 6)) mine += wtot[i];
            all += wtot[i];
        }
        if (hit && mine == r) a.ids[m] = (int32_t)(x + 256 * j);
        seen += all;
        __syncthreads();
    }
}

static int pow2_at_least(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// The ALL-mode part of a sampler workspace lies behind the top-k part (`head` bytes of it).
static int64_t all_ws_offset(int64_t head) { return (head + 255) / 256 * 256; }
static int64_t sample_ws_head(int64_t M, int64_t V) { return M * ((V + kSlice - 1) / kSlice) * kMaxTopK * 8 + M * 8 + 64; }
static int64_t rows_ws_head(int64_t M, int64_t V) { return M * ((V + kSlice - 1) / kSlice) * kMaxTopK * 8 + 64; }

// The two whole-vocabulary launches over the M rows of r; rows not in ALL mode leave at once.
template <bool MAPPED>
static int launch_all(const RowsArgs& r, int64_t M, void* ws, int64_t head, hipStream_t st) {
    const AllWs w{(char*)ws + all_ws_offset(head), AllWs::bytes_per_row(r.V)};
    QIE_TRY(raise_dynamic_lds((const void*)all_count_kernel<MAPPED>, kAllCountLds));
    hipLaunchKernelGGL(all_count_kernel<MAPPED>, dim3(2, (unsigned)M), dim3(kAllThreads), kAllCountLds, st, r, w);
    QIE_LAUNCH_CHECK();
    hipLaunchKernelGGL(all_draw_kernel<MAPPED>, dim3((unsigned)M), dim3(kAllThreads), 0, st, r, w);
    QIE_LAUNCH_CHECK();
    return 0;
}

}  // namespace qie

using namespace qie;

extern "C" {

int64_t qie_sample_workspace_bytes(int64_t M, int64_t V) {
    return all_ws_offset(sample_ws_head(M, V)) + M * AllWs::bytes_per_row(V);
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
    if (s->top_k == QIE_TOP_K_ALL && s->temperature > 0.f) {   // every row, under the call's values
        RowsArgs r{};
        r.logits = (const uint16_t*)logits, r.V = V, r.ld = ld;
        r.fb = *s, r.step = step_dev, r.ids = out_ids;
        return launch_all<false>(r, M, ws, sample_ws_head(M, V), st);
    }
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
    return all_ws_offset(rows_ws_head(M, V)) + M * AllWs::bytes_per_row(V);
}

}  // extern "C"

// qie_sample_rows and its mapped form: the same two launches, MAPPED reading row_slot / tail_off;
// all_mode: a row may be in ALL mode (entries are device data), so the two whole-vocabulary
// launches follow
template <bool MAPPED>
static int sample_rows(const qie_sample_rows_args* a, const int32_t* row_slot, const int32_t* tail_off, bool all_mode,
                       void* stream, const char* who) {
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
    if (all_mode) QIE_TRY(launch_all<MAPPED>(r, a->M, a->ws, rows_ws_head(a->M, V), st));
    return 0;
}

int qie::sample_rows_launch(const qie_sample_rows_args* a, const int32_t* row_slot_dev, const int32_t* tail_off_dev,
                            bool all_mode, void* stream) {
    if (row_slot_dev) return sample_rows<true>(a, row_slot_dev, tail_off_dev, all_mode, stream, "qie_sample_rows_mapped");
    return sample_rows<false>(a, nullptr, nullptr, all_mode, stream, "qie_sample_rows");
}

extern "C" {

int qie_sample_rows(const qie_sample_rows_args* a, void* stream) {
    return sample_rows<false>(a, nullptr, nullptr, true, stream, "qie_sample_rows");
}

int qie_sample_rows_mapped(const qie_sample_rows_args* a, const int32_t* row_slot_dev, const int32_t* tail_off_dev,
                           void* stream) {
    QIE_REQUIRE(row_slot_dev && (tail_off_dev || !(a && a->tail_dev)), "qie_sample_rows_mapped: bad arguments");
    return sample_rows<true>(a, row_slot_dev, tail_off_dev, true, stream, "qie_sample_rows_mapped");
}

}  // extern "C"
