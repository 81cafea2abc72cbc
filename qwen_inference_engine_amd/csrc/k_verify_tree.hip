// k_verify_tree.hip — the kernels that frame a tree verify step (verify.hpp) and
// the two operators only that step needs: the q/k post-projection with the RoPE position apart
// from the cache row (qie_qkv_post_tree) and the compaction of the accepted path's K/V rows
// (qie_kv_compact).  The step's attention is attn_extend_block's TREE form (k_attn_extend.hip).
// Plain HIP, vector stores only; the tree's shape, every position and every id come from device
// memory, so one captured hipGraph serves every tree of M rows.
#include "verify.hpp"
#include "qkv_post.hpp"

namespace qie {

// node j's parent, whatever the words hold a value in [0, j) (the host refused a malformed tree)
__device__ __forceinline__ int tree_parent(const int32_t* vt, int j) {
    const int q = vt[kVtParent + j - 1];
    return q < 0 ? 0 : (q >= j ? j - 1 : q);
}
__device__ __forceinline__ int32_t tree_draft(const int32_t* vt, int j, int32_t vocab) {
    const int32_t t = vt[kVtDraft + j - 1];
    return t < 0 || t >= vocab ? 0 : t;   // (the host refused such a draft; never read out of bounds)
}

// Block i builds row i as verify_rows_kernel does (node 0: the pending token's embedding in
// x_res[seq]; node i >= 1: the embedding of its drafted id), and thread 0 walks the node's root
// path for what the other kernels read: the RoPE position and sampling counter p + depth and
// step + depth, the cache row p + i, the ancestor-or-self mask, and the ids of the path below the
// root in depth order (the sampler's tail: the window is the slot's history, then these).
__global__ __launch_bounds__(256) void verify_tree_rows_kernel(VerifyTreeRowsArgs a) {
    const int i = blockIdx.x;
    const uint4* src = a.x_res + (int64_t)a.seq * a.H8;
    if (i > 0) src = a.E + (int64_t)tree_draft(a.vt, i, a.vocab) * a.H8;
    uint4* dst = a.vx + (int64_t)i * a.H8;
    for (int64_t j = threadIdx.x; j < a.H8; j += 256) dst[j] = src[j];
    if (threadIdx.x == 0) {
        int depth = 0;
        uint32_t anc = 1u << i;
        for (int j = i; j > 0; depth++) {
            j = tree_parent(a.vt, j);
            anc |= 1u << j;
        }
        int d = depth;
        for (int j = i; j > 0; j = tree_parent(a.vt, j)) a.vt[kVtIds + 16 * i + --d] = tree_draft(a.vt, j, a.vocab);
        const int32_t p = a.pos[a.seq];
        a.vpos[i] = p + depth;
        a.vstep[i] = a.step[a.seq] + depth;
        a.vt[kVtRow + i] = p + i;
        a.vt[kVtAnc + i] = (int32_t)anc;
        a.vt[kVtDepth + i] = depth;
        a.vt[kVtTailOff + i] = 16 * i;
        a.vt[kVtSlot + i] = a.seq;
    }
}

// One block.  Row i chose token t_i as in verify_commit_kernel.  The accepted path starts at the
// root and follows, while there is one, the lowest child whose drafted id is the token its parent
// chose; its nodes by depth are path[0 .. a], the emitted tokens t_path[0] .. t_path[a].  The
// sequence is left as after a + 1 decode steps (verify_commit_kernel's words, from the path's
// rows), and the path stays in the step's words for qie_kv_compact.
__global__ __launch_bounds__(1024) void verify_tree_commit_kernel(VerifyTreeCommitArgs a) {
    __shared__ int32_t s_tok[kVerifyMaxRows];
    __shared__ int s_last, s_lastrow;
    const int tid = threadIdx.x;
    const int32_t p = a.pos[a.seq];
    if (tid < a.M) {
        int32_t tok = a.keys ? key_idx(a.keys[tid]) : a.ids[tid];
        if (tok < 0 || tok >= a.vocab) tok = 0;
        s_tok[tid] = tok;
    }
    __syncthreads();
    if (tid == 0) {
        int32_t* hist = a.hist + (int64_t)a.seq * a.hist_stride;
        int cur = 0, acc = 0;
        for (;;) {
            a.vt[kVtPath + acc] = cur;
            a.vt[kVtRes + 1 + acc] = s_tok[cur];
            if (p + 1 + acc < a.hist_stride) hist[p + 1 + acc] = s_tok[cur];
            int next = 0;
            for (int j = a.M - 1; j > cur; j--)
                if (tree_parent(a.vt, j) == cur && a.vt[kVtDraft + j - 1] == s_tok[cur]) next = j;
            if (!next) break;
            cur = next;
            acc++;
        }
        for (int d = acc + 1; d < kVerifyMaxRows; d++) a.vt[kVtPath + d] = 0, a.vt[kVtRes + 1 + d] = 0;
        a.vt[kVtAcc] = acc;
        a.vt[kVtRes] = acc + 1;
        a.pos[a.seq] = p + acc + 1;
        a.step[a.seq] = a.step[a.seq] + acc + 1;
        a.ids_out[a.seq] = s_tok[cur];
        s_last = acc;
        s_lastrow = cur;
    }
    if (tid < a.M && a.keys) a.keys[tid] = 0ull;
    __syncthreads();
    const int acc = s_last, cur = s_lastrow;
    write_rope_cur(a.rca, a.seq, p + acc + 1);
    const uint4* src = a.E + (int64_t)s_tok[cur] * a.H8;
    uint4* dst = a.x_res + (int64_t)a.seq * a.H8;
    for (int64_t j = tid; j < a.H8; j += blockDim.x) dst[j] = src[j];
    copy_row_bf16(a.vlogits + (int64_t)cur * a.Vl, a.logits + (int64_t)a.seq * a.Vl, a.Vl);
}

int launch_verify_tree_rows(const VerifyTreeRowsArgs& a, hipStream_t st) {
    QIE_REQUIRE(a.M >= 1 && a.M <= kVerifyMaxRows, "verify_tree_rows: %d rows", a.M);
    hipLaunchKernelGGL(verify_tree_rows_kernel, dim3(a.M), dim3(256), 0, st, a);
    QIE_LAUNCH_CHECK();
    return 0;
}

int launch_verify_tree_commit(const VerifyTreeCommitArgs& a, hipStream_t st) {
    QIE_REQUIRE(a.M >= 1 && a.M <= kVerifyMaxRows, "verify_tree_commit: %d rows", a.M);
    hipLaunchKernelGGL(verify_tree_commit_kernel, dim3(1), dim3(1024), 0, st, a);
    QIE_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------- q/k post-projection of a tree's rows
// qkv_post_kernel (k_misc.hip) for the rows of ONE sequence, with row m rotated at rpos[m] and its
// K/V written at cache row crow[m]: the loads, qkv_post_pair and the stores are that kernel's, so a
// row gives the q, K and V bits it gives there at the same position.
struct QkvPostTreeArgs : QkvPostArgs {
    const int32_t* crow;
    int seq;
};

template <bool PG, bool HF>
__global__ __launch_bounds__(256) void qkv_post_tree_kernel(QkvPostTreeArgs a) {
#pragma clang fp contract(off)
    const int64_t m = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hd = a.hd, half = hd / 2;
    const int QD = a.nq * hd, KD = a.nkv * hd;
    const int ptot = a.nq + 2 * a.nkv;
    const int p = a.pos[m], cr = a.crow[m];
    const uint16_t* row = a.qkv + m * (int64_t)(QD + 2 * KD);
    const bool active = lane < half;
    const int i0 = HF ? lane : 2 * lane;
    const int i1 = HF ? lane + half : 2 * lane + 1;
    const float c = active ? a.cs[(int64_t)p * half + lane] : 0.f;
    const float s = active ? a.sn[(int64_t)p * half + lane] : 0.f;
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
            uint16_t* dst;
            const uint16_t* nw = nullptr;
            bool rope = true;
            if (h < a.nq) {
                dst = a.q_out + m * (int64_t)QD + h * hd;
                nw = a.q_norm;
            } else if (h < a.nq + a.nkv) {
                const int g = h - a.nq;
                dst = a.kc + kv_run_off(a.km, (int64_t)a.layer * a.nkv + g, hd) + kv_tok<PG>(a.km, a.seq, cr, hd);
                nw = a.k_norm;
            } else {
                const int g = h - a.nq - a.nkv;
                dst = a.vc + kv_run_off(a.km, (int64_t)a.layer * a.nkv + g, hd) + kv_tok<PG>(a.km, a.seq, cr, hd);
                rope = false;
            }
            float y0, y1;
            qkv_post_pair<HF>(raw[b], active, rope, nw, i0, i1, c, s, hd, a.eps, y0, y1);
            if (active) {
                if (HF) {
                    dst[i0] = f2bf(y0);
                    dst[i1] = f2bf(y1);
                } else {
                    reinterpret_cast<uint32_t*>(dst)[lane] = pack2(y0, y1);
                }
            }
        }
    }
}

// ------------------------------------------- compaction of the accepted path
// Block per (layer, kv head), 512 threads.  Thread t owns one 16-byte word: depth d = 1 + t / (2 C)
// (C = hd / 8 words per row), operand K or V, word t % C of cache row p + path[d], which moves to
// row p + d.  Every thread loads before any stores (one barrier): along a path node indices rise,
// so path[d] >= d and a destination may be another depth's source, never the other way round
// after the barrier.  p, a and the path are device words; rows whose source is their destination
// and depths past a move nothing.  A row past max_ctx is never touched.
struct KvCompactArgs {
    uint16_t* kc;
    uint16_t* vc;
    KvMap km;
    int seq, nkv, hd, max_ctx;
    const int32_t* p;
    const int32_t* acc;
    const int32_t* path;
};

template <bool PG>
__global__ __launch_bounds__(512) void kv_compact_kernel(KvCompactArgs a) {
    const int C = a.hd / 8;
    const int t = threadIdx.x;
    const int d = 1 + t / (2 * C), op = (t / C) & 1, w = t % C;
    const int p = a.p[0];
    int acc = a.acc[0];
    acc = acc < 0 ? 0 : (acc > kVerifyMaxRows - 1 ? kVerifyMaxRows - 1 : acc);
    bool move = d <= acc;
    int node = move ? a.path[d] : d;
    move = move && node > d && node < kVerifyMaxRows && p >= 0 && p + node < a.max_ctx;
    uint16_t* base = (op ? a.vc : a.kc) + kv_run_off(a.km, blockIdx.x, a.hd);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (move) v = reinterpret_cast<const uint4*>(base + kv_tok<PG>(a.km, a.seq, p + node, a.hd))[w];
    __syncthreads();
    if (move) reinterpret_cast<uint4*>(base + kv_tok<PG>(a.km, a.seq, p + d, a.hd))[w] = v;
}

}  // namespace qie

using namespace qie;

extern "C" {

int qie_qkv_post_tree(const void* qkv, int32_t M, const int32_t* rope_pos, const int32_t* cache_row, int32_t seq,
                      const void* q_norm, const void* k_norm, const float* rope_cos, const float* rope_sin,
                      int32_t n_heads, const qie_kv_cache* cache, int32_t layer, float eps, int32_t numerics,
                      void* q_out, void* stream) {
    const char* who = "qie_qkv_post_tree";
    QIE_REQUIRE(qkv && rope_pos && cache_row && cache && cache->k && cache->v && rope_cos && rope_sin && q_out &&
                    M >= 1 && M <= kVerifyMaxRows && seq >= 0 && n_heads > 0 && cache->n_kv_heads > 0 &&
                    n_heads % cache->n_kv_heads == 0 && layer >= 0 && layer < cache->n_layers,
                "%s: bad arguments (1 .. %d rows)", who, kVerifyMaxRows);
    QIE_REQUIRE(cache->head_dim == 64 || cache->head_dim == 128, "%s: head_dim must be 64 or 128 (got %d)", who,
                cache->head_dim);
    QkvPostTreeArgs a;
    a.qkv = (const uint16_t*)qkv;
    a.pos = rope_pos;
    a.crow = cache_row;
    a.seq = seq;
    a.rows_per_seq = M;
    a.q_norm = (const uint16_t*)q_norm;
    a.k_norm = (const uint16_t*)k_norm;
    a.cs = rope_cos;
    a.sn = rope_sin;
    a.nq = n_heads;
    a.nkv = cache->n_kv_heads;
    a.hd = cache->head_dim;
    a.kc = (uint16_t*)cache->k;
    a.vc = (uint16_t*)cache->v;
    QIE_TRY(kv_map_make(cache, &a.km, who));
    a.layer = layer;
    a.eps = eps;
    a.numerics = numerics;
    a.q_out = (uint16_t*)q_out;
    const bool hf = numerics == QIE_NUMERICS_HF;
    auto fn = a.km.table ? (hf ? qkv_post_tree_kernel<true, true> : qkv_post_tree_kernel<true, false>)
                         : (hf ? qkv_post_tree_kernel<false, true> : qkv_post_tree_kernel<false, false>);
    hipLaunchKernelGGL(fn, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, a);
    QIE_LAUNCH_CHECK();
    return 0;
}

int qie_kv_compact(const qie_kv_cache* cache, int32_t seq, const int32_t* p_dev, const int32_t* a_dev,
                   const int32_t* path_dev, void* stream) {
    const char* who = "qie_kv_compact";
    QIE_REQUIRE(cache && cache->k && cache->v && seq >= 0 && p_dev && a_dev && path_dev && cache->n_layers > 0 &&
                    cache->n_kv_heads > 0,
                "%s: bad arguments", who);
    QIE_REQUIRE(cache->head_dim == 64 || cache->head_dim == 128, "%s: head_dim must be 64 or 128 (got %d)", who,
                cache->head_dim);
    KvCompactArgs a;
    a.kc = (uint16_t*)cache->k;
    a.vc = (uint16_t*)cache->v;
    QIE_TRY(kv_map_make(cache, &a.km, who));
    a.seq = seq, a.nkv = cache->n_kv_heads, a.hd = cache->head_dim, a.max_ctx = cache->max_ctx;
    a.p = p_dev, a.acc = a_dev, a.path = path_dev;
    auto fn = a.km.table ? kv_compact_kernel<true> : kv_compact_kernel<false>;
    hipLaunchKernelGGL(fn, dim3((unsigned)(cache->n_layers * cache->n_kv_heads)), dim3(512), 0, (hipStream_t)stream, a);
    QIE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
