// engine.hip — qie engine: weight arena, per-batch KV cache and activations,
// prefill and hipGraph-captured decode.
//
// Reference driver being replaced: llm() (layers/src/qwen_main.cu:64-417),
// create_new_sequence (iengine.cu:25-47), initialize_model_buffers
// (utills.cu:4-129), load_all_weights_to_gpu_chunked (iengine.cu:117-223),
// page list helpers (iengine.cu:73-109).  Op order per layer follows
// qwen_main.cu:77-217 (prefill) / :271-359 (decode):
//   rms -> q,k,v -> [qk-norm] -> RoPE -> KV write -> attention -> o -> +res ->
//   rms -> up, gate -> silu*up -> down -> +res;  final rms -> lm_head -> sample.
// MI355X design: the decode step is 5 launches per layer
//   [rms+QKV(+bias) GEMV] [qk-norm+RoPE+KV append] [attention(+combine)]
//   [O GEMV + residual] [rms+gate/up GEMV + SwiGLU] [down GEMV + residual]
// plus [rms+lm_head GEMV + fused arg-max] [finalize: id, position, next
// embedding], captured once into a hipGraph; positions and token ids live in
// device memory so the graph replays without host edits.
#include "qie_common.hpp"
#include "linear_plan.hpp"
#include "../../include/qie/qie_engine.h"
#include "qie_index.hpp"
#include "qie_comm.hpp"
#include "verify.hpp"
#include "row_bufs.hpp"
#include "page_pool.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <functional>
#include <vector>

namespace qie {
bool dec8_applies(const qie_linear_args* a);
int dec8_reserve(hipStream_t st);
bool dec4_applies(const qie_linear_args* a);
int dec4_reserve(hipStream_t st);
bool persist_supported(const qie_model_spec& s, int B, int tp, bool fp8, bool fp4, bool paged, int ncu, const char** why);
size_t persist_attn_table_bytes(int n_layers);
int persist_attn_table(const qie_model_spec& s, const qie_layer_weights* h_layers, const void* qkv_scratch,
                       const int32_t* pos, const float* rope_cos, const float* rope_sin, const qie_kv_cache* cache,
                       void* dec_ws, void* d_attp, hipStream_t st);
int persist_decode_launch(const qie_model_spec& s, const qie_layer_weights* d_layers, const void* d_attp,
                          uint16_t* x_res, unsigned long long* granules, const unsigned* epoch, unsigned* err,
                          const int32_t* pos, int splits_target, unsigned long long* ts, hipStream_t st);
int64_t persist_granule_count(const qie_model_spec& s);
int persist_ts_slots();
}  // namespace qie


using namespace qie;

// Tensor-parallel shard of one rank (tp = 1: the whole model).  Column-parallel
// QKV (by heads) and gate/up (by I), row-parallel O and down, vocab-parallel lm_head;
// embedding, norms and the residual stream are replicated.
// Heads: n_kv_heads % tp == 0 splits both head kinds evenly; otherwise, when
// tp % n_kv_heads == 0, every kv head is replicated on rep = tp / n_kv_heads ranks and
// the G = n_heads / n_kv_heads q heads of its group are split among those ranks as
// evenly as they go (the first G % rep ranks take one more): Qwen2-7B (28 / 4 heads) at
// TP 8 gives q heads 4,3,4,3,... with one kv head each.  Every q head lives
// on exactly one rank, so the row-parallel O all-reduce still sums each head once.
struct TpShard {
    int tp = 1, rank = 0;
    int nq = 0, nkv = 0, ffn = 0, vocab = 0;   // local counts
    int q0 = 0, kv0 = 0;                        // first global q / kv head of this rank
    int64_t vocab0 = 0;                         // first global vocab row of this rank
};

// Head split of rank `rank` of `tp` (see TpShard); false when the heads do not shard.
static bool shard_heads(int nq, int nkv, int tp, int rank, TpShard& sh) {
    if (nkv % tp == 0 && nq % tp == 0) {
        sh.nq = nq / tp;
        sh.nkv = nkv / tp;
        sh.q0 = rank * sh.nq;
        sh.kv0 = rank * sh.nkv;
        return true;
    }
    if (tp % nkv != 0) return false;
    const int rep = tp / nkv, G = nq / nkv, g = rank / rep, sub = rank % rep;
    if (rep > G) return false;   // a rank without q heads
    const int base = G / rep, extra = G % rep;
    sh.nkv = 1;
    sh.kv0 = g;
    sh.nq = base + (sub < extra ? 1 : 0);
    sh.q0 = g * G + sub * base + std::min(sub, extra);
    return true;
}

struct qie_engine {
    qie_model_spec spec{};   // the full model
    TpShard sh;              // this rank's shard
    qie_comm* comm = nullptr;
    qie_engine_opts opts{};
    hipStream_t stream = nullptr;
    void* arena = nullptr;
    size_t arena_bytes = 0;
    qie_index* index = nullptr;
    std::vector<qie_layer_weights> layers;
    qie_model_weights w{};
    bool have_weights = false;
    bool fp8 = false;            // linear weights are e4m3 + row scales (fp8_arena)
    bool fp8_t16 = false;        // ... and the decode projections in the 16-row tiled layout
    bool fp8_t16_head = false;   // ... and the lm_head too
    // fp8 engines: the same (dequantised) layer weights as bf16, in place in the arena —
    // prefill's MFMA GEMMs read these (compute-bound: the LDS-DMA bf16 kernel), decode's
    // bandwidth-bound GEMVs the fp8 codes; both compute the one dequantised model
    std::vector<qie_layer_weights> layers_pf;
    void* fp8_arena = nullptr;
    // MXFP4 projections (opts.weight_fp4): the seven layer projections as e2m1 codes + e8m0 block
    // scales in fp4_arena (e->layers points there), read by every M <= 16 launch; layers_pf holds
    // their exact dequantisation for the M > 16 GEMMs — in place in the engine's own arena, or in
    // pf_arena where the bf16 weights are the caller's (never written).  The head stays bf16, or
    // is fp8 on its own (fp8 = true) with weight_fp8.
    bool fp4 = false;
    bool fp4_t16 = false;        // ... in the 16-row tiled layout (qie_fp4_tile16)
    void* fp4_arena = nullptr;
    void* pf_arena = nullptr;
    float* rope_cos = nullptr;
    float* rope_sin = nullptr;
    int rope_rows = 0;
};

static int dmalloc(void** p, size_t bytes) {
    QIE_HIP(hipMalloc(p, bytes < 16 ? 16 : bytes));
    return 0;
}

// One device allocation that frees itself: the per-call workspaces that grow on their own
// schedule, and the timing calls' scratch
struct DevBlock {
    void* p = nullptr;
    size_t bytes = 0;
    DevBlock() = default;
    DevBlock(const DevBlock&) = delete;
    DevBlock& operator=(const DevBlock&) = delete;
    ~DevBlock() { release(); }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // at least n bytes (never null afterwards); freed before it is made anew, so the peak does
    // not double and a failure leaves nothing dangling
    int grow(size_t n) {
        if (p && n <= bytes) return 0;
        release();
        QIE_TRY(dmalloc(&p, n));
        bytes = n;
        return 0;
    }
};

// A prefix kept alive after its slot is gone (qie_batch_prefix_save): one reference
// on each of its pages and a host copy of its ids.  Host state only.
struct qie_kv_prefix {
    qie_batch* owner = nullptr;
    std::vector<int32_t> pages, ids;
};

// Device rows (row_bufs.hpp; DESIGN.md §2 "Row buffers").  Pointer stability: `dec` and `v` are
// made once and never reallocated, `pf`, `pf_ws`, `sc` and `sc_ws` grow (freed, then made anew);
// captured work (the decode graph, captured verify steps, the persistent step's attention table)
// may reference only the former.
struct qie_batch {
    qie_engine* e = nullptr;
    int B = 0, max_ctx = 0;
    // KV pools (not rows): their own allocations
    uint16_t* kc = nullptr;
    uint16_t* vc = nullptr;
    int64_t seq_stride = 0;
    int run_pad = 0;             // contiguous: run = max_ctx + run_pad tokens (dev A/B)
    DecodeRows dec;              // the B slots, made by batch_create
    std::vector<int32_t> h_pos;
    PrefillRows pf;              // prompt rows, grown to the largest prefill so far
    DevBlock pf_ws;              // its attention workspace: depends on n and on the form (short prompts split;
                                 //   an append's partials grow with its rows), not monotone in n
    // paged KV (qie_batch_create_paged): pool pages of page_tokens tokens; the host block table,
    // the free list, the pages held per slot and the count per page live in `pool`
    // (page_pool.hpp), the device table [B + 1][max_pages] mirrors its table.  Row B belongs to
    // no slot: a writer stages the shared page it is replacing there, so that qie_kv_copy can
    // read the old page and write the new one through the one table (commit_kv_writes).
    int page_tokens = 0, max_pages = 0, n_pages = 0;
    int32_t* d_table = nullptr;
    PagePool pool;
    std::vector<qie_kv_prefix*> prefixes;   // open prefix handles (dropped by qie_batch_destroy)
    std::vector<char> idle;
    bool table_dirty = false;
    // decode graph
    hipGraphExec_t gexec = nullptr;
    qie_sampling gs{};
    bool graph_ok = false;
    // qie_batch_debug_step: while set, the decode enqueue copies the residual stream after every
    // attention block and every MLP block into dbg_x ([2L + 1][B][H] bf16; slot 0 = the input)
    uint16_t* dbg_x = nullptr;
    // decode structure (qie_batch_set_decode_mode): 0 = five launches per layer, 1 = the whole
    // layer stack as one persistent launch (k_persist.hip).  pk_mem: hand-off granules, then the
    // step epoch and the error word (zeroed once; the finalize kernel advances the epoch)
    int decode_mode = 0;
    void* pk_mem = nullptr;
    qie_layer_weights* d_layers = nullptr;
    void* d_attp = nullptr;      // the attention role's parameters per layer (persist_attn_table)
    unsigned long long* pk_ts = nullptr;   // qie_batch_pk_trace: phase timestamps [cu][layer][slots]
    // speculative verify (qie_verify): the step's own rows, made once at
    // kVerifyMaxRows rows by the first call, and one captured step per (slot, rows, sampling)
    VerifyRows v;
    struct VerifyGraph {
        int seq, M;
        bool entries;   // the slot held an entry: the call's sampling is not part of the step
        bool greedy;
        qie_sampling smp;
        hipGraphExec_t exec;
        qie_row_segs segs{};   // qie_verify_batch: the table (n >= 1, and seq = -1); qie_verify: n = 0
        bool all_entries = false;   // qie_verify_batch: EVERY segment's slot held an entry (else the
                                    // call's sampling is captured for the rows of slots without one)
    };
    int v_captures = 0;   // verify steps captured so far, both kinds (qie_batch_debug_verify_captures)
    std::vector<VerifyGraph> v_graphs;
    int v_rows = 0;   // rows of the last qie_verify / qie_verify_batch (what qie_verify_logits returns)
    // the batched step (qie_verify_batch) runs on the same rows `v`, and its
    // captured steps live in v_graphs under (seq = -1, rows, the segment table, sampling).
    // vb_aux (made once by the first call): the result words [kVerifyBatchResWords], then the
    // rows' slots, tail offsets and tail lengths [kVerifyMaxRows] each
    int32_t* vb_aux = nullptr;
    // scoring (qie_score, qie_batch_logprobs): device targets, log-probabilities and
    // greedy ids of sc.rows rows, and the fused head's workspace; grown before any launch
    ScoreRows sc;
    DevBlock sc_ws;
    // per-slot sampling entries (qie_batch_set_slot_sampling): the host copies, and
    // from the first set on the device table [B] (n_bias < 0: no entry) followed by the verify
    // rows' tail lengths 0 .. kVerifyMaxRows - 1, and qie_sample_rows' own workspace.  Both are
    // made once and never reallocated: captured steps hold their pointers.
    std::vector<qie_slot_sampling> slot_h;
    std::vector<char> slot_set;
    int n_slot_set = 0;
    qie_slot_sampling* d_slots = nullptr;
    int32_t* d_tail_len = nullptr;
    void* rows_ws = nullptr;
    bool g_entries = false;   // the decode graph was captured on the entry path
};

namespace qie {

// ------------------------------------------------------------ small kernels
// Step finalisation: chosen id -> token history, position + 1, sample step + 1,
// next step's input row x_res[m] = E[id] (embedding_matrix_func, decode branch
// qwen_main.cu:259-268, without the host round trip).
// (the slot's current-position RoPE row: RopeCurArgs / write_rope_cur, qie_common.hpp)
__global__ __launch_bounds__(256) void finalize_kernel(int m0, unsigned long long* keys, const int32_t* ids_in,
                                                       int32_t* ids_out, int32_t* pos, int32_t* step,
                                                       int32_t* hist, int hist_stride, const uint4* E,
                                                       uint4* x_res, int64_t H8, int32_t vocab, RopeCurArgs rca,
                                                       unsigned* pk_epoch) {
    const int m = m0 + blockIdx.x;
    // the persistent step's hand-off epoch advances once per step (k_persist.hip tags)
    if (pk_epoch && blockIdx.x == 0 && threadIdx.x == 0) *pk_epoch += 1u;
    int32_t tok = keys ? key_idx(keys[m]) : ids_in[m];
    const int32_t p = pos[m];
    __syncthreads();
    if (tok < 0 || tok >= vocab) tok = 0;
    if (threadIdx.x == 0) {
        if (keys) keys[m] = 0ull;
        if (p + 1 < hist_stride) hist[(int64_t)m * hist_stride + p + 1] = tok;
        pos[m] = p + 1;
        step[m] = step[m] + 1;
        ids_out[m] = tok;
    }
    write_rope_cur(rca, m, p + 1);
    const uint4* src = E + (int64_t)tok * H8;
    uint4* dst = x_res + (int64_t)m * H8;
    for (int64_t i = threadIdx.x; i < H8; i += 256) dst[i] = src[i];
}

__global__ void set_state_kernel(int m, int32_t pos_v, int32_t step_v, int32_t tok, int32_t* pos,
                                 int32_t* step, int32_t* hist, int hist_stride, const uint4* E,
                                 uint4* x_res, int64_t H8, int write_row, RopeCurArgs rca) {
    write_rope_cur(rca, m, pos_v);
    if (threadIdx.x == 0) {
        pos[m] = pos_v;
        step[m] = step_v;
        if (pos_v >= 0 && pos_v < hist_stride) hist[(int64_t)m * hist_stride + pos_v] = tok;
    }
    if (write_row)
        for (int64_t i = threadIdx.x; i < H8; i += blockDim.x) x_res[(int64_t)m * H8 + i] = E[(int64_t)tok * H8 + i];
}

// positions of n_seqs equal-length prompts laid end to end: row i sits at i % len
// (plus base: an append's rows start at its pos0)
__global__ void iota_kernel(int32_t* p, int n, int len, int base) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = base + i % len;
}

// prompt z (blockIdx.y) of len ids -> history row z of dst (stride dst_stride)
__global__ void copy_ids_kernel(const int32_t* src, int32_t* dst, int len, int64_t dst_stride) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) dst[blockIdx.y * dst_stride + i] = src[(int64_t)blockIdx.y * len + i];
}

// qie_prefill_ragged's form of the two kernels above: row i of segment z (the table travels by
// value) sits at pos0[z] + i - row0[z], and its id lands there in history row seq[z]
struct RaggedRows {
    qie_row_segs segs;
    int32_t pos0[QIE_RAGGED_MAX_SEGS];
};
__global__ void ragged_rows_kernel(RaggedRows t, const int32_t* ids, int32_t* pos, int32_t* hist, int64_t hist_stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.segs.row0[QIE_RAGGED_MAX_SEGS]) return;   // the caller repeats M in the unused entries
    int row0 = 0, seq = t.segs.seq[0], p0 = t.pos0[0];   // constant indices only
#pragma unroll
    for (int z = 1; z < QIE_RAGGED_MAX_SEGS; z++)
        if (z < t.segs.n && i >= t.segs.row0[z]) row0 = t.segs.row0[z], seq = t.segs.seq[z], p0 = t.pos0[z];
    const int p = p0 + i - row0;
    pos[i] = p;
    hist[seq * hist_stride + p] = ids[i];
}

static RopeCurArgs rope_cur_args(const qie_batch* b) {
    const qie_engine* e = b->e;
    return RopeCurArgs{b->dec.rope_cur, e->rope_cos, e->rope_sin, (int)e->spec.head_dim, e->rope_rows};
}

// Enqueues set_state_kernel for one slot: position, step counter, history[pos] = tok and the RoPE
// row; write_row: also the next input row x[slot] = E[tok].
static int set_slot_state(qie_batch* b, int slot, int pos, int step, int tok, int write_row) {
    const qie_engine* e = b->e;
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(256), 0, e->stream, slot, pos, step, tok, b->dec.pos, b->dec.step,
                       b->dec.hist, b->max_ctx, (const uint4*)e->w.embed, (uint4*)b->dec.x, (int64_t)e->spec.hidden / 8,
                       write_row, rope_cur_args(b));
    QIE_LAUNCH_CHECK();
    return 0;
}

// KV descriptor of the batch's sequences seq0.. (kernels see them as sequences 0..)
static qie_kv_cache batch_cache(const qie_batch* b, int seq0) {
    const qie_engine* e = b->e;
    qie_kv_cache c{};
    c.n_layers = e->spec.n_layers;
    c.n_kv_heads = e->sh.nkv;
    c.head_dim = e->spec.head_dim;
    c.max_ctx = b->max_ctx + b->run_pad;   // the run length (positions stay below b->max_ctx)
    c.seq_stride = b->seq_stride;
    if (b->d_table) {
        c.k = b->kc;
        c.v = b->vc;
        c.block_table = b->d_table + (int64_t)seq0 * b->max_pages;
        c.page_tokens = b->page_tokens;
        c.max_pages = b->max_pages;
    } else {
        c.k = b->kc + (int64_t)seq0 * b->seq_stride;
        c.v = b->vc + (int64_t)seq0 * b->seq_stride;
    }
    return c;
}

static int build_rope(qie_engine* e) {
    const int hd = e->spec.head_dim, half = hd / 2, rows = e->opts.max_ctx;
    std::vector<float> c((size_t)rows * half), s((size_t)rows * half);
    QIE_TRY(qie_rope_table_host(c.data(), s.data(), rows, hd, e->spec.rope_theta, e->spec.numerics));
    QIE_TRY(dmalloc((void**)&e->rope_cos, c.size() * 4));
    QIE_TRY(dmalloc((void**)&e->rope_sin, s.size() * 4));
    QIE_HIP(hipMemcpyAsync(e->rope_cos, c.data(), c.size() * 4, hipMemcpyHostToDevice, e->stream));
    QIE_HIP(hipMemcpyAsync(e->rope_sin, s.data(), s.size() * 4, hipMemcpyHostToDevice, e->stream));
    QIE_HIP(hipStreamSynchronize(e->stream));   // the host tables go out of scope
    e->rope_rows = rows;
    return 0;
}

static int check_align(const void* p, const char* what, int layer) {
    if (((uintptr_t)p) % 16 != 0)
        return fail(-22, "weight %s (layer %d) is not 16-byte aligned", what, layer);
    return 0;
}

// fp8 weights (opts.weight_fp8): every linear weight and the lm_head are quantised on
// device into a second arena (OCP e4m3 codes + power-of-two row scales, qie_ops.h) and
// the layer pointers switched to it; embeddings, norms and biases stay bf16 in the
// first arena (a tied embedding keeps its bf16 copy for the token gather).
// own_arena: the bf16 weights live in the engine's arena (synthetic init, weights.bin), so
// they may be rewritten with their dequantisation for prefill; caller-owned weights
// (qie_engine_set_weights) are never written — their prefill takes the fp8 GEMM path.
static bool dec8_takes_tiled_projections(const qie_engine* e);   // (beside the projection builders)
// head_only (weight_fp4 + weight_fp8): the lm_head alone; the projections are MXFP4's.
static int quantize_weights_fp8(qie_engine* e, bool own_arena, bool head_only = false) {
    QIE_REQUIRE(e->sh.tp == 1, "fp8 weights with tensor parallelism are not supported yet");
    const qie_model_spec& s = e->spec;
    const int64_t H = s.hidden, QD = (int64_t)s.n_heads * s.head_dim, KD = (int64_t)s.n_kv_heads * s.head_dim;
    const int64_t I = s.ffn, V = s.vocab;
    QIE_REQUIRE(H % 16 == 0 && QD % 16 == 0 && I % 16 == 0, "fp8 weights need hidden, q dim and ffn % 16 == 0");
    struct Slot { const void** p; int64_t rows, cols; };
    std::vector<Slot> ts;
    for (auto& L : e->layers) {
        if (head_only) break;
        ts.push_back({&L.wq, QD, H});
        ts.push_back({&L.wk, KD, H});
        ts.push_back({&L.wv, KD, H});
        ts.push_back({&L.wo, H, QD});
        ts.push_back({&L.w_gate, I, H});
        ts.push_back({&L.w_up, I, H});
        ts.push_back({&L.w_down, H, I});
    }
    ts.push_back({&e->w.lm_head, V, H});
    size_t total = 0;
    for (auto& t : ts) total += (size_t)((qie_fp8_weight_bytes(t.rows, t.cols) + 255) / 256 * 256);
    if (e->fp8_arena) hipFree(e->fp8_arena);
    e->fp8_arena = nullptr;
    QIE_HIP(hipMalloc(&e->fp8_arena, total));
    char* dst = (char*)e->fp8_arena;
    if (!head_only) e->layers_pf.clear();
    if (own_arena && !head_only) e->layers_pf = e->layers;   // bf16 arena pointers, rewritten below with the dequantised values
    for (auto& t : ts) {
        const void* src = *t.p;
        QIE_TRY(qie_quantize_fp8(src, t.rows, t.cols, dst, e->stream));
        // layer weights: the arena copy becomes the exact dequantisation (prefill reads it);
        // the lm_head is left alone (a tied one is also the embedding table)
        if (own_arena && t.p != &e->w.lm_head)
            QIE_TRY(qie_dequantize_fp8(dst, t.rows, t.cols, const_cast<void*>(src), e->stream));
        *t.p = dst;
        dst += (qie_fp8_weight_bytes(t.rows, t.cols) + 255) / 256 * 256;
    }
    QIE_HIP(hipStreamSynchronize(e->stream));
    // prefill_fp8: the block-scaled GEMM takes only the exponent field of a weight row scale
    // (qie_ops.h QIE_LINEAR_ACT_FP8), so every projection's scales must be positive normal
    // powers of two; checked once here, where they are made
    if (e->opts.prefill_fp8) {
        std::vector<uint32_t> sc;
        for (auto& t : ts) {
            if (t.p == &e->w.lm_head) continue;
            sc.resize((size_t)t.rows);
            QIE_HIP(hipMemcpy(sc.data(), (const char*)*t.p + t.rows * t.cols, (size_t)t.rows * 4, hipMemcpyDeviceToHost));
            for (const uint32_t b : sc)
                QIE_REQUIRE((b & 0x807fffffu) == 0 && (b >> 23) != 0 && (b >> 23) != 255,
                            "prefill_fp8: an fp8 weight row scale (bits 0x%08x) is not a normal power of two", b);
        }
    }
    e->w.layers = e->layers.data();
    e->fp8 = true;
    e->fp8_t16 = e->fp8_t16_head = false;
    // The decode projections go to the 16-row tiled layout (qie_fp8_tile16: every 1-KiB wave
    // load of the batched-decode kernel contiguous) when that kernel takes every one of them
    // at any batch (it is then their only reader; prefill reads the dequantised bf16 copy, so
    // the engine must own its arena).  QIE_FP8_T16=0 (dev) keeps the plain layout.
    if (own_arena && dev_env("QIE_FP8_T16", 1) != 0) {
        const bool all = dec8_takes_tiled_projections(e);
        // the vocabulary projection too: its readers (the decode step's and the prefill's
        // last-row heads, <= 8 rows) run the skinny kernel, which reads the tiled layout
        // (through the batched-decode kernel instead — one 7-wave block per CU, ~37 tiles
        // each — config 4's lm_head took 168.9 vs 119-120 µs plain); dev QIE_FP8_T16_HEAD=0
        // keeps it plain
        const bool head = all && dev_env("QIE_FP8_T16_HEAD", 1) != 0 && H % 64 == 0 && V % 16 == 0 &&
                          (size_t)8 * (H + 8) * 2 <= 120 * 1024;
        if (all) {
            size_t big = 0;
            for (auto& t : ts)
                if (t.p != &e->w.lm_head || head) big = std::max<size_t>(big, (size_t)qie_fp8_weight_bytes(t.rows, t.cols));
            void* tmp = nullptr;
            QIE_TRY(dmalloc(&tmp, big));
            int rc = 0;
            for (auto& t : ts) {
                if (t.p == &e->w.lm_head && !head) continue;
                const size_t nb = (size_t)qie_fp8_weight_bytes(t.rows, t.cols);
                rc = qie_fp8_tile16(*t.p, t.rows, t.cols, tmp, e->stream);
                if (rc) break;
                if (hipMemcpyAsync(const_cast<void*>(*t.p), tmp, nb, hipMemcpyDeviceToDevice, e->stream) != hipSuccess) {
                    rc = fail(-5, "fp8 tiling: copy failed");
                    break;
                }
            }
            if (!rc && hipStreamSynchronize(e->stream) != hipSuccess) rc = fail(-5, "fp8 tiling: synchronize failed");
            hipFree(tmp);
            if (rc) return rc;
            e->fp8_t16 = !head_only;
            e->fp8_t16_head = head;
        }
    }
    return 0;
}

// MXFP4 projections (opts.weight_fp4), beside the fp8 form above: the seven projections of every
// layer are quantised on device into fp4_arena (qie_ops.h: e2m1 codes in 32-element blocks + e8m0
// scales), tiled (qie_fp4_tile16) where every segment is whole 16-row tiles, and the layer
// pointers switched to it.  Their exact dequantisation, which the M > 16 GEMMs read (layers_pf),
// replaces the bf16 values in the engine's own arena; caller-owned weights are never written: the
// dequantised copies go to a private allocation (pf_arena).  Embeddings, norms, biases and the
// lm_head stay as they are; with weight_fp8 the lm_head alone is then quantised to fp8.
static bool fp4_takes_projections(const qie_engine* e, int flags);   // (beside the projection builders)
static int quantize_weights_fp4(qie_engine* e, bool own_arena) {
    QIE_REQUIRE(e->sh.tp == 1, "fp4 weights with tensor parallelism are not supported");
    const qie_model_spec& s = e->spec;
    const int64_t H = s.hidden, QD = (int64_t)s.n_heads * s.head_dim, KD = (int64_t)s.n_kv_heads * s.head_dim;
    const int64_t I = s.ffn;
    QIE_REQUIRE(fp4_takes_projections(e, QIE_LINEAR_FP4),
                "fp4 weights: the MXFP4 kernel does not take this model's projections (hidden %lld, q dim %lld, ffn %lld)",
                (long long)H, (long long)QD, (long long)I);
    struct Slot { const void** p; int64_t rows, cols; };
    std::vector<Slot> ts;
    for (auto& L : e->layers) {
        ts.push_back({&L.wq, QD, H});
        ts.push_back({&L.wk, KD, H});
        ts.push_back({&L.wv, KD, H});
        ts.push_back({&L.wo, H, QD});
        ts.push_back({&L.w_gate, I, H});
        ts.push_back({&L.w_up, I, H});
        ts.push_back({&L.w_down, H, I});
    }
    auto a256 = [](int64_t n) { return (size_t)((n + 255) / 256 * 256); };
    size_t total = 0, total_pf = 0, big = 0;
    for (auto& t : ts) {
        total += a256(qie_fp4_weight_bytes(t.rows, t.cols));
        total_pf += a256(t.rows * t.cols * 2);
        big = std::max(big, (size_t)qie_fp4_weight_bytes(t.rows, t.cols));
    }
    if (e->fp4_arena) hipFree(e->fp4_arena);
    if (e->pf_arena) hipFree(e->pf_arena);
    e->fp4_arena = e->pf_arena = nullptr;
    QIE_HIP(hipMalloc(&e->fp4_arena, total));
    if (!own_arena) QIE_HIP(hipMalloc(&e->pf_arena, total_pf));
    const bool tile = fp4_takes_projections(e, QIE_LINEAR_FP4 | QIE_LINEAR_FP4_T16);
    void* tmp = nullptr;
    if (tile) QIE_TRY(dmalloc(&tmp, big));
    e->layers_pf = e->layers;   // the bf16 pointers; the projections' are replaced below where the copy is private
    std::vector<const void*> pf_ptr(ts.size());
    char* dst = (char*)e->fp4_arena;
    char* pf = (char*)e->pf_arena;
    int rc = 0;
    for (size_t i = 0; i < ts.size() && !rc; i++) {
        const Slot& t = ts[i];
        const void* src = *t.p;
        void* plain = tile ? tmp : (void*)dst;
        rc = qie_quantize_fp4(src, t.rows, t.cols, plain, e->stream);
        void* deq = own_arena ? const_cast<void*>(src) : (void*)pf;
        if (!rc) rc = qie_dequantize_fp4(plain, t.rows, t.cols, deq, e->stream);
        if (!rc && tile) rc = qie_fp4_tile16(tmp, t.rows, t.cols, dst, e->stream);
        pf_ptr[i] = deq;
        *t.p = dst;
        dst += a256(qie_fp4_weight_bytes(t.rows, t.cols));
        if (!own_arena) pf += a256(t.rows * t.cols * 2);
    }
    if (!rc && hipStreamSynchronize(e->stream) != hipSuccess) rc = fail(-5, "fp4 quantisation: synchronize failed");
    if (tmp) hipFree(tmp);
    if (rc) return rc;
    for (size_t l = 0; l < e->layers_pf.size(); l++) {
        qie_layer_weights& L = e->layers_pf[l];
        const void** slots[7] = {&L.wq, &L.wk, &L.wv, &L.wo, &L.w_gate, &L.w_up, &L.w_down};
        for (int j = 0; j < 7; j++) *slots[j] = pf_ptr[l * 7 + j];
    }
    e->w.layers = e->layers.data();
    e->fp4 = true;
    e->fp4_t16 = tile;
    e->fp8 = e->fp8_t16 = e->fp8_t16_head = false;
    return e->opts.weight_fp8 ? quantize_weights_fp8(e, own_arena, true) : 0;
}
// after the weights are bound: the quantised forms the options ask for
static int quantize_weights(qie_engine* e, bool own_arena) {
    if (e->opts.weight_fp4) return quantize_weights_fp4(e, own_arena);
    return e->opts.weight_fp8 ? quantize_weights_fp8(e, own_arena) : 0;
}

// Resolve role pointers from the reference index (short_name, layer) ->
// arena + data_offsets[0]  (assign_weight_pointer, helpers.cuh:19-30).
static int bind_from_index(qie_engine* e) {
    const qie_model_spec& s = e->spec;
    char* base = (char*)e->arena;
    auto get = [&](const char* sn, int layer, const void** out, bool required) -> int {
        const qie_index_entry* t = index_find(e->index, sn, layer);
        if (!t) {
            if (required) return fail(-22, "tensor %s (layer %d) missing from index", sn, layer);
            *out = nullptr;
            return 0;
        }
        *out = base + t->off0;
        return check_align(*out, sn, layer);
    };
    e->layers.assign(s.n_layers, qie_layer_weights{});
    for (int l = 0; l < s.n_layers; l++) {
        qie_layer_weights& L = e->layers[l];
        QIE_TRY(get("input_layernorm.weight", l, &L.attn_norm, true));
        QIE_TRY(get("self_attn.q_proj.weight", l, &L.wq, true));
        QIE_TRY(get("self_attn.k_proj.weight", l, &L.wk, true));
        QIE_TRY(get("self_attn.v_proj.weight", l, &L.wv, true));
        QIE_TRY(get("self_attn.q_proj.bias", l, &L.bq, s.qkv_bias != 0));
        QIE_TRY(get("self_attn.k_proj.bias", l, &L.bk, s.qkv_bias != 0));
        QIE_TRY(get("self_attn.v_proj.bias", l, &L.bv, s.qkv_bias != 0));
        QIE_TRY(get("self_attn.q_norm.weight", l, &L.q_norm, s.qk_norm != 0));
        QIE_TRY(get("self_attn.k_norm.weight", l, &L.k_norm, s.qk_norm != 0));
        QIE_TRY(get("self_attn.o_proj.weight", l, &L.wo, true));
        QIE_TRY(get("post_attention_layernorm.weight", l, &L.ffn_norm, true));
        QIE_TRY(get("mlp.gate_proj.weight", l, &L.w_gate, true));
        QIE_TRY(get("mlp.up_proj.weight", l, &L.w_up, true));
        QIE_TRY(get("mlp.down_proj.weight", l, &L.w_down, true));
    }
    QIE_TRY(get("embed_tokens.weight", -1, &e->w.embed, true));
    QIE_TRY(get("norm.weight", -1, &e->w.final_norm, true));
    if (s.tie_embeddings && e->sh.tp == 1) e->w.lm_head = e->w.embed;
    else QIE_TRY(get("logits", -1, &e->w.lm_head, true));
    e->w.n_layers = s.n_layers;
    e->w.layers = e->layers.data();
    e->have_weights = true;
    return quantize_weights(e, true);
}

// ------------------------------------------------------------- enqueue helpers
static qie_linear_args lin_args(int flags) {
    qie_linear_args a;
    std::memset(&a, 0, sizeof(a));
    a.flags = flags;
    return a;
}
// every weight linear of the engine: fp8 weights when the engine quantised them
static int lin_flags(const qie_engine* e) { return e->fp8 ? QIE_LINEAR_FP8 : 0; }
// the layer projections (QKV, O, gate/up, down): + the tiled-layout flag where they are tiled
static int proj_flags(const qie_engine* e) {
    if (e->fp4) return QIE_LINEAR_FP4 | (e->fp4_t16 ? QIE_LINEAR_FP4_T16 : 0);
    return lin_flags(e) | (e->fp8_t16 ? QIE_LINEAR_FP8_T16 : 0);
}

// The exchange steps go through the communicator under tensor parallelism, and at world 1
// when the engine was asked to (opts.comm_always: the captured-collective path on one GPU).
static bool use_comm(const qie_engine* e) { return e->comm && (e->sh.tp > 1 || e->opts.comm_always); }

// Device -> host on the engine stream (then wait): never the legacy null stream, whose
// implicit ordering against every blocking stream HIP refuses while ANY thread of the process
// captures a graph (the TP ranks of one process capture their decode graphs concurrently).
static hipError_t d2h(const qie_engine* e, void* dst, const void* src, size_t bytes) {
    hipError_t he = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    return he;
}

// After a stream synchronisation: a device-side exchange failure (the peer backend's bounded
// wait) makes the call fail instead of returning ids computed from a partial exchange.
static int comm_fail(const char* who, long long err) {
    return fail(-7, "%s: tensor-parallel exchange failed on the device (error word %lld: a peer rank did "
                    "not arrive within the bounded wait); the communicator is unusable", who, err);
}
static int comm_check(const qie_engine* e, const char* who) {
    if (!use_comm(e)) return 0;
    const int err = e->comm->error_state(e->stream);
    return err ? comm_fail(who, err) : 0;
}

// Row-parallel projection epilogue under tensor parallelism: fp32 partials -> all-reduce
// -> x = bf16(x + bf16(sum)); the single-GPU path fuses the residual into the GEMV/GEMM.
static int row_parallel(qie_batch* b, qie_linear_args& a, uint16_t* x, float* part, int64_t rows) {
    qie_engine* e = b->e;
    if (!use_comm(e)) {
        a.y = x;
        a.epilogue = QIE_EPI_RESIDUAL;
        return qie_linear(&a, e->stream);
    }
    a.y = part;
    a.epilogue = QIE_EPI_F32;
    const int64_t n = rows * e->spec.hidden;
    // peer backend, one row: the GEMV's epilogue pushes each finished output straight into
    // every rank's tagged exchange slot (the send overlaps the projection's tail), and the
    // exchange kernel only waits, reduces and adds (comm.hip peer_tag_kernel)
    PeerPush pp;
    if (rows == 1 && e->comm->peer_push(&pp, n)) {
        bool taken = false;
        LinearExtras ex;
        ex.push = &pp;
        ex.push_taken = &taken;
        QIE_TRY(linear(&a, ex, e->stream));
        if (taken) return e->comm->allreduce_residual_pushed(x, n, e->stream);
        return e->comm->allreduce_residual_bf16(part, x, n, e->stream);
    }
    QIE_TRY(qie_linear(&a, e->stream));
    return e->comm->allreduce_residual_bf16(part, x, n, e->stream);   // one kernel on the peer backend
}

// Batched rows (2 <= M <= 16, the skinny MFMA kernel): RMSNorm the M rows once into xn [M][K]
// (qie_rmsnorm, normalization.cu:5-25 semantics) and feed the projection plain rows.  The
// skinny kernel's fused norm prologue recomputed every row's norm in every workgroup and
// cost 13-16 us per launch at B = 8 (tools/ubench_b8.py, QIE_SKINNY_DBG); M = 1 keeps the
// GEMV's fused x-first prologue.  QIE_PRENORM=0 restores the fused form (A/B).
// The decision (qie_batch_time_kernel applies it without launching a norm) ...
static bool prenorm_applies(const qie_linear_args& a) {
    static const int on = dev_env("QIE_PRENORM", 1);
    if (!on || a.M < 2 || a.M > 16 || !a.norm_w) return false;
    if (a.flags & QIE_LINEAR_FP4) return false;   // the MXFP4 kernel fuses the norm at every M it takes
    return !dec8_applies(&a) || dev_env("QIE_DEC8_PRENORM", 0) != 0;   // the fp8 batched-decode kernel fuses the norm
}
// ... and the action: the projection reads the normed rows xn instead of norming x itself
static void take_normed(qie_linear_args& a, const uint16_t* xn) {
    a.x = xn;
    a.ldx = a.K;
    a.norm_w = nullptr;
}
static int norm_rows(qie_batch* b, qie_linear_args& a, uint16_t* xn) {
    QIE_TRY(qie_rmsnorm(a.x, a.norm_w, xn, a.M, a.K, a.norm_eps, a.numerics, b->e->stream));
    take_normed(a, xn);
    return 0;
}
static int prenorm(qie_batch* b, qie_linear_args& a, uint16_t* xn) {
    return prenorm_applies(a) ? norm_rows(b, a, xn) : 0;
}

// batch 1, REF numerics, no qk-norm (Qwen2): the decode QKV projection's epilogue rotates q
// and k (LinearExtras::rope), so the attention's critical path loses the position -> RoPE-table round
// trip (QIE_ATTN_PREROPED)
static bool rope_in_projection(const qie_batch* b) {
    const qie_model_spec& s = b->e->spec;
    if (b->e->fp4) return false;   // the MXFP4 kernel has no RoPE epilogue: the attention launch rotates
    return b->B == 1 && !s.qk_norm && s.numerics == QIE_NUMERICS_REF && dev_env("QIE_ROPE_IN_PROJ", 0) != 0;
}

// qie_batch_debug_step: residual stream snapshot `slot` (eager step only, never captured)
static int dbg_snap(qie_batch* b, int slot) {
    if (!b->dbg_x) return 0;
    const int64_t n = (int64_t)b->B * b->e->spec.hidden;
    QIE_HIP(hipMemcpyAsync(b->dbg_x + slot * n, b->dec.x, (size_t)n * 2, hipMemcpyDeviceToDevice, b->e->stream));
    return 0;
}

// The four projections of a layer, described once: [norm + QKV (+ bias)], [O], [norm + gate/up +
// SwiGLU], [down].  L: the layer's weights (e->layers[l], or the dequantised e->layers_pf[l]);
// flags: proj_flags(e), less the fp8 bits on the dequantised copy.  Nothing is launched; O and
// down get their output and epilogue from row_parallel.
static qie_linear_args qkv_args(const qie_engine* e, const qie_layer_weights& L, int flags, const LayerRows& r) {
    const qie_model_spec& s = e->spec;
    const int64_t H = s.hidden, QD = (int64_t)e->sh.nq * s.head_dim, KD = (int64_t)e->sh.nkv * s.head_dim;
    qie_linear_args a = lin_args(flags);
    a.x = r.x; a.ldx = H;
    a.w[0] = L.wq; a.w[1] = L.wk; a.w[2] = L.wv;
    a.bias[0] = L.bq; a.bias[1] = L.bk; a.bias[2] = L.bv;
    a.seg_rows[0] = QD; a.seg_rows[1] = KD; a.seg_rows[2] = KD;
    a.M = r.M; a.K = H; a.N = QD + 2 * KD;
    a.y = r.qkv; a.ldy = QD + 2 * KD;
    a.epilogue = QIE_EPI_STORE;
    a.norm_w = L.attn_norm; a.norm_eps = s.rms_eps; a.numerics = s.numerics;
    return a;
}
static qie_linear_args o_args(const qie_engine* e, const qie_layer_weights& L, int flags, const LayerRows& r) {
    const int64_t H = e->spec.hidden, QD = (int64_t)e->sh.nq * e->spec.head_dim;
    qie_linear_args a = lin_args(flags);
    a.x = r.att; a.ldx = QD;
    a.w[0] = L.wo; a.seg_rows[0] = H;
    a.M = r.M; a.K = QD; a.N = H;
    a.ldy = H;
    return a;
}
static qie_linear_args gate_up_args(const qie_engine* e, const qie_layer_weights& L, int flags, const LayerRows& r) {
    const qie_model_spec& s = e->spec;
    const int64_t H = s.hidden, I = e->sh.ffn;
    qie_linear_args a = lin_args(flags);
    a.x = r.x; a.ldx = H;
    a.w[0] = L.w_gate; a.w[1] = L.w_up; a.seg_rows[0] = I; a.seg_rows[1] = I;
    a.M = r.M; a.K = H; a.N = I;
    a.y = r.h; a.ldy = I;
    a.epilogue = QIE_EPI_SWIGLU;
    a.norm_w = L.ffn_norm; a.norm_eps = s.rms_eps; a.numerics = s.numerics;
    return a;
}
static qie_linear_args down_args(const qie_engine* e, const qie_layer_weights& L, int flags, const LayerRows& r) {
    const int64_t H = e->spec.hidden, I = e->sh.ffn;
    qie_linear_args a = lin_args(flags);
    a.x = r.h; a.ldx = I;
    a.w[0] = L.w_down; a.seg_rows[0] = H;
    a.M = r.M; a.K = I; a.N = H;
    a.ldy = H;
    return a;
}

// quantize_weights_fp8: whether the fp8 batched-decode kernel takes every projection of the
// decode step from 16-row tiled weights, already at one row (then it is their only reader)
static bool dec8_takes_tiled_projections(const qie_engine* e) {
    const LayerRows r{1};
    const qie_layer_weights& L = e->layers[0];
    const int fl = QIE_LINEAR_FP8 | QIE_LINEAR_FP8_T16;
    qie_linear_args o = o_args(e, L, fl, r), down = down_args(e, L, fl, r);
    o.epilogue = down.epilogue = QIE_EPI_RESIDUAL;   // as row_parallel launches them on one GPU
    const qie_linear_args all[] = {qkv_args(e, L, fl, r), o, gate_up_args(e, L, fl, r), down};
    for (const qie_linear_args& a : all)
        if (!dec8_applies(&a)) return false;
    return true;
}

// quantize_weights_fp4 / qie_engine_create: whether the MXFP4 kernel takes all four projection
// launches of a layer under `flags` (plain or tiled); the plan does not depend on M <= 16 or on
// the pointers, so a spec is enough
static bool fp4_takes_spec(const qie_model_spec& s, int flags) {
    qie_engine probe;
    probe.spec = s;
    probe.sh.nq = s.n_heads, probe.sh.nkv = s.n_kv_heads, probe.sh.ffn = s.ffn;
    const LayerRows r{1};
    qie_layer_weights L{};
    qie_linear_args o = o_args(&probe, L, flags, r), down = down_args(&probe, L, flags, r);
    o.epilogue = down.epilogue = QIE_EPI_RESIDUAL;
    const qie_linear_args all[] = {qkv_args(&probe, L, flags, r), o, gate_up_args(&probe, L, flags, r), down};
    for (qie_linear_args a : all) {
        if (a.epilogue == QIE_EPI_STORE || a.epilogue == QIE_EPI_SWIGLU) a.norm_w = &probe;   // (planned as fused; not read)
        if (!dec4_applies(&a)) return false;
    }
    return true;
}
static bool fp4_takes_projections(const qie_engine* e, int flags) { return fp4_takes_spec(e->spec, flags); }

// How a built projection gets its input, applied before the launch:
//   Decode  prenorm()'s rule (2..16 rows: norm once into the rows' xn; else the fused norm)
//   Normed  RMSNorm into xn at every row count (prefill)
//   Fp8     Normed (no norm for O and down), then the rows quantised per row to e4m3 codes +
//           exponents (opts.prefill_fp8: QIE_LINEAR_ACT_FP8 on the block-scaled MFMA GEMM)
enum class InputForm { Decode, Normed, Fp8 };
static int stage_input(qie_batch* b, InputForm form, qie_linear_args& a, const LayerRows& r) {
    if (form == InputForm::Decode) return prenorm(b, a, r.xn);
    if (a.norm_w) QIE_TRY(norm_rows(b, a, r.xn));
    if (form == InputForm::Normed) return 0;
    QIE_TRY(qie_quantize_rows_fp8(a.x, a.ldx, a.M, a.K, b->pf.q8, a.K, b->pf.e8, b->e->stream));
    a.x = b->pf.q8; a.ldx = a.K; a.x_exps = b->pf.e8;
    a.flags |= QIE_LINEAR_ACT_FP8;
    return 0;
}

// Which weight table a step's projections read, with which base flags and input form
struct LayerPath {
    const qie_layer_weights* layers;
    int flags;
    InputForm in;
};
static LayerPath decode_path(const qie_engine* e) { return LayerPath{e->layers.data(), proj_flags(e), InputForm::Decode}; }

// input stage, then the launch: QKV and gate/up as built ...
static int run_proj(qie_batch* b, qie_linear_args a, InputForm in, const LayerRows& r,
                    const LinearExtras& ex = LinearExtras{}) {
    QIE_TRY(stage_input(b, in, a, r));
    return linear(&a, ex, b->e->stream);
}
// ... O and down in residual or exchange form
static int run_row_proj(qie_batch* b, qie_linear_args a, InputForm in, const LayerRows& r) {
    QIE_TRY(stage_input(b, in, a, r));
    return row_parallel(b, a, r.x, r.part, r.M);
}

// the decode QKV projection's fused RoPE (rope_in_projection)
static LinearExtras decode_qkv_extras(const qie_batch* b) {
    const qie_engine* e = b->e;
    const int64_t hd = e->spec.head_dim;
    LinearExtras ex;
    if (rope_in_projection(b)) ex.rope = RopeArgs{b->dec.pos, e->rope_cos, e->rope_sin, (int)hd, (e->sh.nq + e->sh.nkv) * hd};
    return ex;
}
// the decode step's attention of layer l into out ([B][QD]: b->dec.att, or the timing call's scratch)
static int attend_decode(qie_batch* b, int l, void* out) {
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    const qie_layer_weights& L = e->layers[l];
    const qie_kv_cache cache = batch_cache(b, 0);
    set_decode_rope_cur(b->dec.rope_cur);
    const int rc = qie_attention_decode(b->dec.qkv, b->B, b->dec.pos, L.q_norm, L.k_norm, e->rope_cos, e->rope_sin, e->sh.nq,
                                        &cache, l, s.rms_eps,
                                        s.numerics | (rope_in_projection(b) ? QIE_ATTN_PREROPED : 0), out, b->dec.dec_ws,
                                        e->stream);
    set_decode_rope_cur(nullptr);
    return rc;
}

static int enqueue_layer_decode(qie_batch* b, int l) {
    qie_engine* e = b->e;
    const LayerPath p = decode_path(e);
    const qie_layer_weights& L = p.layers[l];
    const LayerRows r = layer_rows(b->dec, b->B, 1);
    QIE_TRY(run_proj(b, qkv_args(e, L, p.flags, r), p.in, r, decode_qkv_extras(b)));
    QIE_TRY(attend_decode(b, l, r.att));
    QIE_TRY(run_row_proj(b, o_args(e, L, p.flags, r), p.in, r));
    QIE_TRY(dbg_snap(b, 2 * l + 1));
    QIE_TRY(run_proj(b, gate_up_args(e, L, p.flags, r), p.in, r));
    QIE_TRY(run_row_proj(b, down_args(e, L, p.flags, r), p.in, r));
    return dbg_snap(b, 2 * l + 2);
}

// The layer of the multi-row forms (prefill, append, the verify step): the q/k post-projection
// writes the rows' K/V at their positions r.pos, then `attend` runs over them — qie_attention
// from position 0 (the rows are the whole context), qie_attention_extend where the rows
// continue a cached prefix (each row sees the prefix and the rows before it).  r.segs set
// (qie_prefill_ragged): the rows are segments of any lengths, each of its own sequence, and both
// steps take their ragged forms (`attend` is not consulted).
using AttentionFn = decltype(&qie_attention);
static int enqueue_layer_rows(qie_batch* b, int l, const LayerRows& r, const LayerPath& p, const qie_kv_cache& cache,
                              AttentionFn attend, void* attn_ws) {
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    const qie_layer_weights& L = p.layers[l];
    hipStream_t st = e->stream;
    QIE_TRY(run_proj(b, qkv_args(e, L, p.flags, r), p.in, r));
    if (r.segs) {
        QIE_TRY(qie_qkv_post_ragged(r.qkv, r.M, r.pos, r.segs, L.q_norm, L.k_norm, e->rope_cos, e->rope_sin, e->sh.nq,
                                    &cache, l, s.rms_eps, s.numerics, r.q, st));
        QIE_TRY(qie_attention_ragged(r.q, r.pos, r.segs, &cache, l, e->sh.nq, r.att, attn_ws, st));
    } else {
        QIE_TRY(qie_qkv_post(r.qkv, r.M, r.pos, r.rows_per_seq, L.q_norm, L.k_norm, e->rope_cos, e->rope_sin, e->sh.nq,
                             &cache, l, s.rms_eps, s.numerics, r.q, st));
        QIE_TRY(attend(r.q, r.M, r.pos, r.rows_per_seq, &cache, l, e->sh.nq, r.att, attn_ws, st));
    }
    QIE_TRY(run_row_proj(b, o_args(e, L, p.flags, r), p.in, r));
    QIE_TRY(run_proj(b, gate_up_args(e, L, p.flags, r), p.in, r));
    return run_row_proj(b, down_args(e, L, p.flags, r), p.in, r);
}

static bool is_greedy(const qie_sampling* s) { return !s || s->top_k <= 1 || !(s->temperature > 0.f); }

// tmp[r][i][j] (rank r's logit shard of row i) -> full[m0 + i][r * Vl + j]
__global__ void unshard_rows_kernel(const uint16_t* __restrict__ tmp, uint16_t* __restrict__ full, int tp, int M,
                                    int64_t Vl, int64_t V, int m0) {
    const int64_t n = (int64_t)tp * M * Vl;
    for (int64_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
        const int64_t j = k % Vl, i = (k / Vl) % M, r = k / (Vl * M);
        full[(m0 + i) * V + r * Vl + j] = tmp[k];
    }
}

// all-gather of M rows of vocab-parallel logits into hb.logits_full rows [full_row0, + M)
static int gather_rows(qie_batch* b, const HeadBufs& hb, int M) {
    qie_engine* e = b->e;
    const int64_t Vl = e->sh.vocab;
    QIE_TRY(e->comm->allgather(hb.logits, hb.gather_tmp, (int64_t)M * Vl * 2, e->stream));
    const int64_t n = (int64_t)e->sh.tp * M * Vl;
    hipLaunchKernelGGL(unshard_rows_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0,
                       e->stream, hb.gather_tmp, hb.logits_full, e->sh.tp, M, Vl, (int64_t)e->spec.vocab, hb.full_row0);
    QIE_LAUNCH_CHECK();
    return 0;
}
// ... of the batch's rows [m0, m0 + M)
static int gather_logits(qie_batch* b, int m0, int M) { return gather_rows(b, head_bufs(b->dec, m0, b->e->sh.vocab), M); }

// the persistent step's words behind its granules: [0] step epoch, [1] error word
static unsigned* pk_epoch_ptr(const qie_batch* b) {
    return (unsigned*)((unsigned long long*)b->pk_mem + persist_granule_count(b->e->spec));
}

// [final norm + lm_head] over M rows of x into hb.logits; greedy: + the fused arg-max into hb.keys
static qie_linear_args head_args(const qie_engine* e, const uint16_t* x, int64_t ldx, int M, bool greedy,
                                 const HeadBufs& hb) {
    const qie_model_spec& s = e->spec;
    const int64_t Vl = e->sh.vocab;
    qie_linear_args a = lin_args(lin_flags(e) | (e->fp8_t16_head ? QIE_LINEAR_FP8_T16 : 0));
    a.x = x; a.ldx = ldx;
    a.w[0] = e->w.lm_head; a.seg_rows[0] = Vl;
    a.M = M; a.K = s.hidden; a.N = Vl;
    a.y = hb.logits; a.ldy = Vl;
    a.epilogue = QIE_EPI_STORE;
    a.norm_w = e->w.final_norm; a.norm_eps = s.rms_eps; a.numerics = s.numerics;
    if (greedy) {
        a.argmax_keys = (uint64_t*)hb.keys;
        a.key_col0 = e->sh.vocab0;   // keys carry global vocab ids
    }
    return a;
}

// The rows of a head launch that sample under per-slot entries: row m belongs to slot
// slot0 + m * slot_stride and its input token sits at position q[m]; a verify step's rows carry
// the drafts as a tail (tail_len[m] = m).  row_slot set (a batched verify step): row m's slot and
// its tail's first word come from the device arrays row_slot / tail_off (qie_sample_rows_mapped).
struct EntryRows {
    int slot0, slot_stride;
    const int32_t *q, *tail, *tail_len;
    const int32_t *row_slot = nullptr, *tail_off = nullptr;
};
// does a slot of [m0, m0 + M) hold an entry?
static bool any_entry(const qie_batch* b, int m0, int M) {
    if (b->n_slot_set == 0) return false;
    for (int m = m0; m < m0 + M; m++)
        if (b->slot_set[m]) return true;
    return false;
}

// lm_head over M rows of x (already the residual stream), then the sampler; leaves the
// choices in hb.keys (greedy without entries) or hb.ids.  er: the rows sample through
// qie_sample_rows (smp is what rows without an entry use); null: the fused keys / qie_sample.
static int enqueue_head_rows(qie_batch* b, const uint16_t* x, int64_t ldx, int M, const qie_sampling* smp,
                             const HeadBufs& hb, const EntryRows* er = nullptr) {
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    hipStream_t st = e->stream;
    const bool greedy = !er && is_greedy(smp);
    qie_linear_args a = head_args(e, x, ldx, M, greedy, hb);
    QIE_TRY(prenorm(b, a, hb.xn));
    QIE_TRY(linear(&a, LinearExtras{}, st));
    if (greedy && use_comm(e)) QIE_TRY(e->comm->allreduce_max_u64((uint64_t*)hb.keys, M, st));
    if (!greedy) {
        const uint16_t* lg = hb.logits;
        if (use_comm(e)) {   // every rank samples the same draw from the gathered row
            QIE_TRY(gather_rows(b, hb, M));
            lg = hb.logits_full + (int64_t)hb.full_row0 * s.vocab;
        }
        if (er) {
            qie_sample_rows_args ra{};
            ra.logits = lg, ra.M = M, ra.V = s.vocab, ra.ld = s.vocab;
            ra.table = b->d_slots, ra.slot0 = er->slot0, ra.slot_stride = er->slot_stride;
            ra.fallback = smp;
            ra.hist = b->dec.hist, ra.hist_stride = b->max_ctx;
            ra.q_dev = er->q, ra.tail_dev = er->tail, ra.tail_len_dev = er->tail_len;
            ra.step_dev = hb.step, ra.out_ids = hb.ids, ra.ws = b->rows_ws;
            if (er->row_slot) QIE_TRY(qie_sample_rows_mapped(&ra, er->row_slot, er->tail_off, st));
            else QIE_TRY(qie_sample_rows(&ra, st));
        } else {
            QIE_TRY(qie_sample(lg, M, s.vocab, s.vocab, smp, hb.step, hb.ids, hb.samp_ws, st));
        }
    }
    return 0;
}

// ... over rows [m0, m0+M) of the batch, then the step finalisation of those slots
static int enqueue_head(qie_batch* b, const uint16_t* x, int64_t ldx, int m0, int M, const qie_sampling* smp) {
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    hipStream_t st = e->stream;
    // a slot's position is its pending token's: the window's last position
    const EntryRows er{m0, 1, b->dec.pos + m0, nullptr, nullptr};
    const bool entries = any_entry(b, m0, M);
    QIE_TRY(enqueue_head_rows(b, x, ldx, M, smp, head_bufs(b->dec, m0, b->e->sh.vocab), entries ? &er : nullptr));
    const bool greedy = !entries && is_greedy(smp);
    hipLaunchKernelGGL(finalize_kernel, dim3(M), dim3(256), 0, st, m0, greedy ? b->dec.keys : nullptr,
                       b->dec.ids, b->dec.ids, b->dec.pos, b->dec.step, b->dec.hist, b->max_ctx,
                       (const uint4*)e->w.embed, (uint4*)b->dec.x, (int64_t)s.hidden / 8, s.vocab, rope_cur_args(b),
                       b->pk_mem ? pk_epoch_ptr(b) : nullptr);
    QIE_LAUNCH_CHECK();
    return 0;
}

static bool pk_on(const qie_batch* b) { return b->decode_mode == 1 && b->pk_mem && !b->dbg_x; }

// the split target of the batch-1 decode attention (qie_attention_decode's rule at B = 1)
static int pk_splits_target(const qie_batch* b) { (void)b; return 32; }

static int enqueue_layers_persistent(qie_batch* b) {
    qie_engine* e = b->e;
    return persist_decode_launch(e->spec, b->d_layers, b->d_attp, b->dec.x, (unsigned long long*)b->pk_mem,
                                 pk_epoch_ptr(b), pk_epoch_ptr(b) + 1, b->dec.pos, pk_splits_target(b), b->pk_ts,
                                 e->stream);
}

static int enqueue_decode(qie_batch* b, const qie_sampling* smp) {
    if (pk_on(b)) QIE_TRY(enqueue_layers_persistent(b));
    else
        for (int l = 0; l < b->e->spec.n_layers; l++) QIE_TRY(enqueue_layer_decode(b, l));
    return enqueue_head(b, b->dec.x, b->e->spec.hidden, 0, b->B, smp);
}

// opts.prefill_fp8 (numerics flag): the prefill projections on the block-scaled fp8 MFMA
// GEMM (QIE_LINEAR_ACT_FP8) — fp8 weights in the engine's arena, every projection input
// quantised per row (qie_quantize_rows_fp8), K of each a multiple of 128 — qie_engine_create
// refuses the flag where that does not hold, so it is never dropped silently here
static bool prefill_mx(const qie_engine* e) {
    return e->fp8 && e->opts.prefill_fp8;
}

// Workspace of the attention form a prefill of n rows runs: qie_attention from position 0,
// qie_attention_extend (sized for the cache's run length, as batch_cache hands it over) for an
// append
static int64_t prefill_attn_ws_bytes(const qie_batch* b, int64_t n, bool extend) {
    const qie_model_spec& s = b->e->spec;
    if (extend) return qie_attention_extend_workspace_bytes(n, b->e->sh.nq, s.head_dim, b->max_ctx + b->run_pad);
    return qie_attention_workspace_bytes(n, b->e->sh.nq, s.head_dim, b->max_ctx);
}

// The shared dimensions of a block of `rows` rows on this rank; the caller adds the workspace
// byte counts its set carves
static RowDims row_dims(const qie_engine* e, int64_t rows) {
    const qie_model_spec& s = e->spec;
    RowDims d;
    d.rows = rows;
    d.H = s.hidden, d.QD = (int64_t)e->sh.nq * s.head_dim, d.KD = (int64_t)e->sh.nkv * s.head_dim;
    d.I = e->sh.ffn, d.Vl = e->sh.vocab, d.V = s.vocab;
    d.exchange = use_comm(e);
    return d;
}

// One allocation for what `list(carver, rows)` names: the listing runs for the size, then for
// the pointers.  `r` is written only once the allocation exists.
template <class Rows, class List>
static int alloc_rows(Rows& r, int64_t rows, List list) {
    Carver c;
    list(c, r);
    void* mem = nullptr;
    QIE_TRY(dmalloc(&mem, c.off));
    c = Carver{(char*)mem};
    list(c, r);
    r.mem = mem, r.bytes = c.off, r.rows = rows;
    return 0;
}
template <class Rows>
static void free_rows(Rows& r) {
    if (r.mem) hipFree(r.mem);
    r = Rows{};
}

// The growable blocks: the old block is freed (and nulled) BEFORE the new one is made, so the
// peak does not double and a failed allocation leaves rows == 0 and nothing dangling.  Not zeroed.
static int ensure_prefill_scratch(qie_batch* b, int64_t n, bool extend) {
    if (n > b->pf.rows) {
        free_rows(b->pf);
        const RowDims d = row_dims(b->e, n);
        QIE_TRY(alloc_rows(b->pf, n, [&](Carver& c, PrefillRows& r) { carve_prefill(c, r, d, prefill_mx(b->e)); }));
    }
    return b->pf_ws.grow((size_t)prefill_attn_ws_bytes(b, n, extend));
}

// The persistent step's error word (a bounded hand-off wait that gave up): the step's outputs
// are garbage and the call fails loudly (never a hang; k_persist.hip)
static int pk_fail(unsigned w) {
    return fail(-8, "decode: the persistent decode step gave up on a hand-off wait (error word 0x%x: a CU never "
                    "published its part within the bound); outputs of this step are invalid", w);
}
static int pk_check(qie_batch* b) {
    if (!b->pk_mem) return 0;
    unsigned w = 0;
    QIE_HIP(hipMemcpyAsync(&w, pk_epoch_ptr(b) + 1, 4, hipMemcpyDeviceToHost, b->e->stream));
    QIE_HIP(hipStreamSynchronize(b->e->stream));
    return w ? pk_fail(w) : 0;
}

// A step's results (the ids, a verify step's result words), the exchange error word (tensor
// parallel, peer backend) and the persistent step's error word come back in ONE stream-ordered
// batch with one synchronisation — not a second blocking round trip per token; a
// backend without the word keeps comm_check's own read.
static int read_back(qie_batch* b, void* dst, const void* src, size_t bytes, const char* who) {
    qie_engine* e = b->e;
    QIE_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
    const unsigned* ew = use_comm(e) ? e->comm->error_word() : nullptr;
    unsigned err = 0, pkw = 0;
    if (ew) QIE_HIP(hipMemcpyAsync(&err, ew, sizeof(err), hipMemcpyDeviceToHost, e->stream));
    if (b->pk_mem) QIE_HIP(hipMemcpyAsync(&pkw, pk_epoch_ptr(b) + 1, 4, hipMemcpyDeviceToHost, e->stream));
    QIE_HIP(hipStreamSynchronize(e->stream));
    if (pkw) return pk_fail(pkw);
    if (ew) return err ? comm_fail(who, err) : 0;
    return comm_check(e, who);
}

static int sync_ids(qie_batch* b, int32_t* next_ids) {
    return next_ids ? read_back(b, next_ids, b->dec.ids, (size_t)b->B * 4, "decode") : pk_check(b);
}

}  // namespace qie

extern "C" {

int qie_engine_create(const qie_model_spec* spec, const qie_engine_opts* opts, qie_engine** out) {
    QIE_REQUIRE(spec && out, "qie_engine_create: bad arguments");
    const qie_model_spec& s = *spec;
    QIE_REQUIRE(s.n_layers > 0 && s.hidden > 0 && s.n_heads > 0 && s.n_kv_heads > 0 && s.head_dim > 0 &&
                    s.ffn > 0 && s.vocab > 0 && s.n_heads % s.n_kv_heads == 0,
                "qie_engine_create: invalid model spec");
    QIE_REQUIRE(s.hidden % 8 == 0 && s.ffn % 8 == 0 && (s.head_dim == 64 || s.head_dim == 128),
                "qie_engine_create: hidden/ffn must be multiples of 8 and head_dim 64 or 128");
    qie_comm* comm = opts ? (qie_comm*)opts->tp_comm : nullptr;
    const int tp = comm ? comm->world : 1;
    TpShard probe;
    QIE_REQUIRE(shard_heads(s.n_heads, s.n_kv_heads, tp, 0, probe) && s.ffn % tp == 0 && (s.ffn / tp) % 8 == 0 &&
                    s.vocab % tp == 0,
                "qie_engine_create: tensor parallel %d needs n_kv_heads divisible by it (or dividing it, with at "
                "most n_heads / n_kv_heads ranks per kv head), vocab divisible by it and ffn / tp a multiple of 8 "
                "(use replicas for this model at this size)", tp);
    // prefill_fp8 is a numerics choice (every projection input quantised to e4m3): refuse it
    // where the engine could not honour it, instead of silently running bf16 activations
    // against a caller (and an oracle) that expects the fp8-activation model
    if (opts && opts->weight_fp4) {
        QIE_REQUIRE(tp == 1, "qie_engine_create: weight_fp4 with tensor parallelism is not supported (a tp_comm of "
                             "%d ranks was given)", tp);
        QIE_REQUIRE(!opts->prefill_fp8, "qie_engine_create: weight_fp4 does not combine with prefill_fp8 (block-scaled "
                                        "fp8 activations need fp8 projection weights)");
        QIE_REQUIRE(fp4_takes_spec(s, QIE_LINEAR_FP4),
                    "qie_engine_create: weight_fp4: the MXFP4 kernel does not take this model's projections: hidden "
                    "(%d), q dim (%d) and ffn (%d) must be multiples of 128 (hidden at most 8192), q and kv widths "
                    "multiples of 16", s.hidden, s.n_heads * s.head_dim, s.ffn);
    }
    if (opts && opts->prefill_fp8) {
        const int64_t qd = (int64_t)probe.nq * s.head_dim, ffl = s.ffn / tp;
        QIE_REQUIRE(opts->weight_fp8, "qie_engine_create: prefill_fp8 needs weight_fp8 (fp8 weights are the "
                                      "block-scaled MFMA's second operand)");
        QIE_REQUIRE(s.hidden % 128 == 0 && qd % 128 == 0 && ffl % 128 == 0,
                    "qie_engine_create: prefill_fp8 needs hidden (%lld), this rank's q width (%lld) and ffn / tp "
                    "(%lld) to be multiples of 128 (the fp8 MFMA's k block)",
                    (long long)s.hidden, (long long)qd, (long long)ffl);
    }
    qie_engine* e = new qie_engine();
    e->spec = s;
    if (opts) e->opts = *opts;
    if (e->opts.max_ctx <= 0) e->opts.max_ctx = 32786;   // reference CONTEXT_SIZE (iengine.cuh:19)
    e->comm = comm;
    e->sh.tp = tp;
    e->sh.rank = comm ? comm->rank : 0;
    shard_heads(s.n_heads, s.n_kv_heads, tp, e->sh.rank, e->sh);
    e->sh.ffn = s.ffn / tp;
    e->sh.vocab = s.vocab / tp;
    e->sh.vocab0 = (int64_t)e->sh.rank * e->sh.vocab;
    e->opts.tp_size = tp;
    e->opts.tp_rank = e->sh.rank;
    if (comm && !comm->graph_capturable()) e->opts.use_graph = 0;
    hipError_t he = hipSetDevice(e->opts.device);
    if (he != hipSuccess) {
        delete e;
        return fail((int)he, "hipSetDevice(%d): %s", opts ? opts->device : 0, hipGetErrorString(he));
    }
    he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he != hipSuccess) {
        delete e;
        return fail((int)he, "hipStreamCreate: %s", hipGetErrorString(he));
    }
    int rc = build_rope(e);
    if (rc) {
        qie_engine_destroy(e);
        return rc;
    }
    *out = e;
    return 0;
}

static int alloc_arena_synthetic(qie_engine* e) {
    if (e->index) qie_index_destroy(e->index);
    e->index = nullptr;
    QIE_TRY(qie_index_synthetic(&e->spec, &e->index));
    e->arena_bytes = (size_t)qie_index_total_bytes(e->index);
    if (e->arena) hipFree(e->arena);
    e->arena = nullptr;
    QIE_HIP(hipMalloc(&e->arena, e->arena_bytes));
    return 0;
}

// This rank's part of one full tensor: rows [row0, row0 + rows) x cols [col0, col0 + cols)
// of the row-major [full_rows, full_cols] tensor `src` (1-D tensors are one row).
struct ShardSlice {
    const qie_index_entry* src = nullptr;
    int64_t rows = 0, cols = 0, full_cols = 0, row0 = 0, col0 = 0;
};

static ShardSlice plan_slice(const qie_index_entry& t, const qie_model_spec& s, const TpShard& sh) {
    ShardSlice x;
    x.src = &t;
    const int64_t d0 = t.shape.empty() ? 1 : t.shape[0];
    const int64_t d1 = t.shape.size() >= 2 ? t.shape[1] : 1;
    const bool two_d = t.shape.size() >= 2;
    x.rows = two_d ? d0 : 1;
    x.cols = two_d ? d1 : d0;
    x.full_cols = x.cols;
    const int64_t hd = s.head_dim;
    const std::string& n = t.short_name;
    auto rows_part = [&](int64_t local, int64_t first) { x.rows = local; x.row0 = first; };
    auto cols_part = [&](int64_t local, int64_t first) { x.cols = local; x.col0 = first; };
    if (sh.tp == 1) return x;
    const int64_t qn = sh.nq * hd, q0 = (int64_t)sh.q0 * hd, kn = sh.nkv * hd, k0 = (int64_t)sh.kv0 * hd;
    if (n == "self_attn.q_proj.weight") rows_part(qn, q0);                              // column-parallel
    else if (n == "self_attn.k_proj.weight" || n == "self_attn.v_proj.weight") rows_part(kn, k0);
    else if (n == "self_attn.q_proj.bias") cols_part(qn, q0);
    else if (n == "self_attn.k_proj.bias" || n == "self_attn.v_proj.bias") cols_part(kn, k0);
    else if (n == "self_attn.o_proj.weight") cols_part(qn, q0);                         // row-parallel
    else if (n == "mlp.gate_proj.weight" || n == "mlp.up_proj.weight") rows_part(sh.ffn, (int64_t)sh.rank * sh.ffn);
    else if (n == "mlp.down_proj.weight") cols_part(sh.ffn, (int64_t)sh.rank * sh.ffn);
    else if (n == "logits") rows_part(sh.vocab, (int64_t)sh.rank * sh.vocab);          // vocab-parallel
    return x;
}

// Shard index: same names / roles as the full index, local shapes and arena offsets
// (256-B aligned).  A tied lm_head becomes a vocab slice of the embedding under tp > 1.
static int build_shard_index(qie_engine* e, const qie_index* full, qie_index** out, std::vector<ShardSlice>& sl) {
    qie_index* idx = new qie_index();
    sl.clear();
    int64_t off = 0;
    auto add = [&](const qie_index_entry& src, const ShardSlice& x, const char* short_name) {
        qie_index_entry le;
        le.name = src.name;
        le.short_name = short_name ? short_name : src.short_name;
        le.layer = src.layer;
        le.shape = src.shape.size() >= 2 ? std::vector<int64_t>{x.rows, x.cols} : std::vector<int64_t>{x.cols};
        le.off0 = off;
        le.off1 = off + x.rows * x.cols * 2;
        off = (le.off1 + 255) / 256 * 256;
        idx->t.push_back(le);
        sl.push_back(x);
    };
    for (const auto& t : full->t) add(t, plan_slice(t, e->spec, e->sh), nullptr);
    if (e->spec.tie_embeddings && e->sh.tp > 1) {
        const qie_index_entry* emb = index_find(full, "embed_tokens.weight", -1);
        if (!emb) {
            delete idx;
            return fail(-22, "tied lm_head: embed_tokens.weight missing from index");
        }
        qie_index_entry as_logits = *emb;
        as_logits.short_name = "logits";
        ShardSlice x = plan_slice(as_logits, e->spec, e->sh);
        x.src = emb;
        add(*emb, x, "logits");
    }
    *out = idx;
    return 0;
}

static int init_synthetic_sharded(qie_engine* e, uint64_t seed, float w_scale, float norm_scale, float bias_scale) {
    qie_index* full = nullptr;
    QIE_TRY(qie_index_synthetic(&e->spec, &full));
    std::vector<ShardSlice> sl;
    qie_index* local = nullptr;
    int rc = build_shard_index(e, full, &local, sl);
    if (!rc) {
        if (e->index) qie_index_destroy(e->index);
        e->index = local;
        e->arena_bytes = (size_t)(local->t.empty() ? 16 : local->t.back().off1);
        if (e->arena) hipFree(e->arena);
        e->arena = nullptr;
        hipError_t he = hipMalloc(&e->arena, e->arena_bytes);
        if (he != hipSuccess) rc = fail((int)he, "weight arena (%zu bytes): %s", e->arena_bytes, hipGetErrorString(he));
    }
    for (size_t i = 0; !rc && i < sl.size(); i++) {
        const qie_index_entry& le = local->t[i];
        const ShardSlice& x = sl[i];
        const std::string& sn = x.src->short_name;
        float scale = w_scale, offset = 0.f;
        if (sn.find("norm") != std::string::npos) { scale = norm_scale; offset = 1.0f; }
        else if (sn.find("bias") != std::string::npos) { scale = bias_scale; }
        rc = qie_synthetic_fill_slice((char*)e->arena + le.off0, x.rows, x.cols, x.full_cols, x.row0, x.col0,
                                      qie_tensor_id(x.src->name.c_str()), seed, scale, offset, e->stream);
    }
    qie_index_destroy(full);   // slices point into it only during the fill
    if (rc) return rc;
    QIE_HIP(hipStreamSynchronize(e->stream));
    return bind_from_index(e);
}

int qie_engine_init_synthetic(qie_engine* e, uint64_t seed, float w_scale, float norm_scale, float bias_scale) {
    QIE_REQUIRE(e, "qie_engine_init_synthetic: null engine");
    if (e->sh.tp > 1) return init_synthetic_sharded(e, seed, w_scale, norm_scale, bias_scale);
    QIE_TRY(alloc_arena_synthetic(e));
    const int n = qie_index_count(e->index);
    for (int i = 0; i < n; i++) {
        const char *name, *sn;
        int32_t layer, nd;
        int64_t o0, o1, shp[4];
        qie_index_get(e->index, i, &name, &sn, &layer, &o0, &o1, &nd, shp);
        const std::string sname(sn);
        float scale = w_scale, offset = 0.f;
        if (sname.find("norm") != std::string::npos) { scale = norm_scale; offset = 1.0f; }
        else if (sname.find("bias") != std::string::npos) { scale = bias_scale; }
        QIE_TRY(qie_synthetic_fill((char*)e->arena + o0, (o1 - o0) / 2, qie_tensor_id(name), seed, scale, offset,
                                   e->stream));
    }
    QIE_HIP(hipStreamSynchronize(e->stream));
    return bind_from_index(e);
}

// Tensor-parallel load: each rank reads only its slices of weights.bin (row slices in
// one read, column slices row by row) — 1/tp of the bytes per rank for the big tensors.
static int load_weights_sharded(qie_engine* e, const char* weights_bin, const char* meta) {
    qie_index* full = nullptr;
    QIE_TRY(qie_index_load_meta(meta, &full));
    std::vector<ShardSlice> sl;
    qie_index* local = nullptr;
    int rc = build_shard_index(e, full, &local, sl);
    if (rc) {
        qie_index_destroy(full);
        return rc;
    }
    if (e->index) qie_index_destroy(e->index);
    e->index = local;
    e->arena_bytes = (size_t)(local->t.empty() ? 16 : local->t.back().off1);
    if (e->arena) hipFree(e->arena);
    e->arena = nullptr;
    std::ifstream f(weights_bin, std::ios::binary);
    if (!f.good()) rc = fail(-2, "cannot open %s", weights_bin);
    if (!rc) {
        hipError_t he = hipMalloc(&e->arena, e->arena_bytes);
        if (he != hipSuccess) rc = fail((int)he, "weight arena: %s", hipGetErrorString(he));
    }
    std::vector<uint16_t> host;
    for (size_t i = 0; !rc && i < sl.size(); i++) {
        const ShardSlice& x = sl[i];
        host.resize((size_t)(x.rows * x.cols));
        if (x.cols == x.full_cols) {
            f.seekg(x.src->off0 + x.row0 * x.full_cols * 2);
            f.read((char*)host.data(), x.rows * x.cols * 2);
            if (!f) rc = fail(-5, "short read of %s (%s)", weights_bin, x.src->name.c_str());
        } else {
            for (int64_t r = 0; r < x.rows && !rc; r++) {
                f.seekg(x.src->off0 + ((x.row0 + r) * x.full_cols + x.col0) * 2);
                f.read((char*)(host.data() + r * x.cols), x.cols * 2);
                if (!f) rc = fail(-5, "short read of %s (%s)", weights_bin, x.src->name.c_str());
            }
        }
        if (!rc) {
            // stream-ordered before the engine's kernels (its stream is non-blocking: a copy on the
            // legacy null stream is not), complete before the staging vector is refilled
            hipError_t he = hipMemcpyAsync((char*)e->arena + local->t[i].off0, host.data(),
                                           (size_t)(x.rows * x.cols * 2), hipMemcpyHostToDevice, e->stream);
            if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
            if (he != hipSuccess) rc = fail((int)he, "H2D: %s", hipGetErrorString(he));
        }
    }
    qie_index_destroy(full);
    if (rc) return rc;
    return bind_from_index(e);
}

int qie_engine_load_weights_bin(qie_engine* e, const char* weights_bin, const char* meta, int64_t chunk_bytes) {
    QIE_REQUIRE(e && weights_bin && meta, "qie_engine_load_weights_bin: bad arguments");
    if (e->sh.tp > 1) return load_weights_sharded(e, weights_bin, meta);
    if (e->index) qie_index_destroy(e->index);
    e->index = nullptr;
    QIE_TRY(qie_index_load_meta(meta, &e->index));
    std::ifstream f(weights_bin, std::ios::binary | std::ios::ate);
    QIE_REQUIRE(f.good(), "cannot open %s", weights_bin);
    const int64_t file_bytes = (int64_t)f.tellg();
    f.seekg(0);
    const int64_t need = qie_index_total_bytes(e->index);
    QIE_REQUIRE(file_bytes >= need, "%s is %lld bytes, index needs %lld", weights_bin, (long long)file_bytes,
                (long long)need);
    e->arena_bytes = (size_t)need;
    if (e->arena) hipFree(e->arena);
    e->arena = nullptr;
    QIE_HIP(hipMalloc(&e->arena, e->arena_bytes));
    if (chunk_bytes <= 0) chunk_bytes = (int64_t)1 << 28;
    // Two pinned staging buffers: file read of chunk i+1 overlaps H2D of chunk i.
    void* stage[2] = {nullptr, nullptr};
    hipEvent_t done[2];
    QIE_HIP(hipHostMalloc(&stage[0], chunk_bytes, hipHostMallocDefault));
    QIE_HIP(hipHostMalloc(&stage[1], chunk_bytes, hipHostMallocDefault));
    QIE_HIP(hipEventCreate(&done[0]));
    QIE_HIP(hipEventCreate(&done[1]));
    int64_t off = 0;
    int which = 0;
    bool pending[2] = {false, false};
    int rc = 0;
    while (off < need) {
        const int64_t n = std::min<int64_t>(chunk_bytes, need - off);
        if (pending[which]) {
            hipEventSynchronize(done[which]);
            pending[which] = false;
        }
        f.read((char*)stage[which], n);
        if (f.gcount() != n) { rc = fail(-5, "short read of %s at %lld", weights_bin, (long long)off); break; }
        hipError_t he = hipMemcpyAsync((char*)e->arena + off, stage[which], n, hipMemcpyHostToDevice, e->stream);
        if (he != hipSuccess) { rc = fail((int)he, "H2D: %s", hipGetErrorString(he)); break; }
        hipEventRecord(done[which], e->stream);
        pending[which] = true;
        off += n;
        which ^= 1;
    }
    hipStreamSynchronize(e->stream);
    hipEventDestroy(done[0]);
    hipEventDestroy(done[1]);
    hipHostFree(stage[0]);
    hipHostFree(stage[1]);
    if (rc) return rc;
    return bind_from_index(e);
}

int qie_engine_set_weights(qie_engine* e, const qie_model_weights* w) {
    QIE_REQUIRE(e && w && w->layers && w->n_layers == e->spec.n_layers && w->embed && w->final_norm && w->lm_head,
                "qie_engine_set_weights: bad arguments");
    e->layers.assign(w->layers, w->layers + w->n_layers);
    for (int l = 0; l < w->n_layers; l++) {
        const qie_layer_weights& L = e->layers[l];
        QIE_REQUIRE(L.attn_norm && L.wq && L.wk && L.wv && L.wo && L.ffn_norm && L.w_gate && L.w_up && L.w_down,
                    "qie_engine_set_weights: layer %d incomplete", l);
        QIE_REQUIRE(!e->spec.qkv_bias || (L.bq && L.bk && L.bv), "layer %d: q/k/v bias missing", l);
        QIE_REQUIRE(!e->spec.qk_norm || (L.q_norm && L.k_norm), "layer %d: q/k norm missing", l);
        const void* ps[] = {L.attn_norm, L.wq, L.wk, L.wv, L.wo, L.ffn_norm, L.w_gate, L.w_up, L.w_down};
        for (const void* p : ps) QIE_TRY(check_align(p, "weight", l));
    }
    e->w = *w;
    e->w.layers = e->layers.data();
    e->have_weights = true;
    return quantize_weights(e, false);
}

int qie_engine_weights(const qie_engine* e, qie_model_weights* out, const qie_layer_weights** layers) {
    QIE_REQUIRE(e && e->have_weights, "qie_engine_weights: no weights");
    if (out) *out = e->w;
    if (layers) *layers = e->layers.data();
    return 0;
}

int qie_engine_spec(const qie_engine* e, qie_model_spec* out) {
    QIE_REQUIRE(e && out, "qie_engine_spec: bad arguments");
    *out = e->spec;
    return 0;
}

void* qie_engine_stream(qie_engine* e) { return e ? (void*)e->stream : nullptr; }

int qie_engine_sync(qie_engine* e) {
    QIE_REQUIRE(e, "qie_engine_sync: null");
    QIE_HIP(hipStreamSynchronize(e->stream));
    return comm_check(e, "qie_engine_sync");
}

void qie_engine_destroy(qie_engine* e) {
    if (!e) return;
    if (e->stream) hipStreamSynchronize(e->stream);
    if (e->arena) hipFree(e->arena);
    if (e->fp8_arena) hipFree(e->fp8_arena);
    if (e->fp4_arena) hipFree(e->fp4_arena);
    if (e->pf_arena) hipFree(e->pf_arena);
    if (e->rope_cos) hipFree(e->rope_cos);
    if (e->rope_sin) hipFree(e->rope_sin);
    if (e->index) qie_index_destroy(e->index);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;
}

// ------------------------------------------------------------ page pool
// Host-side allocator of the paged batch (page_pool.hpp) and the entry points that
// deal in pages and slots.  Decisions are deterministic, so the tensor-parallel ranks (each
// holding its own heads' pages) stay in step.

// uploads the host table (ordered after everything already on the stream)
static int flush_table(qie_batch* b) {
    if (!b->d_table || !b->table_dirty) return 0;
    // on the engine stream (non-blocking: a legacy-null-stream copy is not ordered before its
    // kernels), complete before the host table may change again
    QIE_HIP(hipMemcpyAsync(b->d_table, b->pool.table.data(), b->pool.table.size() * 4, hipMemcpyHostToDevice, b->e->stream));
    QIE_HIP(hipStreamSynchronize(b->e->stream));
    b->table_dirty = false;
    return 0;
}

// The reservation of one engine call: every call that writes KV rows names them
// as spans — positions [lo, hi] of a slot; hi < lo: only growth to lo tokens; restart: the slot
// begins a new sequence — plans them, compares need with free under its own error line, and
// commits.  This pair is the only place where a writer touches the pool.
struct KvWrites {
    PagePool::Reservation r;   // r.need: growth plus a private copy of every shared page of the spans
    int64_t free = 0;
    bool fits() const { return r.need <= free; }
};

// Changes nothing.  A contiguous batch has no pool: nothing is needed, and commit returns at once.
static int plan_kv_writes(const qie_batch* b, const PagePool::Span* spans, int n, KvWrites& w) {
    w = KvWrites{};
    if (!b->d_table) return 0;
    QIE_REQUIRE(n <= kMaxBatchSlots, "KV pages: %d spans in one call", n);
    for (int i = 0; i < n; i++) {
        const int64_t ntok = spans[i].hi >= spans[i].lo ? spans[i].hi + 1 : spans[i].lo;
        QIE_REQUIRE(b->pool.pages_for(ntok) <= b->max_pages, "KV pages: %lld tokens exceed max_ctx %d",
                    (long long)ntok, b->max_ctx);
    }
    w.r = b->pool.plan_reserve(spans, n);
    w.free = b->pool.free_count();
    return 0;
}

// Applies a plan that fits: restart slots let go of their pages, shared pages of the spans become
// private ones, every slot grows, and for each replaced page with rows below lo those rows are
// copied from the page the slot shared — staged in table row B, so that qie_kv_copy reads it
// through the one table — into its replacement.  The other holders' pages are not touched.
static int commit_kv_writes(qie_batch* b, const KvWrites& w) {
    if (!b->d_table) return 0;
    bool changes = w.r.need != 0;
    for (int i = 0; i < w.r.n; i++) changes |= w.r.spans[i].restart;
    if (changes) {
        PagePool::CopyJob jobs[kMaxBatchSlots];
        const int n_jobs = b->pool.commit(w.r, jobs);
        b->table_dirty = true;
        const qie_kv_cache c = batch_cache(b, 0);
        for (int j = 0; j < n_jobs; j++) {
            b->pool.row(b->B)[jobs[j].index] = jobs[j].old_page;
            QIE_TRY(flush_table(b));
            const int rc = qie_kv_copy(&c, b->B, &c, jobs[j].slot, jobs[j].index * b->page_tokens, jobs[j].rows,
                                       b->e->stream);
            b->pool.row(b->B)[jobs[j].index] = 0;
            b->table_dirty = true;
            QIE_TRY(rc);
        }
    }
    return flush_table(b);
}

// Slot dst becomes a live sequence at position n with current token tok and step counter step_v:
// its next input row, RoPE row and history[n] as set_state_kernel sets them; synchronises.  The
// one tail of qie_batch_set_position, qie_batch_fork and qie_batch_prefix_load.
static int start_slot(qie_batch* b, int dst, int n, int step_v, int tok) {
    QIE_TRY(set_slot_state(b, dst, n, step_v, tok, 1));
    QIE_HIP(hipStreamSynchronize(b->e->stream));
    b->idle[dst] = 0;
    b->h_pos[dst] = n;
    return 0;
}

int qie_batch_release(qie_batch* b, int32_t seq) {
    QIE_REQUIRE(b && seq >= 0 && seq < b->B, "qie_batch_release: bad arguments");
    if (b->d_table) {   // the pages no other holder references return to the free list
        b->pool.release(seq);
        b->table_dirty = true;
    }
    b->idle[seq] = 1;
    QIE_TRY(flush_table(b));
    QIE_TRY(set_slot_state(b, seq, 0, 0, 0, 1));
    QIE_HIP(hipStreamSynchronize(b->e->stream));
    b->h_pos[seq] = 0;
    return 0;
}

int qie_batch_page_stats(qie_batch* b, int32_t* free_pages, int32_t* pages_per_seq, int32_t* page_tokens) {
    QIE_REQUIRE(b, "qie_batch_page_stats: null batch");
    if (free_pages) *free_pages = (int32_t)b->pool.free_count();
    if (pages_per_seq)
        for (int m = 0; m < b->B; m++) pages_per_seq[m] = b->d_table ? b->pool.held[m] : 0;
    if (page_tokens) *page_tokens = b->page_tokens;
    return 0;
}

int qie_batch_block_table(qie_batch* b, int32_t seq, int32_t* host_pages, int32_t n) {
    QIE_REQUIRE(b && b->d_table && host_pages && seq >= 0 && seq < b->B && n >= 0 && n <= b->max_pages,
                "qie_batch_block_table: bad arguments (paged batch, n <= max_pages)");
    QIE_HIP(hipStreamSynchronize(b->e->stream));
    QIE_HIP(d2h(b->e, host_pages, b->d_table + (int64_t)seq * b->max_pages, (size_t)n * 4));
    return 0;
}

int qie_batch_reserve(qie_batch* b, int32_t seq, int32_t n_tokens) {
    QIE_REQUIRE(b && seq >= 0 && seq < b->B && n_tokens >= 0, "qie_batch_reserve: bad arguments");
    QIE_REQUIRE(n_tokens <= b->max_ctx, "qie_batch_reserve: %d tokens exceed max_ctx %d", n_tokens, b->max_ctx);
    // a grow-only span: the raw tier ignores sharing on purpose
    const PagePool::Span span{seq, n_tokens, (int64_t)n_tokens - 1, false};
    KvWrites kv;
    QIE_TRY(plan_kv_writes(b, &span, 1, kv));
    QIE_REQUIRE(kv.fits(), "KV pages: sequence %d needs %lld more pages, %lld free", seq, (long long)kv.r.need,
                (long long)kv.free);
    QIE_TRY(commit_kv_writes(b, kv));
    b->idle[seq] = 0;
    return 0;
}

int qie_batch_set_position(qie_batch* b, int32_t seq, int32_t pos, int32_t token) {
    QIE_REQUIRE(b && seq >= 0 && seq < b->B && pos >= 0 && pos + 1 < b->max_ctx && token >= 0 &&
                    token < b->e->spec.vocab,
                "qie_batch_set_position: bad arguments");
    // a rewind into a page another holder shares: this slot gets a private copy of it first
    const PagePool::Span span{seq, pos, pos, false};
    KvWrites kv;
    QIE_TRY(plan_kv_writes(b, &span, 1, kv));
    if (!kv.fits() && kv.r.plans[0].n_private)
        return fail(-28, "qie_batch_set_position: KV pool exhausted (position %d lies in a shared page: %lld pages "
                         "needed, %lld free)", pos, (long long)kv.r.need, (long long)kv.free);
    QIE_REQUIRE(kv.fits(), "KV pages: sequence %d needs %lld more pages, %lld free", seq, (long long)kv.r.need,
                (long long)kv.free);
    QIE_TRY(commit_kv_writes(b, kv));
    return start_slot(b, seq, pos, pos, token);
}

// --- forks and prefix handles: they share pages (a fork draws at most its tail page, after its
// own check) and write no rows, so they use the pool directly

// ------------------------------------------------------------ per-slot sampling
static qie_slot_sampling no_entry() {
    qie_slot_sampling z{};
    z.n_bias = -1;
    z.repetition_penalty = 1.f;
    return z;
}

// The device table and the sampler's workspace, at the first set: fixed for the batch's lifetime
static int ensure_slot_table(qie_batch* b) {
    if (b->d_slots) return 0;
    qie_engine* e = b->e;
    const size_t tb = (size_t)b->B * sizeof(qie_slot_sampling);
    void *tab = nullptr, *ws = nullptr;
    if (dmalloc(&tab, tb + kVerifyMaxRows * 4) ||
        dmalloc(&ws, (size_t)qie_sample_rows_workspace_bytes(std::max(b->B, kVerifyMaxRows), e->spec.vocab))) {
        hipFree(tab);
        return fail(-2, "qie_batch_set_slot_sampling: device allocation failed: %s", qie_last_error());
    }
    std::vector<qie_slot_sampling> none(b->B, no_entry());
    int32_t iota[kVerifyMaxRows];
    for (int i = 0; i < kVerifyMaxRows; i++) iota[i] = i;
    hipError_t he = hipMemcpyAsync(tab, none.data(), tb, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync((char*)tab + tb, iota, sizeof(iota), hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);   // the host sources go out of scope
    if (he != hipSuccess) {
        hipFree(tab);
        hipFree(ws);
        return fail((int)he, "qie_batch_set_slot_sampling: table init: %s", hipGetErrorString(he));
    }
    b->d_slots = (qie_slot_sampling*)tab;
    b->d_tail_len = (int32_t*)((char*)tab + tb);
    b->rows_ws = ws;
    return 0;
}

// Slot seq's entry := *p (null: none), host copy and device table; the copy is ordered on the
// engine's stream behind the steps already enqueued, outside any graph.  Already validated.
static int write_slot_entry(qie_batch* b, int seq, const qie_slot_sampling* p) {
    if (!p && !b->d_slots) return 0;
    QIE_TRY(ensure_slot_table(b));
    const qie_slot_sampling v = p ? *p : no_entry();
    QIE_HIP(hipMemcpyAsync(b->d_slots + seq, &v, sizeof(v), hipMemcpyHostToDevice, b->e->stream));
    QIE_HIP(hipStreamSynchronize(b->e->stream));   // `v` goes out of scope
    b->n_slot_set += (p ? 1 : 0) - (b->slot_set[seq] ? 1 : 0);
    b->slot_set[seq] = p ? 1 : 0;
    b->slot_h[seq] = p ? *p : qie_slot_sampling{};
    return 0;
}

int qie_batch_set_slot_sampling(qie_batch* b, int32_t seq, const qie_slot_sampling* p) {
    QIE_REQUIRE(b && seq >= 0 && seq < b->B, "qie_batch_set_slot_sampling: bad arguments");
    if (p) {
        const int64_t V = b->e->spec.vocab;
        QIE_REQUIRE(p->n_bias >= 0 && p->n_bias <= QIE_SLOT_BIAS_MAX, "qie_batch_set_slot_sampling: n_bias %d outside [0, %d]",
                    p->n_bias, QIE_SLOT_BIAS_MAX);
        for (int i = 0; i < p->n_bias; i++) {
            QIE_REQUIRE(p->bias_ids[i] >= 0 && p->bias_ids[i] < V, "qie_batch_set_slot_sampling: bias id %d out of range",
                        p->bias_ids[i]);
            for (int j = 0; j < i; j++)
                QIE_REQUIRE(p->bias_ids[j] != p->bias_ids[i], "qie_batch_set_slot_sampling: bias id %d listed twice",
                            p->bias_ids[i]);
            QIE_REQUIRE(p->bias[i] == p->bias[i] && p->bias[i] != INFINITY,
                        "qie_batch_set_slot_sampling: the bias of id %d is NaN or +inf", p->bias_ids[i]);
        }
        QIE_REQUIRE(std::isfinite(p->temperature) && std::isfinite(p->repetition_penalty) &&
                        std::isfinite(p->presence_penalty) && std::isfinite(p->frequency_penalty),
                    "qie_batch_set_slot_sampling: temperature and penalties must be finite");
        QIE_REQUIRE(p->repetition_penalty > 0.f, "qie_batch_set_slot_sampling: repetition_penalty must be > 0 (1 = off)");
        QIE_REQUIRE(p->min_p >= 0.f && p->min_p <= 1.f, "qie_batch_set_slot_sampling: min_p outside [0, 1]");
        QIE_REQUIRE(p->penalty_start >= 0 && p->penalty_last_n >= 0,
                    "qie_batch_set_slot_sampling: penalty_start and penalty_last_n must be >= 0");
    }
    return write_slot_entry(b, seq, p);
}

int qie_batch_slot_sampling(const qie_batch* b, int32_t seq, qie_slot_sampling* out, int32_t* is_set) {
    QIE_REQUIRE(b && seq >= 0 && seq < b->B && (out || is_set), "qie_batch_slot_sampling: bad arguments");
    if (out) *out = b->slot_h[seq];
    if (is_set) *is_set = b->slot_set[seq];
    return 0;
}

int qie_batch_fork(qie_batch* b, int32_t src, int32_t dst, int32_t n_tokens, int32_t step_offset) {
    QIE_REQUIRE(b && src >= 0 && src < b->B && dst >= 0 && dst < b->B && src != dst,
                "qie_batch_fork: bad arguments (two different slots of the batch)");
    QIE_REQUIRE(!b->idle[src], "qie_batch_fork: slot %d holds no live sequence", src);
    const int p = b->h_pos[src], n = n_tokens;
    QIE_REQUIRE(n >= 1 && n <= p, "qie_batch_fork: n_tokens %d outside [1, %d] (the source's position)", n, p);
    if (b->d_table && !b->pool.fork_fits(dst, n))
        return fail(-28, "qie_batch_fork: KV pool exhausted (no page for the %d rows past the last full page; "
                         "%lld free)", n % b->page_tokens, (long long)b->pool.free_count());
    // nothing can fail for lack of pages from here on
    qie_engine* e = b->e;
    hipStream_t st = e->stream;
    int32_t tok_step[2] = {0, 0};   // the source's history[n] and its step counter
    QIE_HIP(hipMemcpyAsync(&tok_step[0], b->dec.hist + (int64_t)src * b->max_ctx + n, 4, hipMemcpyDeviceToHost, st));
    QIE_HIP(hipMemcpyAsync(&tok_step[1], b->dec.step + src, 4, hipMemcpyDeviceToHost, st));
    QIE_HIP(hipStreamSynchronize(st));
    const int tok = tok_step[0];
    // every writer of the history stores ids in [0, vocab): anything else means the history is
    // corrupt, and a fork would only copy the damage — fail while nothing has changed
    if (tok < 0 || tok >= e->spec.vocab)
        return fail(-5, "qie_batch_fork: history[%d] of slot %d holds %d, not a token id", n, src, tok);
    const qie_kv_cache c = batch_cache(b, 0);
    if (b->d_table) {   // full pages shared, the partial last page copied into a page of dst's own
        b->pool.fork(src, dst, n);
        b->table_dirty = true;
        QIE_TRY(flush_table(b));
        const int tail = n % b->page_tokens;
        QIE_TRY(qie_kv_copy(&c, src, &c, dst, n - tail, tail, st));
    } else {
        QIE_TRY(qie_kv_copy(&c, src, &c, dst, 0, n, st));
    }
    QIE_HIP(hipMemcpyAsync(b->dec.hist + (int64_t)dst * b->max_ctx, b->dec.hist + (int64_t)src * b->max_ctx,
                           (size_t)(n + 1) * 4, hipMemcpyDeviceToDevice, st));
    if (n == p)   // the pending token's logits: row dst of qie_batch_logits equals row src
        QIE_HIP(hipMemcpyAsync(b->dec.logits + (int64_t)dst * e->sh.vocab, b->dec.logits + (int64_t)src * e->sh.vocab,
                               (size_t)e->sh.vocab * 2, hipMemcpyDeviceToDevice, st));
    QIE_TRY(start_slot(b, dst, n, tok_step[1] + step_offset, tok));
    // dst samples as src does: src's entry, or none
    if (b->slot_set[src] || b->slot_set[dst]) QIE_TRY(write_slot_entry(b, dst, b->slot_set[src] ? &b->slot_h[src] : nullptr));
    return 0;
}

int qie_batch_page_refs(qie_batch* b, int32_t* host_refs, int32_t n) {
    QIE_REQUIRE(b && b->d_table && host_refs && n >= 0 && n <= b->n_pages,
                "qie_batch_page_refs: bad arguments (paged batch, n <= its pages)");
    for (int i = 0; i < n; i++) host_refs[i] = b->pool.refs[i];
    return 0;
}

int qie_batch_prefix_save(qie_batch* b, int32_t seq, int32_t n_tokens, qie_kv_prefix** out) {
    QIE_REQUIRE(b && out && seq >= 0 && seq < b->B, "qie_batch_prefix_save: bad arguments");
    QIE_REQUIRE(b->d_table, "qie_batch_prefix_save: prefix handles need a paged batch");
    QIE_REQUIRE(!b->idle[seq], "qie_batch_prefix_save: slot %d holds no live sequence", seq);
    QIE_REQUIRE(n_tokens > 0 && n_tokens % b->page_tokens == 0 && n_tokens <= b->h_pos[seq],
                "qie_batch_prefix_save: n_tokens %d must be a positive multiple of %d and at most the position %d",
                n_tokens, b->page_tokens, b->h_pos[seq]);
    qie_kv_prefix* p = new qie_kv_prefix();
    p->owner = b;
    p->ids.resize(n_tokens);
    const hipError_t he = d2h(b->e, p->ids.data(), b->dec.hist + (int64_t)seq * b->max_ctx, (size_t)n_tokens * 4);
    if (he != hipSuccess) {
        delete p;
        return fail((int)he, "qie_batch_prefix_save: reading the history: %s", hipGetErrorString(he));
    }
    for (int i = 0; i < n_tokens / b->page_tokens; i++) {
        p->pages.push_back(b->pool.row(seq)[i]);
        b->pool.share(p->pages.back());
    }
    b->prefixes.push_back(p);
    *out = p;
    return 0;
}

int qie_batch_prefix_load(qie_batch* b, const qie_kv_prefix* p, int32_t dst, int32_t n_tokens, int32_t token) {
    QIE_REQUIRE(b && p && dst >= 0 && dst < b->B && token >= 0 && token < b->e->spec.vocab,
                "qie_batch_prefix_load: bad arguments");
    QIE_REQUIRE(b->d_table && p->owner == b, "qie_batch_prefix_load: the handle belongs to another batch");
    QIE_REQUIRE(n_tokens > 0 && n_tokens % b->page_tokens == 0 && n_tokens <= (int)p->ids.size() &&
                    n_tokens + 1 < b->max_ctx,
                "qie_batch_prefix_load: n_tokens %d must be a positive multiple of %d, at most the handle's %zu and "
                "below max_ctx", n_tokens, b->page_tokens, p->ids.size());
    // shares pages only: nothing is taken from the free list, so the call cannot run out
    b->pool.release(dst);
    for (int i = 0; i < n_tokens / b->page_tokens; i++) b->pool.push_shared(dst, p->pages[i]);
    b->table_dirty = true;
    QIE_TRY(flush_table(b));
    QIE_HIP(hipMemcpyAsync(b->dec.hist + (int64_t)dst * b->max_ctx, p->ids.data(), (size_t)n_tokens * 4,
                           hipMemcpyHostToDevice, b->e->stream));
    return start_slot(b, dst, n_tokens, n_tokens, token);
}

int qie_batch_prefix_tokens(const qie_kv_prefix* p, int32_t* host_ids, int32_t n) {
    QIE_REQUIRE(p, "qie_batch_prefix_tokens: null handle");
    if (!host_ids) return (int)p->ids.size();
    QIE_REQUIRE(n >= 0 && n <= (int)p->ids.size(), "qie_batch_prefix_tokens: n %d exceeds the handle's %zu ids", n,
                p->ids.size());
    std::memcpy(host_ids, p->ids.data(), (size_t)n * 4);
    return 0;
}

int qie_batch_prefix_drop(qie_batch* b, qie_kv_prefix* p) {
    QIE_REQUIRE(b && p && p->owner == b, "qie_batch_prefix_drop: bad arguments");
    for (size_t i = 0; i < b->prefixes.size(); i++)
        if (b->prefixes[i] == p) {
            for (int32_t g : p->pages) b->pool.drop(g);
            b->prefixes.erase(b->prefixes.begin() + i);
            delete p;
            return 0;
        }
    return fail(-22, "qie_batch_prefix_drop: not an open handle of this batch");
}

static int batch_create(qie_engine* e, int32_t batch, int32_t max_ctx, int32_t page_tokens, int32_t n_pages,
                        qie_batch** out) {
    QIE_REQUIRE(e && out && batch > 0 && batch <= kMaxBatchSlots && max_ctx > 1,
                "qie_batch_create: bad arguments (B <= %d)", kMaxBatchSlots);
    QIE_REQUIRE(e->have_weights, "qie_batch_create: engine has no weights");
    QIE_REQUIRE(max_ctx <= e->rope_rows, "qie_batch_create: max_ctx %d > engine max_ctx %d", max_ctx, e->rope_rows);
    const qie_model_spec& s = e->spec;
    qie_batch* b = new qie_batch();
    b->e = e;
    b->B = batch;
    b->max_ctx = max_ctx;
    const TpShard& sh = e->sh;
    const int64_t hd = s.head_dim;
    int64_t n_runs = batch;   // sequences (contiguous) or pages (paged) in the K and V pools
    if (page_tokens > 0) {
        b->page_tokens = page_tokens;
        b->max_pages = (max_ctx + page_tokens - 1) / page_tokens;
        b->n_pages = n_pages > 0 ? n_pages : batch * b->max_pages + 1;
        b->seq_stride = (int64_t)s.n_layers * sh.nkv * page_tokens * hd;   // elements per page
        n_runs = b->n_pages;
        b->pool.init(batch + 1, b->max_pages, page_tokens, b->n_pages);   // page 1 handed out first; row B: staging
        b->table_dirty = true;
    } else {
        b->run_pad = dev_env("QIE_KV_RUN_PAD", 0);   // dev A/B: tokens of padding per (layer, head) run
        b->seq_stride = (int64_t)s.n_layers * sh.nkv * (max_ctx + b->run_pad) * hd;   // this rank's kv heads only
    }
    // Slots start idle: a slot runs as a live sequence only after a prefill or
    // set_position, so unused slots never take pool pages (they run on scratch page 0)
    // and are rewound before they would pass max_ctx (prepare_steps).
    b->idle.assign(batch, 1);
    b->h_pos.assign(batch, 0);
    b->slot_h.assign(batch, qie_slot_sampling{});
    b->slot_set.assign(batch, 0);
    // the KV pools, the block table, and the slots' rows: one block, zero but for the RoPE rows'
    // tags (-1: no position).  Never reallocated: the decode graph and the persistent step's
    // attention table hold pointers into it.
    auto make = [&]() -> int {
        const size_t pool = (size_t)n_runs * b->seq_stride * 2;
        QIE_TRY(dmalloc((void**)&b->kc, pool));
        QIE_TRY(dmalloc((void**)&b->vc, pool));
        if (page_tokens > 0) QIE_TRY(dmalloc((void**)&b->d_table, b->pool.table.size() * 4));
        RowDims d = row_dims(e, batch);
        d.samp_ws_bytes = qie_sample_workspace_bytes(batch, s.vocab);
        const int64_t rc_floats = rope_cur_stride((int)hd);
        const int64_t dec_ws = qie_attention_decode_workspace_bytes(batch, sh.nq, sh.nkv, s.head_dim, max_ctx);
        QIE_TRY(alloc_rows(b->dec, batch,
                           [&](Carver& c, DecodeRows& r) { carve_decode(c, r, d, max_ctx, rc_floats, dec_ws); }));
        QIE_HIP(hipMemsetAsync(b->kc, 0, pool, e->stream));
        QIE_HIP(hipMemsetAsync(b->vc, 0, pool, e->stream));
        QIE_HIP(hipMemsetAsync(b->dec.mem, 0, b->dec.bytes, e->stream));
        QIE_HIP(hipMemsetAsync(b->dec.rope_cur, 0xff, (size_t)batch * rc_floats * 4, e->stream));
        QIE_HIP(hipStreamSynchronize(e->stream));
        QIE_TRY(flush_table(b));
        // the fp8 batched-decode split-K workspace of this stream, before any graph capture
        if (e->fp8 && (batch >= 2 || e->fp8_t16)) QIE_TRY(dec8_reserve(e->stream));
        if (e->fp4) QIE_TRY(dec4_reserve(e->stream));   // (the MXFP4 kernel has no other kernel to decline to)
        return 0;
    };
    if (const int rc = make()) {
        qie_batch_destroy(b);
        return rc;
    }
    *out = b;
    return 0;
}

int qie_batch_create(qie_engine* e, int32_t batch, int32_t max_ctx, qie_batch** out) {
    return batch_create(e, batch, max_ctx, 0, 0, out);
}

int qie_batch_create_paged(qie_engine* e, int32_t batch, int32_t max_ctx, int32_t page_tokens, int32_t n_pages,
                           qie_batch** out) {
    if (page_tokens == 0) page_tokens = 128;
    QIE_REQUIRE(page_tokens >= 128 && (page_tokens & (page_tokens - 1)) == 0,
                "qie_batch_create_paged: page_tokens %d must be a power of two >= 128", page_tokens);
    QIE_REQUIRE(n_pages >= 0, "qie_batch_create_paged: bad n_pages");
    QIE_REQUIRE(n_pages == 0 || n_pages >= 2, "qie_batch_create_paged: need the scratch page and one more");
    return batch_create(e, batch, max_ctx, page_tokens, n_pages, out);
}

void qie_batch_destroy(qie_batch* b) {
    if (!b) return;
    if (b->e && b->e->stream) hipStreamSynchronize(b->e->stream);
    if (b->gexec) hipGraphExecDestroy(b->gexec);
    for (auto& g : b->v_graphs) hipGraphExecDestroy(g.exec);
    free_rows(b->dec);
    free_rows(b->pf);
    free_rows(b->v);
    free_rows(b->sc);
    for (void* p : {(void*)b->kc, (void*)b->vc, (void*)b->d_table, b->pk_mem, (void*)b->d_layers, b->d_attp,
                    (void*)b->pk_ts, (void*)b->d_slots, b->rows_ws, (void*)b->vb_aux})
        if (p) hipFree(p);
    // (the DevBlock workspaces free themselves)
    for (qie_kv_prefix* p : b->prefixes) delete p;   // handles still open: their pages go with the pool
    delete b;
}

// ------------------------------------------------------------ scoring
struct ScoreReq {
    const int32_t* targets;   // host [n], each in [0, V) or -1
    int32_t flags;            // QIE_SCORE_*
    float* logprobs;          // host [n]
    int32_t* greedy_ids;      // host [n] or null
};

// The fused head (qie_score_rows) reads a bf16 lm_head of the whole vocabulary
static bool score_fused(const qie_engine* e, int flags) {
    return !(flags & QIE_SCORE_UNFUSED) && !e->fp8 && !use_comm(e) && e->sh.tp == 1 && e->spec.hidden % 64 == 0 &&
           e->spec.hidden >= 256;
}

static int ensure_verify_bufs(qie_batch* b);

static int ensure_score_scratch(qie_batch* b, int64_t n, bool fused) {
    if (n > b->sc.rows) {
        free_rows(b->sc);
        QIE_TRY(alloc_rows(b->sc, n, [&](Carver& c, ScoreRows& r) { carve_score(c, r, n); }));
    }
    return fused ? b->sc_ws.grow((size_t)qie_score_rows_workspace_bytes(n, b->e->spec.vocab)) : 0;
}

// The scoring head over the n rows of b->pf.x a prefill of slot `seq` has just run (after its own
// last-row head, which is left as it is).  Fused: final norm of all rows into pf.xn (free after
// the layer loop), then qie_score_rows.  General (fp8 heads, the exchange path, QIE_SCORE_UNFUSED):
// rows [0, n - 1) in pieces of <= kVerifyMaxRows through the head launch of decode and qie_verify
// into the verify step's logit rows, qie_logprob_rows on each piece; row n - 1 from the batch's
// own logit row, which the prefill's head has just written.
static int enqueue_score(qie_batch* b, int seq, int n, const ScoreReq& rq) {
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    hipStream_t st = e->stream;
    const int64_t H = s.hidden, V = s.vocab;
    QIE_HIP(hipMemcpyAsync(b->sc.tgt, rq.targets, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (score_fused(e, rq.flags)) {
        QIE_TRY(qie_rmsnorm(b->pf.x, e->w.final_norm, b->pf.xn, n, H, s.rms_eps, s.numerics, st));
        return qie_score_rows(b->pf.xn, H, e->w.lm_head, n, H, V, b->sc.tgt, b->sc.lp, b->sc.ids, b->sc_ws.p, st);
    }
    const HeadBufs hb = head_bufs(b->v, 0, b->e->sh.vocab);
    for (int r0 = 0; r0 < n - 1; r0 += kVerifyMaxRows) {
        const int M = std::min(kVerifyMaxRows, n - 1 - r0);
        qie_linear_args a = head_args(e, b->pf.x + (int64_t)r0 * H, H, M, false, hb);
        QIE_TRY(prenorm(b, a, hb.xn));
        QIE_TRY(linear(&a, LinearExtras{}, st));
        const uint16_t* lg = hb.logits;
        if (use_comm(e)) {
            QIE_TRY(gather_rows(b, hb, M));
            lg = hb.logits_full;
        }
        QIE_TRY(qie_logprob_rows(lg, M, V, V, b->sc.tgt + r0, b->sc.lp + r0, b->sc.ids + r0, st));
    }
    b->v_rows = 0;   // the verify step's logit rows no longer hold a qie_verify's
    const uint16_t* last = b->dec.logits + (int64_t)seq * e->sh.vocab;
    if (use_comm(e)) {
        QIE_TRY(gather_logits(b, seq, 1));
        last = b->dec.logits_full + (int64_t)seq * V;
    }
    return qie_logprob_rows(last, 1, V, V, b->sc.tgt + (n - 1), b->sc.lp + (n - 1), b->sc.ids + (n - 1), st);
}

// The embedding of the r.M ids in pf.ids_in and the layer stack over those rows of b->pf: what
// every prefill form runs between its bookkeeping and its head.
static int enqueue_prompt_layers(qie_batch* b, const LayerRows& r, const qie_kv_cache& cache, AttentionFn attend) {
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    const int64_t n = r.M;
    QIE_TRY(qie_embedding(e->w.embed, b->pf.ids_in, b->pf.x, n, s.hidden, e->stream));
    // opts.prefill_fp8: every projection on fp8 codes x fp8 weights (e->layers: the fp8 arena).
    // Otherwise bf16 rows; on an fp8 engine at >= 256 rows the GEMMs run on the dequantised bf16
    // copy (layers_pf), and with tiled fp8 projections (readable by the batched-decode kernel
    // only) every prefill of more than 16 rows does
    // (fp4 projections: codes up to 16 rows, the dequantised copy beyond — the MXFP4 kernel is their only reader)
    const bool pf16 = e->fp4 ? n > 16 : e->fp8 && !e->layers_pf.empty() && (n >= 256 || (e->fp8_t16 && n > 16));
    LayerPath path{e->layers.data(), proj_flags(e), prefill_mx(e) ? InputForm::Fp8 : InputForm::Normed};
    if (pf16 && path.in == InputForm::Normed)
        path = LayerPath{e->layers_pf.data(), 0, InputForm::Normed};
    for (int l = 0; l < s.n_layers; l++) QIE_TRY(enqueue_layer_rows(b, l, r, path, cache, attend, b->pf_ws.p));
    return 0;
}

// Prefill of n_seqs prompts of len ids each into slots seq0 .. seq0+n_seqs-1 (ids laid end
// to end): every GEMM runs once over all n_seqs * len rows, attention and the KV append see
// the prompts as sequences of rows_per_seq = len, and the head samples the n_seqs last rows
// in one launch.  n_seqs = 1 is qie_prefill.
// pos0 > 0 (qie_prefill_append, n_seqs = 1): the rows continue live sequence seq0 at positions
// pos0 .. pos0 + len - 1 — its pages are kept and grown, the ids land at history offset pos0,
// and attention over the cached prefix runs qie_attention_extend; everything else (the layer
// loop, tensor parallelism, the head) is the same code.
// score (qie_score, n_seqs = 1): after the layer loop and the unchanged last-row head, the scoring
// head runs over all len rows (enqueue_score); everything the plain call does is done as it does it.
static int prefill_rows(qie_batch* b, int seq0, int n_seqs, const int32_t* ids, int len, int pos0,
                        const qie_sampling* smp, int32_t* next_ids, const char* who, const ScoreReq* score = nullptr) {
    QIE_REQUIRE(b && ids && len > 0 && n_seqs > 0 && seq0 >= 0 && seq0 + n_seqs <= b->B && pos0 >= 0,
                "%s: bad arguments", who);
    QIE_REQUIRE(!score || (n_seqs == 1 && score->targets && score->logprobs), "%s: bad arguments", who);
    QIE_REQUIRE((int64_t)pos0 + len < b->max_ctx, "%s: %d tokens from position %d do not fit max_ctx %d", who, len,
                pos0, b->max_ctx);
    const bool append = pos0 > 0;
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    if (append) {
        QIE_REQUIRE(n_seqs == 1, "%s: one sequence per call", who);
        QIE_REQUIRE(!b->idle[seq0], "%s: slot %d holds no live sequence", who, seq0);
        QIE_REQUIRE(pos0 <= b->h_pos[seq0], "%s: pos0 %d is past sequence %d's current position %d", who, pos0, seq0,
                    b->h_pos[seq0]);
        QIE_REQUIRE(!(e->fp8 && e->opts.prefill_fp8),
                    "%s: not available on a prefill_fp8 engine (block-scaled fp8 activations are defined for a "
                    "prefill from position 0 only: an append has no reference to be checked against)", who);
    }
    const int64_t n = (int64_t)n_seqs * len;   // rows
    QIE_REQUIRE(n <= INT32_MAX, "%s: %lld rows", who, (long long)n);
    for (int64_t i = 0; i < n; i++)
        QIE_REQUIRE(ids[i] >= 0 && ids[i] < s.vocab, "%s: token id %d out of range", who, ids[i]);
    if (score)
        for (int64_t i = 0; i < n; i++)
            QIE_REQUIRE(score->targets[i] >= -1 && score->targets[i] < s.vocab,
                        "%s: target %d of row %lld is neither -1 nor a token id", who, score->targets[i], (long long)i);
    hipStream_t st = e->stream;
    // all-or-nothing, before anything is allocated or launched.  A prefill from position 0 starts a
    // new sequence in each slot: every target slot's pages go back to the pool before any slot
    // draws, and the pages only that slot holds count towards the check
    PagePool::Span spans[kMaxBatchSlots];   // n_seqs <= B <= kMaxBatchSlots
    for (int z = 0; z < n_seqs; z++) spans[z] = PagePool::Span{seq0 + z, pos0, (int64_t)pos0 + len - 1, !append};
    KvWrites kv;
    QIE_TRY(plan_kv_writes(b, spans, n_seqs, kv));
    if (!kv.fits() && append)
        return fail(-28, "%s: KV pool exhausted (%lld more pages needed for %d rows at position %d, %lld free)", who,
                    (long long)kv.r.need, len, pos0, (long long)kv.free);
    QIE_REQUIRE(kv.fits(), "%s: KV pool exhausted (%lld pages needed beyond those slots %d..%d hold alone, %lld free)",
                who, (long long)kv.r.need, seq0, seq0 + n_seqs - 1, (long long)kv.free);
    QIE_TRY(ensure_prefill_scratch(b, n, append));
    if (score) {   // the scoring head's scratch too, before anything is launched
        QIE_TRY(ensure_score_scratch(b, n, score_fused(e, score->flags)));
        if (!score_fused(e, score->flags)) QIE_TRY(ensure_verify_bufs(b));
    }
    QIE_TRY(commit_kv_writes(b, kv));
    for (int z = 0; z < n_seqs; z++) b->idle[seq0 + z] = 0;
    const int64_t H = s.hidden;
    QIE_HIP(hipMemcpyAsync(b->pf.ids_in, ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, b->pf.pos, (int)n, len, pos0);
    hipLaunchKernelGGL(copy_ids_kernel, dim3((len + 255) / 256, n_seqs), dim3(256), 0, st, b->pf.ids_in,
                       b->dec.hist + (int64_t)seq0 * b->max_ctx + pos0, len, (int64_t)b->max_ctx);
    QIE_TRY(enqueue_prompt_layers(b, layer_rows(b->pf, n, len), batch_cache(b, seq0),
                                  append ? qie_attention_extend : qie_attention));
    // position of each last prompt token; finalize advances it to pos0 + len (the new token).
    for (int z = 0; z < n_seqs; z++)
        QIE_TRY(set_slot_state(b, seq0 + z, pos0 + len - 1, 0, ids[(int64_t)z * len + len - 1], 0));
    const uint16_t* last = b->pf.x + (int64_t)(len - 1) * H;
    if (n_seqs > 1) {   // the last rows, packed (the head's pre-norm reads contiguous rows)
        QIE_HIP(hipMemcpy2DAsync(b->pf.xn, (size_t)H * 2, last, (size_t)len * H * 2, (size_t)H * 2, n_seqs,
                                 hipMemcpyDeviceToDevice, st));
        last = b->pf.xn;
    }
    QIE_TRY(enqueue_head(b, last, H, seq0, n_seqs, smp));
    for (int z = 0; z < n_seqs; z++) b->h_pos[seq0 + z] = pos0 + len;
    if (score) QIE_TRY(enqueue_score(b, seq0, len, *score));
    if (next_ids) {
        QIE_HIP(hipMemcpyAsync(next_ids, b->dec.ids + seq0, (size_t)n_seqs * 4, hipMemcpyDeviceToHost, st));
        QIE_HIP(hipStreamSynchronize(st));
        QIE_TRY(comm_check(e, who));
    }
    if (score) {
        QIE_HIP(d2h(e, score->logprobs, b->sc.lp, (size_t)len * 4));
        if (score->greedy_ids) QIE_HIP(d2h(e, score->greedy_ids, b->sc.ids, (size_t)len * 4));
        QIE_TRY(comm_check(e, who));
    }
    return 0;
}

int qie_prefill(qie_batch* b, int32_t seq, const int32_t* ids, int32_t n, const qie_sampling* smp, int32_t* next_id) {
    return prefill_rows(b, seq, 1, ids, n, 0, smp, next_id, "qie_prefill");
}

int qie_prefill_append(qie_batch* b, int32_t seq, const int32_t* ids, int32_t n, int32_t pos0,
                       const qie_sampling* smp, int32_t* next_id) {
    QIE_REQUIRE(pos0 >= 1, "qie_prefill_append: pos0 must be >= 1 (a sequence starts with qie_prefill)");
    return prefill_rows(b, seq, 1, ids, n, pos0, smp, next_id, "qie_prefill_append");
}

int qie_prefill_batch(qie_batch* b, int32_t seq0, int32_t n_seqs, const int32_t* ids, int32_t len,
                      const qie_sampling* smp, int32_t* next_ids) {
    return prefill_rows(b, seq0, n_seqs, ids, len, 0, smp, next_ids, "qie_prefill_batch");
}

// Prompts and appends of any lengths in one pass: prefill_rows with a segment
// table in place of the rectangle.  The rows' positions and history come from ragged_rows_kernel,
// the layers run the ragged q/k post-projection and attention (LayerRows::segs), and the head
// runs once per maximal run of consecutive slots over that run's packed last rows.
int qie_prefill_ragged(qie_batch* b, const qie_prefill_seg* segs, int32_t n_segs, const int32_t* ids,
                       const qie_sampling* smp, int32_t* next_ids) {
    const char* who = "qie_prefill_ragged";
    QIE_REQUIRE(b && segs && ids && n_segs >= 1 && n_segs <= b->B && n_segs <= QIE_RAGGED_MAX_SEGS,
                "%s: bad arguments (1 .. min(B, %d) segments)", who, QIE_RAGGED_MAX_SEGS);
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    QIE_REQUIRE(!e->opts.prefill_fp8,
                "%s: not available on a prefill_fp8 engine (block-scaled fp8 activations are defined for a "
                "prefill from position 0 only: an append has no reference to be checked against)", who);
    QIE_REQUIRE(b->decode_mode != 1 || n_segs == 1, "%s: one segment per call in decode mode 1", who);
    RaggedRows t{};
    PagePool::Span spans[kMaxBatchSlots];   // n_segs <= B <= kMaxBatchSlots
    int64_t n = 0;                          // rows
    for (int z = 0; z < n_segs; z++) {
        const qie_prefill_seg& g = segs[z];
        QIE_REQUIRE(g.seq >= 0 && g.seq < b->B && g.n >= 1 && g.pos0 >= 0 && (z == 0 || g.seq > segs[z - 1].seq),
                    "%s: segment %d: bad arguments (slots strictly increasing, n >= 1, pos0 >= 0)", who, z);
        QIE_REQUIRE((int64_t)g.pos0 + g.n < b->max_ctx, "%s: %d tokens from position %d do not fit max_ctx %d", who,
                    g.n, g.pos0, b->max_ctx);
        if (g.pos0 > 0) {
            QIE_REQUIRE(!b->idle[g.seq], "%s: slot %d holds no live sequence", who, g.seq);
            QIE_REQUIRE(g.pos0 <= b->h_pos[g.seq], "%s: pos0 %d is past sequence %d's current position %d", who,
                        g.pos0, g.seq, b->h_pos[g.seq]);
        }
        t.segs.row0[z] = (int32_t)n, t.segs.seq[z] = g.seq, t.pos0[z] = g.pos0;
        spans[z] = PagePool::Span{g.seq, g.pos0, (int64_t)g.pos0 + g.n - 1, g.pos0 == 0};
        n += g.n;
    }
    t.segs.n = n_segs;
    for (int z = n_segs; z <= QIE_RAGGED_MAX_SEGS; z++) t.segs.row0[z] = (int32_t)n;
    for (int64_t i = 0; i < n; i++)
        QIE_REQUIRE(ids[i] >= 0 && ids[i] < s.vocab, "%s: token id %d out of range", who, ids[i]);
    hipStream_t st = e->stream;
    // all-or-nothing, before anything is allocated or launched: one reservation over every segment
    KvWrites kv;
    QIE_TRY(plan_kv_writes(b, spans, n_segs, kv));
    if (!kv.fits())
        return fail(-28, "%s: KV pool exhausted (%lld more pages needed for %lld rows in %d segments, %lld free)", who,
                    (long long)kv.r.need, (long long)n, n_segs, (long long)kv.free);
    QIE_TRY(ensure_prefill_scratch(b, n, true));
    QIE_TRY(commit_kv_writes(b, kv));
    for (int z = 0; z < n_segs; z++) b->idle[segs[z].seq] = 0;
    const int64_t H = s.hidden;
    QIE_HIP(hipMemcpyAsync(b->pf.ids_in, ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ragged_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t, b->pf.ids_in,
                       b->pf.pos, b->dec.hist, (int64_t)b->max_ctx);
    QIE_LAUNCH_CHECK();
    QIE_TRY(enqueue_prompt_layers(b, layer_rows(b->pf, n, 0, &t.segs), batch_cache(b, 0), nullptr));
    // position of each last id (finalize advances it to pos0 + n: the new token), and the last rows
    // packed in segment order into pf.xn, which is free after the layer loop
    for (int z = 0; z < n_segs; z++) {
        const qie_prefill_seg& g = segs[z];
        const int64_t last = t.segs.row0[z + 1] - 1;
        QIE_TRY(set_slot_state(b, g.seq, g.pos0 + g.n - 1, 0, ids[last], 0));
        QIE_HIP(hipMemcpyAsync(b->pf.xn + z * H, b->pf.x + last * H, (size_t)H * 2, hipMemcpyDeviceToDevice, st));
    }
    for (int z0 = 0, z1; z0 < n_segs; z0 = z1) {   // one head per run of consecutive slots
        for (z1 = z0 + 1; z1 < n_segs && segs[z1].seq == segs[z1 - 1].seq + 1;) z1++;
        QIE_TRY(enqueue_head(b, b->pf.xn + z0 * H, H, segs[z0].seq, z1 - z0, smp));
    }
    for (int z = 0; z < n_segs; z++) b->h_pos[segs[z].seq] = segs[z].pos0 + segs[z].n;
    if (next_ids) {
        int32_t all[kMaxBatchSlots];
        QIE_HIP(hipMemcpyAsync(all, b->dec.ids, (size_t)b->B * 4, hipMemcpyDeviceToHost, st));
        QIE_HIP(hipStreamSynchronize(st));
        QIE_TRY(comm_check(e, who));
        for (int z = 0; z < n_segs; z++) next_ids[z] = all[segs[z].seq];
    }
    return 0;
}

int qie_score(qie_batch* b, int32_t seq, const int32_t* ids, int32_t n, int32_t pos0, const int32_t* targets,
              const qie_sampling* smp, int32_t flags, float* logprobs, int32_t* greedy_ids, int32_t* next_id) {
    QIE_REQUIRE(targets && logprobs && (flags & ~QIE_SCORE_UNFUSED) == 0, "qie_score: bad arguments");
    const ScoreReq rq{targets, flags, logprobs, greedy_ids};
    return prefill_rows(b, seq, 1, ids, n, pos0, smp, next_id, "qie_score", &rq);
}

int qie_batch_logprobs(qie_batch* b, const int32_t* ids, float* out) {
    QIE_REQUIRE(b && ids && out, "qie_batch_logprobs: bad arguments");
    qie_engine* e = b->e;
    const int64_t V = e->spec.vocab;
    for (int m = 0; m < b->B; m++)
        QIE_REQUIRE(ids[m] >= -1 && ids[m] < V, "qie_batch_logprobs: id %d of slot %d is neither -1 nor a token id",
                    ids[m], m);
    QIE_TRY(ensure_score_scratch(b, b->B, false));
    const uint16_t* src = b->dec.logits;
    if (use_comm(e)) {   // collective: every rank calls this at the same point
        QIE_TRY(gather_logits(b, 0, b->B));
        src = b->dec.logits_full;
    }
    QIE_HIP(hipMemcpyAsync(b->sc.tgt, ids, (size_t)b->B * 4, hipMemcpyHostToDevice, e->stream));
    QIE_TRY(qie_logprob_rows(src, b->B, V, V, b->sc.tgt, b->sc.lp, nullptr, e->stream));
    QIE_HIP(hipStreamSynchronize(e->stream));
    QIE_TRY(comm_check(e, "qie_batch_logprobs"));
    QIE_TRY(pk_check(b));
    QIE_HIP(d2h(e, out, b->sc.lp, (size_t)b->B * 4));
    return 0;
}

static bool same_sampling(const qie_sampling& a, const qie_sampling* b) {
    qie_sampling g{1, 0.f, 1.f, 0};
    const qie_sampling& bb = b ? *b : g;
    return a.top_k == bb.top_k && a.temperature == bb.temperature && a.top_p == bb.top_p && a.seed == bb.seed;
}

// dev (QIE_GRAPH_DUMP): every node of a captured graph (type, grid, block, LDS)
static void dump_graph(hipGraph_t g) {
    size_t n = 0;
    hipGraphGetNodes(g, nullptr, &n);
    std::vector<hipGraphNode_t> nodes(n);
    hipGraphGetNodes(g, nodes.data(), &n);
    size_t max_shm = 0;
    for (size_t i = 0; i < n; i++) {
        hipGraphNodeType t;
        hipGraphNodeGetType(nodes[i], &t);
        if (t == hipGraphNodeTypeKernel) {
            hipKernelNodeParams kp{};
            hipGraphKernelNodeGetParams(nodes[i], &kp);
            max_shm = std::max(max_shm, (size_t)kp.sharedMemBytes);
            fprintf(stderr, "graph node %zu: kernel %p grid %u,%u,%u block %u,%u,%u dyn_lds %u\n", i, kp.func,
                    kp.gridDim.x, kp.gridDim.y, kp.gridDim.z, kp.blockDim.x, kp.blockDim.y, kp.blockDim.z,
                    kp.sharedMemBytes);
        } else {
            fprintf(stderr, "graph node %zu: type %d\n", i, (int)t);
        }
    }
    fprintf(stderr, "graph: %zu nodes, max dynamic LDS %zu B\n", n, max_shm);
}

// What `enqueue` puts on the engine's stream, captured (thread-local mode) and instantiated
// into *out; the graph is destroyed on every path.  `who` prefixes the failure messages.
static int capture_graph(qie_engine* e, const char* who, const std::function<int()>& enqueue, hipGraphExec_t* out) {
    hipGraph_t g = nullptr;
    QIE_HIP(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    hipError_t he = hipStreamEndCapture(e->stream, &g);
    if (rc || he != hipSuccess) {
        if (g) hipGraphDestroy(g);
        return rc ? rc : fail((int)he, "%sgraph capture: %s", who, hipGetErrorString(he));
    }
    if (dev_env("QIE_GRAPH_DUMP", 0)) dump_graph(g);
    he = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (he != hipSuccess) return fail((int)he, "%sgraph instantiate: %s", who, hipGetErrorString(he));
    return 0;
}

static int launch_step(qie_batch* b, const qie_sampling* smp) {
    qie_engine* e = b->e;
    if (!e->opts.use_graph) return enqueue_decode(b, smp);
    // (entry VALUES are read from the device table: only "some slot has an entry" is captured)
    if (!b->graph_ok || !same_sampling(b->gs, smp) || b->g_entries != (b->n_slot_set > 0)) {
        if (b->gexec) hipGraphExecDestroy(b->gexec);
        b->gexec = nullptr;
        b->graph_ok = false;
        QIE_TRY(capture_graph(e, "", [&] { return enqueue_decode(b, smp); }, &b->gexec));
        b->gs = smp ? *smp : qie_sampling{1, 0.f, 1.f, 0};
        b->g_entries = b->n_slot_set > 0;
        b->graph_ok = true;
    }
    QIE_HIP(hipGraphLaunch(b->gexec, e->stream));
    return 0;
}

// Before n_steps decode steps: every live sequence fits max_ctx and holds the pages the
// steps write (positions h_pos .. h_pos + n_steps - 1); idle slots are rewound to
// position 0 when they would run past max_ctx.  Nothing is launched on failure.
static int prepare_steps(qie_batch* b, int n_steps, const char* who) {
    QIE_REQUIRE(n_steps < b->max_ctx, "%s: %d steps exceed max_ctx %d", who, n_steps, b->max_ctx);
    for (int m = 0; m < b->B; m++)
        if (!b->idle[m])
            QIE_REQUIRE(b->h_pos[m] + n_steps < b->max_ctx, "%s: sequence %d would exceed max_ctx %d", who, m,
                        b->max_ctx);
    // growth, plus a private copy of any shared page in the steps' range (only a slot rewound
    // below a fork point has one: a fork copies its tail page eagerly)
    PagePool::Span spans[kMaxBatchSlots];
    int n = 0;
    for (int m = 0; m < b->B; m++)
        if (!b->idle[m]) spans[n++] = PagePool::Span{m, b->h_pos[m], (int64_t)b->h_pos[m] + n_steps - 1, false};
    KvWrites kv;
    QIE_TRY(plan_kv_writes(b, spans, n, kv));
    QIE_REQUIRE(kv.fits(), "%s: KV pool exhausted (%lld pages needed, %lld free)", who, (long long)kv.r.need,
                (long long)kv.free);
    QIE_TRY(commit_kv_writes(b, kv));
    for (int m = 0; m < b->B; m++)
        if (b->idle[m] && b->h_pos[m] + n_steps >= b->max_ctx) {
            QIE_TRY(set_slot_state(b, m, 0, 0, 0, 1));
            b->h_pos[m] = 0;
        }
    return 0;
}

int qie_decode_step(qie_batch* b, const qie_sampling* smp, int32_t* next_ids) {
    QIE_REQUIRE(b, "qie_decode_step: null batch");
    QIE_TRY(prepare_steps(b, 1, "qie_decode_step"));
    QIE_TRY(launch_step(b, smp));
    for (int m = 0; m < b->B; m++) b->h_pos[m] += 1;
    return sync_ids(b, next_ids);
}

int qie_decode(qie_batch* b, int32_t n_steps, const qie_sampling* smp, int32_t* out_ids) {
    QIE_REQUIRE(b && n_steps >= 0, "qie_decode: bad arguments");
    QIE_TRY(prepare_steps(b, n_steps, "qie_decode"));
    std::vector<int32_t> p0 = b->h_pos;
    for (int i = 0; i < n_steps; i++) {
        QIE_TRY(launch_step(b, smp));
        for (int m = 0; m < b->B; m++) b->h_pos[m] += 1;
    }
    QIE_HIP(hipStreamSynchronize(b->e->stream));
    QIE_TRY(comm_check(b->e, "qie_decode"));
    QIE_TRY(pk_check(b));
    if (out_ids && n_steps > 0) {
        std::vector<int32_t> row(b->max_ctx);
        for (int m = 0; m < b->B; m++) {
            QIE_HIP(d2h(b->e, row.data(), b->dec.hist + (int64_t)m * b->max_ctx, (size_t)b->max_ctx * 4));
            for (int i = 0; i < n_steps; i++) out_ids[(int64_t)i * b->B + m] = row[p0[m] + 1 + i];
        }
    }
    return 0;
}

int qie_batch_logits(qie_batch* b, void* host_out) {
    QIE_REQUIRE(b && host_out, "qie_batch_logits: bad arguments");
    const uint16_t* src = b->dec.logits;
    if (use_comm(b->e)) {   // collective: every rank calls this at the same point
        QIE_TRY(gather_logits(b, 0, b->B));
        src = b->dec.logits_full;
    }
    QIE_HIP(hipStreamSynchronize(b->e->stream));
    QIE_TRY(comm_check(b->e, "qie_batch_logits"));
    QIE_TRY(pk_check(b));
    QIE_HIP(d2h(b->e, host_out, src, (size_t)b->B * b->e->spec.vocab * 2));
    return 0;
}

int qie_batch_positions(qie_batch* b, int32_t* host_pos) {
    QIE_REQUIRE(b && host_pos, "qie_batch_positions: bad arguments");
    QIE_HIP(hipStreamSynchronize(b->e->stream));
    QIE_HIP(d2h(b->e, host_pos, b->dec.pos, (size_t)b->B * 4));
    return 0;
}

int qie_batch_history(qie_batch* b, int32_t seq, int32_t* host_ids, int32_t n) {
    QIE_REQUIRE(b && host_ids && seq >= 0 && seq < b->B && n >= 0 && n <= b->max_ctx,
                "qie_batch_history: bad arguments");
    QIE_HIP(hipStreamSynchronize(b->e->stream));
    QIE_HIP(d2h(b->e, host_ids, b->dec.hist + (int64_t)seq * b->max_ctx, (size_t)n * 4));
    return 0;
}

// ------------------------------------------------------------ speculative verify
// The step's rows, once per batch at kVerifyMaxRows rows and never reallocated: captured steps
// (and the unfused scoring path) keep valid pointers for the batch's lifetime.
static int ensure_verify_bufs(qie_batch* b) {
    if (b->v.mem) return 0;
    qie_engine* e = b->e;
    RowDims d = row_dims(e, kVerifyMaxRows);
    d.attn_ws_bytes = qie_attention_extend_workspace_bytes(d.rows, e->sh.nq, e->spec.head_dim, b->max_ctx + b->run_pad);
    d.samp_ws_bytes = qie_sample_workspace_bytes(d.rows, e->spec.vocab);
    VerifyRows v;
    QIE_TRY(alloc_rows(v, d.rows, [&](Carver& c, VerifyRows& r) { carve_verify(c, r, d); }));
    // key slots start zero (the commit kernel leaves them so); the fp8 batched-decode kernel's
    // split-K workspace must exist before a capture (batch 1 never made it for M = 1)
    hipError_t he = hipMemsetAsync(v.mem, 0, v.bytes, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    int rc = he == hipSuccess ? 0 : fail((int)he, "qie_verify: buffer init: %s", hipGetErrorString(he));
    if (!rc && e->fp8) rc = dec8_reserve(e->stream);
    if (!rc && e->fp4) rc = dec4_reserve(e->stream);
    if (rc) {
        hipFree(v.mem);
        return rc;
    }
    b->v = v;
    return 0;
}

// rows -> layers -> head -> commit, all on device state: capturable as one linear chain
static int enqueue_verify(qie_batch* b, int seq, int M, const qie_sampling* smp) {
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    hipStream_t st = e->stream;
    const int64_t H8 = (int64_t)s.hidden / 8;
    VerifyRowsArgs ra{seq, M, b->v.draft, s.vocab, (const uint4*)e->w.embed, (const uint4*)b->dec.x, H8,
                      b->dec.pos, b->dec.step, (uint4*)b->v.x, b->v.pos, b->v.step};
    QIE_TRY(launch_verify_rows(ra, st));
    const qie_kv_cache cache = batch_cache(b, seq);
    // the M rows of ONE sequence at consecutive positions v.pos, in the decode input form
    const LayerRows r = layer_rows(b->v, M, M);
    for (int l = 0; l < s.n_layers; l++)
        QIE_TRY(enqueue_layer_rows(b, l, r, decode_path(e), cache, qie_attention_extend, b->v.attn_ws));
    // with an entry: row i's window ends at p + i, history [.. p] and then the drafts d1 .. di
    const EntryRows er{seq, 0, b->v.pos, b->v.draft, b->d_tail_len};
    const bool entries = any_entry(b, seq, 1);
    QIE_TRY(enqueue_head_rows(b, b->v.x, s.hidden, M, smp, head_bufs(b->v, 0, b->e->sh.vocab), entries ? &er : nullptr));
    const bool greedy = !entries && is_greedy(smp);
    VerifyCommitArgs ca{seq, M, greedy ? b->v.keys : nullptr, b->v.ids, b->v.draft, s.vocab, b->dec.pos, b->dec.step,
                        b->dec.hist, b->max_ctx, b->dec.ids, (const uint4*)e->w.embed, (uint4*)b->dec.x, H8,
                        rope_cur_args(b), b->v.logits, b->dec.logits, (int64_t)e->sh.vocab, b->v.res};
    return launch_verify_commit(ca, st);
}

// eager, or the captured step of (seq, M, sampling): captured once on the engine's stream
// (a linear chain, no forked branches), replayed afterwards
static int launch_verify(qie_batch* b, int seq, int M, const qie_sampling* smp) {
    qie_engine* e = b->e;
    if (!e->opts.use_graph) return enqueue_verify(b, seq, M, smp);
    const bool greedy = is_greedy(smp), entries = any_entry(b, seq, 1);
    for (const auto& g : b->v_graphs)
        if (g.seq == seq && g.M == M && g.entries == entries &&
            (entries || (g.greedy == greedy && (greedy || same_sampling(g.smp, smp))))) {
            QIE_HIP(hipGraphLaunch(g.exec, e->stream));
            return 0;
        }
    if (b->v_graphs.size() >= 64) {   // bounded: drop the oldest captured step
        hipGraphExecDestroy(b->v_graphs.front().exec);
        b->v_graphs.erase(b->v_graphs.begin());
    }
    hipGraphExec_t exec = nullptr;
    QIE_TRY(capture_graph(e, "qie_verify: ", [&] { return enqueue_verify(b, seq, M, smp); }, &exec));
    b->v_captures++;
    b->v_graphs.push_back({seq, M, entries, greedy, smp ? *smp : qie_sampling{1, 0.f, 1.f, 0}, exec});
    QIE_HIP(hipGraphLaunch(exec, e->stream));
    return 0;
}

int qie_verify(qie_batch* b, int32_t seq, const int32_t* draft, int32_t n_draft, const qie_sampling* smp,
               int32_t* out_ids, int32_t* n_out) {
    QIE_REQUIRE(b && out_ids && n_out && seq >= 0 && seq < b->B && n_draft >= 0 && (n_draft == 0 || draft),
                "qie_verify: bad arguments");
    QIE_REQUIRE(n_draft + 1 <= QIE_VERIFY_MAX_ROWS, "qie_verify: %d drafts exceed the %d rows of a step (at most %d)",
                n_draft, QIE_VERIFY_MAX_ROWS, QIE_VERIFY_MAX_ROWS - 1);
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    QIE_REQUIRE(!b->idle[seq], "qie_verify: slot %d holds no live sequence", seq);
    QIE_REQUIRE(!(e->fp8 && e->opts.prefill_fp8),
                "qie_verify: not available on a prefill_fp8 engine (block-scaled fp8 activations are defined for a "
                "prefill from position 0 only)");
    QIE_REQUIRE(b->decode_mode == 0, "qie_verify: the batch is in decode mode 1 (the persistent step); verify runs "
                                     "the five-launch layer, set mode 0 first");
    for (int i = 0; i < n_draft; i++)
        QIE_REQUIRE(draft[i] >= 0 && draft[i] < s.vocab, "qie_verify: draft id %d out of range", draft[i]);
    const int p = b->h_pos[seq], M = n_draft + 1;
    QIE_REQUIRE((int64_t)p + n_draft + 1 < b->max_ctx, "qie_verify: %d rows from position %d do not fit max_ctx %d", M,
                p, b->max_ctx);
    // all-or-nothing, before anything is allocated or launched (growth + a private copy of a shared page)
    const PagePool::Span span{seq, p, (int64_t)p + M - 1, false};
    KvWrites kv;
    QIE_TRY(plan_kv_writes(b, &span, 1, kv));
    if (!kv.fits())
        return fail(-28, "qie_verify: KV pool exhausted (%lld more pages needed for %d rows at position %d, %lld free)",
                    (long long)kv.r.need, M, p, (long long)kv.free);
    QIE_TRY(ensure_verify_bufs(b));
    QIE_TRY(commit_kv_writes(b, kv));
    hipStream_t st = e->stream;
    if (n_draft > 0) QIE_HIP(hipMemcpyAsync(b->v.draft, draft, (size_t)n_draft * 4, hipMemcpyHostToDevice, st));
    QIE_TRY(launch_verify(b, seq, M, smp));
    // the accepted count and the ids (and the exchange error word) in one stream-ordered batch
    int32_t res[kVerifyMaxRows + 1] = {0};
    QIE_TRY(read_back(b, res, b->v.res, (size_t)(M + 1) * 4, "qie_verify"));
    const int n = res[0];
    if (n < 1 || n > M) return fail(-5, "qie_verify: the step reported %d accepted rows of %d", n, M);
    for (int i = 0; i < n; i++) out_ids[i] = res[1 + i];
    *n_out = n;
    b->h_pos[seq] = p + n;
    b->v_rows = M;
    return 0;
}

int qie_verify_logits(qie_batch* b, void* host_out) {
    QIE_REQUIRE(b && host_out, "qie_verify_logits: bad arguments");
    QIE_REQUIRE(b->v.mem && b->v_rows > 0, "qie_verify_logits: no qie_verify has run on this batch");
    qie_engine* e = b->e;
    const uint16_t* src = b->v.logits;
    if (use_comm(e)) {   // collective: every rank calls this at the same point
        QIE_TRY(gather_rows(b, head_bufs(b->v, 0, b->e->sh.vocab), b->v_rows));
        src = b->v.logits_full;
    }
    QIE_HIP(hipStreamSynchronize(e->stream));
    QIE_TRY(comm_check(e, "qie_verify_logits"));
    QIE_HIP(d2h(e, host_out, src, (size_t)b->v_rows * e->spec.vocab * 2));
    return 0;
}

// ------------------------------------------------------------ the batched verify step
// the step's words beside the rows `v`: made once, never reallocated (captured steps hold them)
static int ensure_verify_batch_bufs(qie_batch* b) {
    QIE_TRY(ensure_verify_bufs(b));
    if (b->vb_aux) return 0;
    const size_t bytes = (size_t)(kVerifyBatchResWords + 3 * kVerifyMaxRows) * 4;
    void* p = nullptr;
    QIE_TRY(dmalloc(&p, bytes));
    hipError_t he = hipMemsetAsync(p, 0, bytes, b->e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(b->e->stream);
    if (he != hipSuccess) {
        hipFree(p);
        return fail((int)he, "qie_verify_batch: buffer init: %s", hipGetErrorString(he));
    }
    b->vb_aux = (int32_t*)p;
    return 0;
}

static bool any_entry_segs(const qie_batch* b, const qie_row_segs& t) {
    if (b->n_slot_set == 0) return false;
    for (int z = 0; z < t.n; z++)
        if (b->slot_set[t.seq[z]]) return true;
    return false;
}

// enqueue_verify over segments: rows -> the decode-form layers in their ragged forms -> one head
// over all M rows -> commit per segment; a linear chain on device state, capturable
static int enqueue_verify_batch(qie_batch* b, const qie_row_segs& t, const qie_sampling* smp) {
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    hipStream_t st = e->stream;
    const int64_t H8 = (int64_t)s.hidden / 8;
    const int M = t.row0[t.n];
    int32_t* res = b->vb_aux;
    int32_t *row_slot = res + kVerifyBatchResWords, *tail_off = row_slot + kVerifyMaxRows,
            *tail_len = tail_off + kVerifyMaxRows;
    VerifyBatchRowsArgs ra{t, b->v.draft, s.vocab, (const uint4*)e->w.embed, (const uint4*)b->dec.x, H8, b->dec.pos,
                           b->dec.step, (uint4*)b->v.x, b->v.pos, b->v.step, row_slot, tail_off, tail_len};
    QIE_TRY(launch_verify_batch_rows(ra, st));
    const qie_kv_cache cache = batch_cache(b, 0);   // the table names the batch's slots
    const LayerRows r = layer_rows(b->v, M, 0, &t);
    for (int l = 0; l < s.n_layers; l++)
        QIE_TRY(enqueue_layer_rows(b, l, r, decode_path(e), cache, nullptr, b->v.attn_ws));
    // with an entry: row i of a segment sees its slot's history [.. p] and then that segment's d1 .. di
    EntryRows er{0, 0, b->v.pos, b->v.draft, tail_len};
    er.row_slot = row_slot, er.tail_off = tail_off;
    const bool entries = any_entry_segs(b, t);
    QIE_TRY(enqueue_head_rows(b, b->v.x, s.hidden, M, smp, head_bufs(b->v, 0, e->sh.vocab), entries ? &er : nullptr));
    const bool greedy = !entries && is_greedy(smp);
    VerifyBatchCommitArgs ca{t, greedy ? b->v.keys : nullptr, b->v.ids, b->v.draft, s.vocab, b->dec.pos, b->dec.step,
                             b->dec.hist, b->max_ctx, b->dec.ids, (const uint4*)e->w.embed, (uint4*)b->dec.x, H8,
                             rope_cur_args(b), b->v.logits, b->dec.logits, (int64_t)e->sh.vocab, res};
    return launch_verify_batch_commit(ca, st);
}

static bool every_entry_segs(const qie_batch* b, const qie_row_segs& t) {
    for (int z = 0; z < t.n; z++)
        if (!b->slot_set[t.seq[z]]) return false;
    return true;
}

static bool same_segs(const qie_row_segs& a, const qie_row_segs& b) {
    if (a.n != b.n) return false;
    for (int z = 0; z < a.n; z++)
        if (a.seq[z] != b.seq[z] || a.row0[z + 1] != b.row0[z + 1]) return false;
    return true;
}

// eager, or the captured step of (segment table, sampling kind, entries) in v_graphs (launch_verify's
// cache and bound; seq = -1 keeps the two kinds apart).  The call's sampling is part of the step
// unless EVERY segment's slot holds an entry: rows of a slot without one sample under it
// (qie_sample_rows' fallback, a by-value launch argument), as the decode graph's do.
static int launch_verify_batch(qie_batch* b, const qie_row_segs& t, const qie_sampling* smp) {
    qie_engine* e = b->e;
    if (!e->opts.use_graph) return enqueue_verify_batch(b, t, smp);
    const bool greedy = is_greedy(smp), entries = any_entry_segs(b, t), all = entries && every_entry_segs(b, t);
    for (const auto& g : b->v_graphs)
        if (g.seq == -1 && same_segs(g.segs, t) && g.entries == entries && g.all_entries == all &&
            (all || (g.greedy == greedy && (greedy || same_sampling(g.smp, smp))))) {
            QIE_HIP(hipGraphLaunch(g.exec, e->stream));
            return 0;
        }
    if (b->v_graphs.size() >= 64) {   // bounded: drop the oldest captured step
        hipGraphExecDestroy(b->v_graphs.front().exec);
        b->v_graphs.erase(b->v_graphs.begin());
    }
    hipGraphExec_t exec = nullptr;
    QIE_TRY(capture_graph(e, "qie_verify_batch: ", [&] { return enqueue_verify_batch(b, t, smp); }, &exec));
    b->v_graphs.push_back({-1, t.row0[t.n], entries, greedy, smp ? *smp : qie_sampling{1, 0.f, 1.f, 0}, exec, t, all});
    b->v_captures++;
    QIE_HIP(hipGraphLaunch(exec, e->stream));
    return 0;
}

int qie_verify_batch(qie_batch* b, const qie_verify_seg* segs, int32_t n_segs, const int32_t* draft,
                     const qie_sampling* smp, int32_t* out_ids, int32_t* n_out) {
    const char* who = "qie_verify_batch";
    QIE_REQUIRE(b && segs && out_ids && n_out && n_segs >= 1 && n_segs <= b->B && n_segs <= QIE_RAGGED_MAX_SEGS,
                "%s: bad arguments (1 .. min(B, %d) segments)", who, QIE_RAGGED_MAX_SEGS);
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    QIE_REQUIRE(!(e->fp8 && e->opts.prefill_fp8),
                "%s: not available on a prefill_fp8 engine (block-scaled fp8 activations are defined for a "
                "prefill from position 0 only)", who);
    QIE_REQUIRE(b->decode_mode == 0, "%s: the batch is in decode mode 1 (the persistent step); verify runs "
                                     "the five-launch layer, set mode 0 first", who);
    qie_row_segs t{};
    PagePool::Span spans[kMaxBatchSlots];   // n_segs <= B <= kMaxBatchSlots
    int M = 0;
    for (int z = 0; z < n_segs; z++) {
        const qie_verify_seg& g = segs[z];
        QIE_REQUIRE(g.seq >= 0 && g.seq < b->B && g.n_draft >= 0 && (z == 0 || g.seq > segs[z - 1].seq),
                    "%s: segment %d: bad arguments (slots strictly increasing, n_draft >= 0)", who, z);
        QIE_REQUIRE(!b->idle[g.seq], "%s: slot %d holds no live sequence", who, g.seq);
        QIE_REQUIRE(g.n_draft < QIE_VERIFY_MAX_ROWS && M + g.n_draft + 1 <= QIE_VERIFY_MAX_ROWS,
                    "%s: the segments' rows (a current token and the drafts each) exceed the %d rows of a step", who,
                    QIE_VERIFY_MAX_ROWS);
        const int p = b->h_pos[g.seq];
        QIE_REQUIRE((int64_t)p + g.n_draft + 1 < b->max_ctx, "%s: %d rows of slot %d from position %d do not fit max_ctx %d",
                    who, g.n_draft + 1, g.seq, p, b->max_ctx);
        t.row0[z] = M, t.seq[z] = g.seq;
        spans[z] = PagePool::Span{g.seq, p, (int64_t)p + g.n_draft, false};
        M += g.n_draft + 1;
    }
    t.n = n_segs;
    for (int z = n_segs; z <= QIE_RAGGED_MAX_SEGS; z++) t.row0[z] = M;
    const int n_drafts = M - n_segs;
    QIE_REQUIRE(n_drafts == 0 || draft, "%s: bad arguments (drafts without ids)", who);
    for (int i = 0; i < n_drafts; i++)
        QIE_REQUIRE(draft[i] >= 0 && draft[i] < s.vocab, "%s: draft id %d out of range", who, draft[i]);
    // all-or-nothing, before anything is allocated or launched: one reservation over every segment
    // (growth + a private copy of every shared page of the write ranges)
    KvWrites kv;
    QIE_TRY(plan_kv_writes(b, spans, n_segs, kv));
    if (!kv.fits())
        return fail(-28, "%s: KV pool exhausted (%lld more pages needed for %d rows in %d segments, %lld free)", who,
                    (long long)kv.r.need, M, n_segs, (long long)kv.free);
    QIE_TRY(ensure_verify_batch_bufs(b));
    QIE_TRY(commit_kv_writes(b, kv));
    hipStream_t st = e->stream;
    if (n_drafts > 0) QIE_HIP(hipMemcpyAsync(b->v.draft, draft, (size_t)n_drafts * 4, hipMemcpyHostToDevice, st));
    QIE_TRY(launch_verify_batch(b, t, smp));
    // every segment's accepted count and ids (and the exchange error word) in one stream-ordered batch
    int32_t res[kVerifyBatchResWords] = {0};
    QIE_TRY(read_back(b, res, b->vb_aux, (size_t)(kVerifyMaxSegs + M) * 4, who));
    for (int z = 0; z < n_segs; z++)
        if (res[z] < 1 || res[z] > segs[z].n_draft + 1)
            return fail(-5, "%s: the step reported %d accepted rows of %d in segment %d", who, res[z],
                        segs[z].n_draft + 1, z);
    for (int z = 0; z < n_segs; z++) {
        for (int i = 0; i < res[z]; i++) out_ids[t.row0[z] + i] = res[kVerifyMaxSegs + t.row0[z] + i];
        n_out[z] = res[z];
        b->h_pos[segs[z].seq] += res[z];
    }
    b->v_rows = M;
    return 0;
}

int qie_batch_debug_verify_captures(const qie_batch* b) { return b ? b->v_captures : -22; }

int qie_verify_logprobs(qie_batch* b, const int32_t* ids, float* out) {
    QIE_REQUIRE(b && ids && out, "qie_verify_logprobs: bad arguments");
    QIE_REQUIRE(b->v.mem && b->v_rows > 0, "qie_verify_logprobs: no qie_verify or qie_verify_batch has run on this batch");
    qie_engine* e = b->e;
    const int64_t V = e->spec.vocab;
    const int rows = b->v_rows;
    for (int m = 0; m < rows; m++)
        QIE_REQUIRE(ids[m] >= -1 && ids[m] < V, "qie_verify_logprobs: id %d of row %d is neither -1 nor a token id",
                    ids[m], m);
    QIE_TRY(ensure_score_scratch(b, rows, false));
    const uint16_t* src = b->v.logits;
    if (use_comm(e)) {   // collective: every rank calls this at the same point
        QIE_TRY(gather_rows(b, head_bufs(b->v, 0, e->sh.vocab), rows));
        src = b->v.logits_full;
    }
    QIE_HIP(hipMemcpyAsync(b->sc.tgt, ids, (size_t)rows * 4, hipMemcpyHostToDevice, e->stream));
    QIE_TRY(qie_logprob_rows(src, rows, V, V, b->sc.tgt, b->sc.lp, nullptr, e->stream));
    QIE_HIP(hipStreamSynchronize(e->stream));
    QIE_TRY(comm_check(e, "qie_verify_logprobs"));
    QIE_HIP(d2h(e, out, b->sc.lp, (size_t)rows * 4));
    return 0;
}

int qie_batch_set_decode_mode(qie_batch* b, int32_t mode) {
    QIE_REQUIRE(b && (mode == 0 || mode == 1), "qie_batch_set_decode_mode: bad arguments (mode 0 or 1)");
    qie_engine* e = b->e;
    if (mode == 1) {
        const char* why = "";
        QIE_REQUIRE(persist_supported(e->spec, b->B, e->sh.tp, e->fp8, e->fp4, b->d_table != nullptr, device_cu_count(), &why),
                    "qie_batch_set_decode_mode: the persistent decode step does not cover this batch (%s)", why);
        if (!b->pk_mem || !b->d_layers || !b->d_attp) {
            // all three or none: a failed allocation leaves the batch in mode 0 with nothing held
            const size_t gb = (size_t)persist_granule_count(e->spec) * 8 + 64;
            hipFree(b->pk_mem);
            hipFree(b->d_layers);
            hipFree(b->d_attp);
            b->pk_mem = nullptr;
            b->d_layers = nullptr;
            b->d_attp = nullptr;
            void *pk = nullptr, *dl = nullptr, *ap = nullptr;
            if (dmalloc(&pk, gb) || dmalloc(&dl, sizeof(qie_layer_weights) * e->layers.size()) ||
                dmalloc(&ap, persist_attn_table_bytes((int)e->layers.size()))) {
                hipFree(pk);
                hipFree(dl);
                hipFree(ap);
                return fail(-2, "qie_batch_set_decode_mode: device allocation failed: %s", qie_last_error());
            }
            b->pk_mem = pk;
            b->d_layers = (qie_layer_weights*)dl;
            b->d_attp = ap;
            QIE_HIP(hipMemsetAsync(b->pk_mem, 0, gb, e->stream));
            QIE_HIP(hipMemcpyAsync(b->d_layers, e->layers.data(), sizeof(qie_layer_weights) * e->layers.size(),
                                   hipMemcpyHostToDevice, e->stream));
            const qie_kv_cache cache = batch_cache(b, 0);
            set_decode_rope_cur(b->dec.rope_cur);
            const int rc = persist_attn_table(e->spec, e->layers.data(), b->dec.qkv, b->dec.pos, e->rope_cos, e->rope_sin,
                                              &cache, b->dec.dec_ws, b->d_attp, e->stream);
            set_decode_rope_cur(nullptr);
            QIE_TRY(rc);
            QIE_HIP(hipStreamSynchronize(e->stream));
        }
    }
    if (mode != b->decode_mode) b->graph_ok = false;   // re-captured at the next step
    b->decode_mode = mode;
    return 0;
}

int qie_batch_decode_mode(const qie_batch* b) { return b ? b->decode_mode : -22; }

int qie_batch_pk_trace(qie_batch* b, int32_t enable, uint64_t* host_out, int64_t n) {
    QIE_REQUIRE(b, "qie_batch_pk_trace: null batch");
    qie_engine* e = b->e;
    const int64_t need = (int64_t)device_cu_count() * e->spec.n_layers * persist_ts_slots();
    if (enable && !b->pk_ts) {
        QIE_TRY(dmalloc((void**)&b->pk_ts, (size_t)need * 8));
        QIE_HIP(hipMemsetAsync(b->pk_ts, 0, (size_t)need * 8, e->stream));
        b->graph_ok = false;
    }
    if (host_out) {
        QIE_REQUIRE(b->pk_ts && n >= need, "qie_batch_pk_trace: tracing off or n < %lld", (long long)need);
        QIE_HIP(hipStreamSynchronize(e->stream));
        QIE_HIP(d2h(e, host_out, b->pk_ts, (size_t)need * 8));
    }
    if (!enable && b->pk_ts) {
        QIE_HIP(hipStreamSynchronize(e->stream));
        hipFree(b->pk_ts);
        b->pk_ts = nullptr;
        b->graph_ok = false;
    }
    return 0;
}

int qie_batch_dims(const qie_batch* b, int32_t* batch, int32_t* max_ctx) {
    QIE_REQUIRE(b, "qie_batch_dims: null batch");
    if (batch) *batch = b->B;
    if (max_ctx) *max_ctx = b->max_ctx;
    return 0;
}

int qie_batch_kv_cache(const qie_batch* b, int32_t seq, qie_kv_cache* out) {
    QIE_REQUIRE(b && out && seq >= 0 && seq < b->B, "qie_batch_kv_cache: bad arguments");
    *out = batch_cache(b, seq);
    return 0;
}

int qie_engine_arena(const qie_engine* e, void** base, int64_t* bytes) {
    QIE_REQUIRE(e && e->have_weights, "qie_engine_arena: engine has no weights");
    if (base) *base = e->arena;
    if (bytes) *bytes = (int64_t)e->arena_bytes;
    return 0;
}

int qie_engine_rope_tables(const qie_engine* e, const float** rope_cos, const float** rope_sin, int32_t* rows) {
    QIE_REQUIRE(e, "qie_engine_rope_tables: null engine");
    if (rope_cos) *rope_cos = e->rope_cos;
    if (rope_sin) *rope_sin = e->rope_sin;
    if (rows) *rows = e->rope_rows;
    return 0;
}

// Live per-kernel timing (bench.py's roofline line).  The launches cycle through layers
// 1 .. L-1 (layer 0 where L == 1), as the decode step does: replaying ONE layer's weights
// back to back would leave a ~272 MB gate/up working set largely in the 256 MiB Infinity
// Cache and time a cache hit rate no decode step sees (round-1 verdict).  lm_head (which 4)
// has one weight; its 1.09 GB stream cannot stay resident.
// which == 6: the persistent layer stack (k_persist.hip) alone, `iters` back-to-back launches at
// the current position.  Each launch gets its own hand-off epoch (a device array of fresh
// values, so no kernel runs between the timed launches); the residual row is restored and the
// real epoch advanced past them afterwards, and the KV rows the launches wrote at the current
// position are rewritten by the next real step.  Bytes: every layer weight read once plus the
// K / V rows the attention reads.
// `warm` untimed launches run(0 ..), then `iters` timed ones run(0 ..) between two events on the
// stream: the mean per launch.  The events are destroyed on every path.
static int time_launches(hipStream_t st, const std::function<int(int)>& run, int warm, int iters, double* avg_us) {
    struct Event {
        hipEvent_t ev = nullptr;
        ~Event() {
            if (ev) hipEventDestroy(ev);
        }
    } t0, t1;
    QIE_HIP(hipEventCreate(&t0.ev));
    QIE_HIP(hipEventCreate(&t1.ev));
    for (int i = 0; i < warm; i++) QIE_TRY(run(i));
    QIE_HIP(hipEventRecord(t0.ev, st));
    for (int i = 0; i < iters; i++) QIE_TRY(run(i));
    QIE_HIP(hipEventRecord(t1.ev, st));
    QIE_HIP(hipEventSynchronize(t1.ev));
    float ms = 0;
    QIE_HIP(hipEventElapsedTime(&ms, t0.ev, t1.ev));
    *avg_us = ms * 1000.0 / iters;
    return 0;
}

static int time_persistent(qie_batch* b, int iters, double* avg_us, double* bytes) {
    qie_engine* e = b->e;
    const qie_model_spec& s = e->spec;
    QIE_REQUIRE(b->decode_mode == 1 && b->pk_mem, "qie_batch_time_kernel: which 6 needs decode mode 1");
    const int64_t H = s.hidden, hd = s.head_dim, QD = (int64_t)s.n_heads * hd, KD = (int64_t)s.n_kv_heads * hd,
                  I = s.ffn;
    int32_t pos = 0;
    unsigned ep = 0;
    QIE_HIP(d2h(e, &pos, b->dec.pos, 4));
    QIE_HIP(d2h(e, &ep, pk_epoch_ptr(b), 4));
    const int n = iters + 4;
    std::vector<unsigned> eps(n);
    for (int i = 0; i < n; i++) eps[i] = ep + 1 + (unsigned)i;
    DevBlock eps_mem, xsave;
    QIE_TRY(eps_mem.grow((size_t)n * 4));
    QIE_TRY(xsave.grow((size_t)H * 2));
    const unsigned* d_eps = (const unsigned*)eps_mem.p;
    QIE_HIP(hipMemcpyAsync(eps_mem.p, eps.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    QIE_HIP(hipMemcpyAsync(xsave.p, b->dec.x, H * 2, hipMemcpyDeviceToDevice, e->stream));
    // launches back to back on the same input: x_res is only read at layer 0 and written at the
    // last layer, so each launch sees a row of the same magnitude (restored afterwards); every
    // launch, warm-up included, takes the next fresh epoch
    int k = 0;
    auto run = [&](int) {
        return persist_decode_launch(s, b->d_layers, b->d_attp, b->dec.x, (unsigned long long*)b->pk_mem, d_eps + k++,
                                     pk_epoch_ptr(b) + 1, b->dec.pos, pk_splits_target(b), nullptr, e->stream);
    };
    QIE_TRY(time_launches(e->stream, run, 4, iters, avg_us));
    const unsigned ep_after = ep + (unsigned)n + 1;
    QIE_HIP(hipMemcpyAsync(b->dec.x, xsave.p, H * 2, hipMemcpyDeviceToDevice, e->stream));
    QIE_HIP(hipMemcpyAsync(pk_epoch_ptr(b), &ep_after, 4, hipMemcpyHostToDevice, e->stream));
    QIE_HIP(hipStreamSynchronize(e->stream));
    QIE_TRY(pk_check(b));
    const double per_layer = (double)(QD + 2 * KD) * H * 2 + (double)(QD + 2 * KD) * 2 * (s.qkv_bias ? 1 : 0) +
                             (double)H * QD * 2 + 2.0 * I * H * 2 + (double)H * I * 2 + 2.0 * H * 2 +
                             (double)(pos + 1) * KD * 2 * 2;
    *bytes = per_layer * s.n_layers;
    return 0;
}

int qie_batch_time_kernel(qie_batch* b, int32_t which, int32_t iters, double* avg_us, double* bytes) {
    QIE_REQUIRE(b && iters > 0 && avg_us && bytes && which >= 0 && which <= 6, "qie_batch_time_kernel: bad arguments");
    qie_engine* e = b->e;
    if (which == 6) return time_persistent(b, iters, avg_us, bytes);
    const qie_model_spec& s = e->spec;
    const TpShard& sh = e->sh;   // this rank's shard sizes
    const int64_t H = s.hidden, hd = s.head_dim, QD = (int64_t)sh.nq * hd, KD = (int64_t)sh.nkv * hd;
    const int64_t I = sh.ffn, B = b->B, V = sh.vocab;
    // scratch output so timing never disturbs the sequence state
    DevBlock scratch_mem;
    QIE_TRY(scratch_mem.grow((size_t)B * std::max<int64_t>(std::max(I, V), QD + 2 * KD) * 2 + B * 8 + 64));
    uint16_t* scratch = (uint16_t*)scratch_mem.p;
    const double wb = e->fp8 ? 1.0 : 2.0;   // weight bytes per element (fp8 row scales: negligible)
    // the layer projections' (fp4: a code nibble + one e8m0 byte per 32 elements)
    const double pb = e->fp4 ? 0.5 + 1.0 / 32 : wb;
    double by = 0;
    switch (which) {
        case 0: by = 2.0 * I * H * pb + B * H * 2 + H * 2 + B * I * 2; break;
        case 1: by = (double)H * I * pb + B * I * 2 + B * H * 2; break;
        case 2: by = (double)(QD + 2 * KD) * H * pb + B * H * 2 + B * (QD + 2 * KD) * 2; break;
        case 3: by = (double)H * QD * pb + B * QD * 2 + B * H * 2; break;
        case 4: by = (double)V * H * wb + B * H * 2 + B * (double)V * 2; break;
        default: {
            std::vector<int32_t> pos(B);
            QIE_HIP(d2h(e, pos.data(), b->dec.pos, B * 4));
            for (int m = 0; m < B; m++) by += (double)(pos[m] + 1) * KD * 2 * 2;
            by += (double)B * QD * 2 * 2;
        }
    }
    // the step's own rows and launches (the builders, prenorm()'s decision, the step's extras),
    // with every output in scratch: gate/up and QKV through their rows, O and down as plain
    // stores (the residual stream stays untouched), the head with its arg-max keys behind its logits
    LayerRows r = layer_rows(b->dec, b->B, 1);
    if (which == 0) r.h = scratch;
    if (which == 2) r.qkv = scratch;
    HeadBufs hb = head_bufs(b->dec, 0, b->e->sh.vocab);
    hb.logits = scratch;
    hb.keys = (unsigned long long*)(((uintptr_t)(scratch + B * V) + 7) & ~(uintptr_t)7);
    const LayerPath p = decode_path(e);
    const int nl = s.n_layers;
    auto run = [&](int i) -> int {
        const int l = which == 4 || nl == 1 ? 0 : 1 + i % (nl - 1);
        if (which == 5) return attend_decode(b, l, scratch);
        const qie_layer_weights& L = p.layers[l];
        qie_linear_args a = which == 0   ? gate_up_args(e, L, p.flags, r)
                            : which == 1 ? down_args(e, L, p.flags, r)
                            : which == 2 ? qkv_args(e, L, p.flags, r)
                            : which == 3 ? o_args(e, L, p.flags, r)
                                         : head_args(e, b->dec.x, H, (int)B, true, hb);
        if (which == 1 || which == 3) {
            a.y = scratch;
            a.epilogue = QIE_EPI_STORE;
        }
        if (prenorm_applies(a)) take_normed(a, b->dec.xn);   // rows normed by the step's own prenorm(): no norm launch here
        return linear(&a, which == 2 ? decode_qkv_extras(b) : LinearExtras{}, e->stream);
    };
    QIE_TRY(time_launches(e->stream, run, std::min(nl, 4), iters, avg_us));
    *bytes = by;
    return 0;
}

int qie_batch_debug_step(qie_batch* b, const qie_sampling* smp, int32_t* next_ids, void* host_x) {
    QIE_REQUIRE(b && host_x, "qie_batch_debug_step: bad arguments");
    qie_engine* e = b->e;
    const int64_t n = (int64_t)b->B * e->spec.hidden, slots = 2 * (int64_t)e->spec.n_layers + 1;
    QIE_TRY(prepare_steps(b, 1, "qie_batch_debug_step"));
    QIE_TRY(dmalloc((void**)&b->dbg_x, (size_t)(slots * n * 2)));
    int rc = dbg_snap(b, 0);
    if (!rc) rc = enqueue_decode(b, smp);   // eager: the graph (if any) is left as it is
    hipError_t he = hipStreamSynchronize(e->stream);
    if (!rc && he == hipSuccess) he = d2h(e, host_x, b->dbg_x, (size_t)(slots * n * 2));
    hipFree(b->dbg_x);
    b->dbg_x = nullptr;
    QIE_TRY(rc);
    QIE_HIP(he);
    for (int m = 0; m < b->B; m++) b->h_pos[m] += 1;
    return sync_ids(b, next_ids);
}

int qie_linear(const qie_linear_args* a, void* stream) { return linear(a, LinearExtras{}, (hipStream_t)stream); }

int qie_debug_linear_plan(const qie_linear_args* a, char* out, int cap) { return linear_plan_text(a, out, cap); }

}  // extern "C"
