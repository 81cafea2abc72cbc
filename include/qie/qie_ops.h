/*
 * qie_ops.h — operator-level C ABI of libqie.so (MI355X / gfx950 HIP kernels).
 *
 * This replaces the reference's operator API, layers/include/helpers.cuh:45-166
 * (launch_rms, launch_rope, launch_rope_single, launch_qknorm, launch_matmul,
 * proj, launch_attn, launch_act, launch_elem, launch_resadd, sample_topk_bf16,
 * copy_last_vocab_vec, copy_first_token) and the __global__ prototypes of
 * layers/include/layers_include.cuh:15-35.
 *
 * Conventions (differences from the reference are deliberate):
 *   - every pointer is a caller-owned DEVICE pointer unless stated; tensors are
 *     bf16 (uint16_t words), row-major, linear weights in PyTorch [out, in];
 *   - every op takes an explicit hipStream_t (passed as void*; NULL = the
 *     legacy default stream the reference uses) and never synchronises, never
 *     allocates — so every op can be captured into a hipGraph;
 *   - every op returns 0 on success, a positive hipError_t, or a negative QIE
 *     error (-22 = invalid argument); qie_last_error() returns the text.
 *     (The reference returns void and prints to stderr.)
 */
#ifndef QIE_OPS_H
#define QIE_OPS_H

#include "qie_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QIE_ABI_VERSION 1

const char* qie_last_error(void);
int qie_abi_version(void);
int qie_device_count(int* count);

/* Device memory plumbing for hosts without their own HIP runtime (ctypes tests,
 * FFI bindings).  A process should use ONE HIP runtime: PyTorch wheels ship their
 * own, so Python callers allocate through these rather than torch.cuda. */
int qie_set_device(int device);
int qie_malloc(void** ptr, int64_t bytes);
int qie_free(void* ptr);
int qie_memcpy_h2d(void* dst, const void* src, int64_t bytes);
int qie_memcpy_d2h(void* dst, const void* src, int64_t bytes);
int qie_memset(void* ptr, int value, int64_t bytes);
int qie_synchronize(void);
/* a non-blocking stream of the current device (ops take it as `void* stream`) */
int qie_stream_create(void** stream_out);
int qie_stream_synchronize(void* stream);
int qie_stream_destroy(void* stream);

/* ---------------------------------------------------------------- tables
 * Replaces precompute_cos_sin (layers/src/include.cpp:5-16, called at
 * utills.cu:36-44).  Fills HOST fp32 tables [n_pos][head_dim/2]: the
 * reference's exact table in REF mode, HF's bf16-rounded table in HF mode. */
int qie_rope_table_host(float* cos_out, float* sin_out, int32_t n_pos, int32_t head_dim,
                        float theta, int32_t numerics);

/* ------------------------------------------------------------- embedding
 * Replaces embedding_matrix_func (layers/src/embedded_matrix.cu:5-17, launched
 * utills.cu:51-54 and qwen_main.cu:267).  out[t,:] = E[ids[t],:]. */
int qie_embedding(const void* E, const int32_t* ids, void* out, int64_t n, int64_t H,
                  void* stream);

/* ---------------------------------------------------------------- RMSNorm
 * Replaces launch_rms / rmsNorm (helpers.cuh:45-49, normalization.cu:5-25).
 * y = rmsnorm(x) * w over rows of H; x and y may not alias. */
int qie_rmsnorm(const void* x, const void* w, void* y, int64_t rows, int64_t H, float eps,
                int32_t numerics, void* stream);

/* ----------------------------------------------------------------- linear
 * Replaces launch_matmul / proj (helpers.cuh:81-106, 132-138; matrix_mul.cu:
 * 165-288) with fused epilogues.  y[m, n] = sum_k x[m, k] * W[n, k], fp32
 * accumulation, one bf16 rounding.  W is up to three [rows_i, K] segments
 * concatenated along N (fused QKV without repacking the weights.bin arena).
 * M <= 8 runs the bandwidth-bound GEMV kernel; larger M the MFMA GEMM.
 */
enum {
    QIE_EPI_STORE = 0,     /* y = bf16(acc [+ bias])                                  */
    QIE_EPI_RESIDUAL = 1,  /* y = bf16(y + bf16(acc))   (launch_resadd fused)          */
    QIE_EPI_SWIGLU = 2,    /* segs (gate, up): y[m, j] = bf16(bf16(up) * bf16(silu(bf16(gate))))
                              (SiLU.cu:10-23 + element_add.cu:4-12 fused); N = I      */
    QIE_EPI_F32 = 3        /* y is float [M, N]: y = acc, unrounded (tensor-parallel
                              partial sums, reduced across ranks before the rounding) */
};

typedef struct qie_linear_args {
    const void* x;          /* [M, K] bf16, row stride ldx (elements)                   */
    int64_t ldx;
    const void* w[3];       /* weight segments, each [seg_rows[i], K]                   */
    const void* bias[3];    /* optional per-segment bias [seg_rows[i]] (Qwen2 q/k/v)    */
    int64_t seg_rows[3];
    int64_t M, K, N;        /* N = output columns (sum of seg_rows; I for SWIGLU)       */
    void* y;                /* [M, N] bf16, row stride ldy                              */
    int64_t ldy;
    int32_t epilogue;       /* QIE_EPI_*                                                */
    int32_t numerics;       /* for the fused norm                                       */
    const void* norm_w;     /* optional fused RMSNorm of x (weight [K]); GEMV path only */
    float norm_eps;
    int32_t flags;          /* QIE_LINEAR_FP8 / QIE_LINEAR_FP4: w[i] are fp8 / MXFP4 weights
                               (see below); else 0                                      */
    uint64_t* argmax_keys;  /* optional [M] selection keys, atomically max-merged
                               (fused greedy arg-max, logit_decode.cu:15-33); caller
                               zeroes them before the launch                            */
    int64_t key_col0;       /* global index of output column 0 in the keys (vocab-
                               parallel lm_head shard offset; 0 otherwise)              */
    const uint8_t* x_exps;  /* QIE_LINEAR_ACT_FP8: [M] e8m0 row exponents of x (below)  */
} qie_linear_args;

int qie_linear(const qie_linear_args* args, void* stream);
/* Test probe: the launch qie_linear would make of *args on the current device (its CU count,
 * this library's knobs), as one line of text: the kernel instantiation, then its grid
 * ("grid=?" where that depends on an occupancy query).  Launches nothing.  out holds cap
 * bytes; -22 if the line does not fit. */
int qie_debug_linear_plan(const qie_linear_args* args, char* out, int cap);

/* --------------------------------------------- q/k post-projection + KV append
 * Replaces launch_qknorm (helpers.cuh:140-142, qk_norm.cu:43-79), launch_rope /
 * launch_rope_single (helpers.cuh:51-55, 143-147; RoPE.cu:6-22) and
 * kv_copy_layer_to_cache_prefill/decode (include_cuda.cu:165-279) in one pass:
 *   qkv rows [M, (nq + 2*nkv)*hd] (projection output, bias already added)
 *   -> q_out [M, nq*hd] (qk-norm'd, rotated)
 *   -> K cache row (qk-norm'd, rotated) and V cache row at position pos[m].
 * KV cache layout (qie), two forms:
 *   contiguous (block_table == NULL): per sequence [L][nkv][max_ctx][hd] bf16,
 *     sequence s at k + s*seq_stride;
 *   paged (block_table != NULL): a pool of pages of page_tokens tokens (a power
 *     of two, multiple of 128), page p at k + p*seq_stride holding
 *     [L][nkv][page_tokens][hd]; token t of sequence s lives in page
 *     block_table[s*max_pages + t/page_tokens] at row t % page_tokens.
 * Row m belongs to sequence m / rows_per_seq.
 * (The reference's pages are [4 tok][L][kvdim] nodes of a linked list in managed
 * memory, iengine.cu:73-109, walked by include_cuda.cu:165-279; qie replaces the
 * list with a device block table and keeps each (layer, kv head) run of a page
 * contiguous, so a 128-key attention step streams one run of one page.) */
typedef struct qie_kv_cache {
    void* k;                 /* contiguous: sequence 0's K cache; paged: page 0       */
    void* v;
    int64_t seq_stride;      /* elements between sequences (contiguous) / pages (paged) */
    int32_t n_layers, n_kv_heads, head_dim, max_ctx;
    const int32_t* block_table;   /* device [n_seq][max_pages] page ids, or NULL       */
    int32_t page_tokens;          /* paged only                                         */
    int32_t max_pages;            /* paged only: block_table row stride                 */
} qie_kv_cache;

int qie_qkv_post(const void* qkv, int64_t M, const int32_t* pos, int32_t rows_per_seq,
                 const void* q_norm, const void* k_norm, const float* rope_cos,
                 const float* rope_sin, int32_t n_heads, const qie_kv_cache* cache,
                 int32_t layer, float eps, int32_t numerics, void* q_out, void* stream);

/* Ragged rows: M rows that are up to QIE_RAGGED_MAX_SEGS segments of any lengths laid end to
 * end, each segment the rows of one cache sequence.  The table is host memory and is copied by
 * value into the kernel arguments: no device table, no allocation, no synchronisation. */
#define QIE_RAGGED_MAX_SEGS 8
typedef struct qie_row_segs {
    int32_t n;                                   /* 1 .. QIE_RAGGED_MAX_SEGS segments              */
    int32_t row0[QIE_RAGGED_MAX_SEGS + 1];       /* rows of segment z: [row0[z], row0[z+1]);
                                                    row0[0] = 0, strictly increasing, row0[n] = M  */
    int32_t seq[QIE_RAGGED_MAX_SEGS];            /* the cache's sequence index of segment z; distinct */
} qie_row_segs;

/* qie_qkv_post with row m's sequence = segs->seq[z] of the segment z that holds it; the per-row
 * arithmetic is qie_qkv_post's.  -22 for a malformed table (n out of range, row0 not strictly
 * increasing from 0 to M, a repeated seq), nothing written. */
int qie_qkv_post_ragged(const void* qkv, int64_t M, const int32_t* pos, const qie_row_segs* segs,
                        const void* q_norm, const void* k_norm, const float* rope_cos,
                        const float* rope_sin, int32_t n_heads, const qie_kv_cache* cache,
                        int32_t layer, float eps, int32_t numerics, void* q_out, void* stream);

/* -------------------------------------------------------------- attention
 * Replaces launch_attn / selfattention (helpers.cuh:121-130,
 * self_attension.cu:10-149): GQA attention of query rows over the cache.
 * Row m attends to positions [0, pos[m]] of sequence m / rows_per_seq
 * (prefill: causal; decode: the whole cache incl. the new token — identical
 * to the reference's causal / mkv = seq_len windows).  Flash-decoding split
 * over the sequence; ws must hold qie_attention_workspace_bytes(). */
int64_t qie_attention_workspace_bytes(int64_t M, int32_t n_heads, int32_t head_dim,
                                      int32_t max_ctx);
int qie_attention(const void* q, int64_t M, const int32_t* pos, int32_t rows_per_seq,
                  const qie_kv_cache* cache, int32_t layer, int32_t n_heads, void* out,
                  void* ws, void* stream);

/* qie_attention's contract (row m attends to [0, pos[m]] of sequence m / rows_per_seq,
 * positions non-decreasing within a sequence, the rows' own K/V already in the cache) for
 * a block of new rows over a long cached prefix: an MFMA kernel with one workgroup per
 * (sequence, kv head, key split, block of 128 flattened (token, head-in-group) rows), so
 * K/V bytes are read once per (kv head, split, row block); fp32 partials in ws, merged by
 * a second launch (none, and no ws, when the cache has a single split).  head_dim 64 or
 * 128, any rows_per_seq >= 1, contiguous and paged caches; never synchronises or allocates.
 * ws must hold qie_attention_extend_workspace_bytes() and need not be initialised.
 * qie_attention_extend_split_tokens: the keys per split (a multiple of 64) of a call of M
 * rows on a cache of max_ctx keys. */
int64_t qie_attention_extend_workspace_bytes(int64_t M, int32_t n_heads, int32_t head_dim,
                                             int32_t max_ctx);
int32_t qie_attention_extend_split_tokens(int64_t M, int32_t max_ctx);
int qie_attention_extend(const void* q, int64_t M, const int32_t* pos, int32_t rows_per_seq,
                         const qie_kv_cache* cache, int32_t layer, int32_t n_heads, void* out,
                         void* ws, void* stream);

/* qie_attention_extend over ragged rows (qie_row_segs above; M = segs->row0[segs->n]): row m
 * attends to [0, pos[m]] of sequence segs->seq[z] of its segment, positions non-decreasing
 * within a segment, the rows' own K/V already in the cache; head_dim 64 or 128, contiguous and
 * paged caches, ws need not be initialised.  One workgroup per (block of 128 flattened rows of
 * one segment, key split, kv head): grid x is the sum of the segments' block counts, so a short
 * segment beside a long one launches no empty block.  The split length and the workspace are
 * qie_attention_extend_split_tokens(M, max_ctx) and qie_attention_extend_workspace_bytes(M, ..)
 * at the total row count M; inside a segment the rows are packed as the extend kernel packs a
 * sequence's, so a segment's result equals, bit for bit, that of qie_attention_extend on those
 * rows alone whenever the two calls use the same split length.  -22 for a malformed table, a
 * bad head shape or layer, or more workgroups than a grid holds; nothing is launched. */
int qie_attention_ragged(const void* q, const int32_t* pos, const qie_row_segs* segs,
                         const qie_kv_cache* cache, int32_t layer, int32_t n_heads, void* out,
                         void* ws, void* stream);

/* Decode attention with the q/k post-projection fused in (one launch per layer):
 * qkv rows [B][(nq + 2 nkv) hd] straight from the QKV projection; applies qk-norm
 * (q_norm/k_norm non-NULL) and RoPE at pos[m] to q and to the new k, appends the
 * new K/V row of sequence m at pos[m], and attends over [0, pos[m]].  Splits of 128
 * keys are combined in-launch by the last-arriving workgroup.  ws must hold
 * qie_attention_decode_workspace_bytes() and be ZEROED once before first use (it
 * is left zeroed by every call).
 * numerics may carry QIE_ATTN_PREROPED (REF numerics, no qk-norm only): q and the new
 * k in qkv are already rotated (the engine's decode QKV projection applies RoPE in its
 * epilogue), so only the K/V append and the attention run here. */
#define QIE_NUMERICS_MASK 0xff
#define QIE_ATTN_PREROPED 0x100
int64_t qie_attention_decode_workspace_bytes(int64_t B, int32_t n_heads, int32_t n_kv_heads,
                                             int32_t head_dim, int32_t max_ctx);
int qie_attention_decode(const void* qkv, int64_t B, const int32_t* pos, const void* q_norm,
                         const void* k_norm, const float* rope_cos, const float* rope_sin,
                         int32_t n_heads, const qie_kv_cache* cache, int32_t layer, float eps,
                         int32_t numerics, void* out, void* ws, void* stream);

/* Diagnostics: one wave, lane l reads 8 bytes at element 4*l of an LDS array whose
 * element i holds i, through ds_read_b64_tr_b16; out_dev[l*4 + e] receives element e
 * of lane l (pins the transposed-read lane mapping the prefill attention relies on). */
int qie_debug_tr16_probe(int32_t* out_dev);

/* ------------------------------------------- standalone in-place head ops
 * The operator tier of a host that keeps the reference's layer loop
 * (qwen_main.cu:77-241); the engine itself fuses these into qie_qkv_post /
 * qie_attention_decode.  Rows [rows][row_stride] of n_heads heads of head_dim.
 *   qie_qknorm: launch_qknorm / qkNorm (helpers.cuh:140-142, qk_norm.cu:43-79),
 *     in place, the reference's tree summation order (REF); HF = transformers.
 *   qie_rope:   launch_rope / launch_rope_single (helpers.cuh:51-55, 143-147;
 *     RoPE.cu:6-22), in place; row r at position pos[r] (device, may be NULL)
 *     or pos0 + r.  Tables as built by qie_rope_table_host.
 *   qie_kv_write: kv_copy_layer_to_cache_prefill / _decode (include_cuda.cu:
 *     165-279): K and V rows [rows][ld] (n_kv_heads*head_dim used) into layer
 *     `layer` of sequence `seq` at positions pos0 .. pos0+rows-1.  Paged caches
 *     need those pages held (qie_batch_reserve). */
int qie_qknorm(void* x, int64_t rows, int64_t row_stride, int32_t n_heads, int32_t head_dim,
               const void* w, float eps, int32_t numerics, void* stream);
int qie_rope(void* x, int64_t rows, int64_t row_stride, int32_t n_heads, int32_t head_dim,
             const int32_t* pos, int32_t pos0, const float* rope_cos, const float* rope_sin,
             int32_t numerics, void* stream);
int qie_kv_write(const void* k, const void* v, int64_t rows, int64_t ld, int32_t pos0,
                 const qie_kv_cache* cache, int32_t seq, int32_t layer, void* stream);
/* The K and V rows of positions [pos0, pos0 + n_rows), every layer and kv head, from sequence
 * src_seq of `src` to the same positions of sequence dst_seq of `dst`, in one launch (k_kvcopy.hip;
 * the reference's sequences never share or copy rows).  Both caches contiguous or both paged (a
 * mixed pair: -22), equal in n_layers, n_kv_heads, head_dim and page_tokens; a paged copy walks
 * both block tables and writes only into the pages dst's table names for those positions, which
 * the caller holds.  n_rows == 0 returns 0 without a launch; the same sequence of the same cache
 * and positions past either max_ctx return -22.  Never allocates or synchronises; capturable. */
int qie_kv_copy(const qie_kv_cache* src, int32_t src_seq, const qie_kv_cache* dst, int32_t dst_seq,
                int32_t pos0, int32_t n_rows, void* stream);

/* ------------------------------------------------------------- elementwise
 * launch_act + launch_elem (helpers.cuh:108-115) and launch_resadd (:116-119)
 * for callers that do not use the fused linear epilogues: qie_silu_mul fuses the
 * two; qie_silu (activation, SiLU.cu:10-23, in place: x = bf16(x*sigmoid(x))) and
 * qie_mul (element_mul, element_add.cu:4-12: c = bf16(a*b)) are the separate ops.
 * qie_memcpy_d2d: copy_last_vocab_vec / copy_first_token (helpers.cuh:149-155). */
int qie_silu(void* x, int64_t n, void* stream);
int qie_mul(const void* a, const void* b, void* c, int64_t n, void* stream);
int qie_memcpy_d2d(void* dst, const void* src, int64_t bytes, void* stream);
int qie_silu_mul(const void* gate, const void* up, void* h, int64_t n, void* stream);
int qie_residual_add(void* x, const void* y, int64_t n, void* stream);
/* Tensor-parallel residual: x = bf16(x + bf16(sum)) with sum the fp32 all-reduced
 * partials of the row-parallel O / down projection (same rounding as the fused
 * QIE_EPI_RESIDUAL epilogue on one GPU). */
int qie_residual_add_f32(void* x, const float* sum, int64_t n, void* stream);

/* ---------------------------------------------------------------- sampling
 * Replaces sample_topk_bf16 / topk_temperature_softmax_sampling_kernel_bf16
 * (helpers.cuh:157-166, logit_decode.cu:149-274).  Writes the chosen id of each
 * of the M logit rows to out_ids (device).  top_k <= 1 -> greedy arg-max.
 * ws must hold qie_sample_workspace_bytes(). */
int64_t qie_sample_workspace_bytes(int64_t M, int64_t V);
int qie_sample(const void* logits, int64_t M, int64_t V, int64_t ld, const qie_sampling* s,
               const int32_t* step_dev, int32_t* out_ids, void* ws, void* stream);
/* Decode fused arg-max keys (see qie_linear_args.argmax_keys) into ids. */
int qie_keys_to_ids(const uint64_t* keys, int64_t M, int32_t* out_ids, void* stream);

/* ------------------------------------------------- per-row sampling entries
 * qie_sample_rows: every one of the M bf16 logit rows [M][ld] is processed and sampled under
 * its OWN entry of a device table (qie_slot_sampling, qie_types.h).  The
 * reference has no such path (one host-side parameter set, logit_decode.cu:149-274).
 *
 * Numerics contract.  A row l[0..V) has an entry e and a window W, a multiset of token ids with
 * c[j] the count of j in W.  The processed row l' is computed in fp32 with IEEE operations, every
 * step rounded, no FMA contraction, plain division:
 *     v = f32(l[j])
 *     if c[j] > 0:
 *         v = (v > 0) ? v / e.repetition_penalty : v * e.repetition_penalty   (skipped when == 1)
 *         t = e.frequency_penalty * (float)c[j];  t = e.presence_penalty + t;  v = v - t
 *     if j is in the bias list:  v = v + bias                                  (-inf bans j)
 *     l'[j] = bf16_rne(v)            (an element with c[j] == 0 and no bias keeps its bits)
 * Rounding back to bf16 makes everything after it what qie_sample does on a bf16 row:
 *   greedy (top_k <= 1 or !(temperature > 0)): the maximum selection key (the reference tie rule);
 *   sampled: the min(top_k, 256, V) largest keys in descending order, v_i = l'_i / T, m = max,
 *     w_i = expf(v_i - m); min_p in (0, 1]: the leading entries with w_i >= min_p stay (entry 0
 *     always); then top_p and the one XORWOW draw from seed + step exactly as qie_sample.
 * A row with no selectable element (NaN / -inf only) yields -1.
 * Window of row m: the ids at positions [lo, q] of its slot's history row, q = q_dev[m],
 *     lo = max(e.penalty_start, e.penalty_last_n > 0 ? q + 1 - e.penalty_last_n : 0, 0);
 * with a tail (tail_len_dev[m] = n > 0) the positions (q - n, q] hold tail_dev[0 .. n) instead
 * of the history's words (a verify row's drafts).  Positions at or past hist_stride are not read,
 * ids outside [0, V) are ignored, so an arbitrary history never indexes out of range.  With the
 * three penalties neutral the window is not walked.
 *
 * Row m reads table[slot0 + m * slot_stride] and history row slot0 + m * slot_stride (decode:
 * stride 1; a verify step: stride 0, one slot for all rows).  An entry with n_bias < 0 stands
 * for "none": the row runs a neutral entry with the four values of `fallback` (host; may be
 * NULL = greedy).  step_dev as in qie_sample.  ws holds qie_sample_rows_workspace_bytes(M, V)
 * bytes; V <= 64 * 4096.  No float atomics (integer LDS counts): two runs are bit-identical.
 * Neither allocates nor synchronises; graph-capturable, and every entry value is read from the
 * table at run time. */
typedef struct qie_sample_rows_args {
    const void* logits;                   /* device bf16 [M][ld] */
    int64_t M, V, ld;
    const qie_slot_sampling* table;       /* device */
    int32_t slot0, slot_stride;
    const qie_sampling* fallback;         /* host, or NULL */
    const int32_t* hist;                  /* device [slots][hist_stride] */
    int64_t hist_stride;
    const int32_t* q_dev;                 /* device [M] */
    const int32_t* tail_dev;              /* device, or NULL */
    const int32_t* tail_len_dev;          /* device [M], or NULL */
    const int32_t* step_dev;              /* device [M], or NULL */
    int32_t* out_ids;                     /* device [M] */
    void* ws;
} qie_sample_rows_args;
int64_t qie_sample_rows_workspace_bytes(int64_t M, int64_t V);
int qie_sample_rows(const qie_sample_rows_args* a, void* stream);
/* The mapped form (a batched verify step): qie_sample_rows under the same
 * numerics contract, with row m's slot and tail read from device arrays instead of the stride —
 * row m reads table[row_slot_dev[m]] and history row row_slot_dev[m], and its tail words are
 * tail_dev[tail_off_dev[m] .. + tail_len_dev[m]).  slot0 / slot_stride are not used.
 * row_slot_dev: device [M], every value a slot of the table; tail_off_dev: device [M], may be NULL
 * when tail_dev is.  Same workspace, same two launches, capturable. */
int qie_sample_rows_mapped(const qie_sample_rows_args* a, const int32_t* row_slot_dev,
                           const int32_t* tail_off_dev, void* stream);

/* ----------------------------------------------------------------- scoring
 * Per-token log-probabilities of the vocabulary head (the reference has no such path: its head,
 * qwen_main.cu:224-241, samples one token from the last row).  Numerics contract (DESIGN.md
 * §17): a row's logits are what the head defines, l[j] = bf16(fp32 acc) of x_row . W[j] in some
 * valid fp32 summation order; everything after that is fp32 arithmetic on those bf16 values,
 *     lse = m + logf(sum_j expf(l[j] - m)),  m = max_j l[j],     logprob(t) = l[t] - lse;
 * the row's greedy id is the maximum selection key (the reference tie rule of qie_sample).  No
 * float atomics: partial sums are merged in a fixed index order, so two runs are bit-identical.
 * No kernel waits on another workgroup.  Neither op allocates or synchronises.
 *
 * qie_logprob_rows: over M materialised bf16 logit rows [M][ld] (ld >= V, V < 2^24), one
 *   workgroup per row.  logprobs[m] = l[targets[m]] - lse, or 0.0f where targets[m] is -1
 *   (or outside [0, V)); ids[m] (ids_dev may be NULL) = the reference-rule arg-max.
 * qie_score_rows: the fused form for x bf16 [M, K] (already normed, row stride ldx, ldx % 8 == 0)
 *   and W bf16 [V, K], both 16-byte aligned; K % 64 == 0 and K >= 256, any M >= 1, any
 *   1 <= V < 2^24 (anything else: -22).  One workgroup per 256 x 256 tile runs the prefill GEMM's
 *   tile pipeline and reduces its rounded accumulators to one {max, sum exp} pair and one key per
 *   (column tile, row) in ws; a second launch merges the column tiles of each row in index order.
 *   Nothing of size M x V is written.  ws must hold qie_score_rows_workspace_bytes(M, V) bytes
 *   (8-byte aligned) and need not be initialised. */
int qie_logprob_rows(const void* logits, int64_t M, int64_t V, int64_t ld, const int32_t* targets_dev,
                     float* logprobs_dev, int32_t* ids_dev, void* stream);
int64_t qie_score_rows_workspace_bytes(int64_t M, int64_t V);
int qie_score_rows(const void* x, int64_t ldx, const void* W, int64_t M, int64_t K, int64_t V,
                   const int32_t* targets_dev, float* logprobs_dev, int32_t* ids_dev, void* ws, void* stream);

/* ------------------------------------------------------- synthetic weights
 * Deterministic counter-based fill used for synthetic checkpoints (no weights
 * ship in this environment): element i of tensor `tensor_id` is
 *   r = splitmix64(splitmix64(seed*0x9E3779B97F4A7C15 ^ (tensor_id << 32)) + i)
 *   u = ((int32)(r >> 40) - 2^23) * 2^-23          (exact, in [-1, 1))
 *   value = bf16(offset + u * scale)
 * bit-identical on the host (qie_synthetic_fill_host, OpenMP) and the GPU. */
uint32_t qie_tensor_id(const char* name);   /* FNV-1a 32 of the tensor name */
int qie_synthetic_fill(void* dev, int64_t n, uint32_t tensor_id, uint64_t seed, float scale,
                       float offset, void* stream);
int qie_synthetic_fill_host(void* host, int64_t n, uint32_t tensor_id, uint64_t seed,
                            float scale, float offset);
/* ------------------------------------------------------------ fp8 weights
 * A linear weight [rows, cols] in fp8 is rows*cols OCP e4m3 codes followed by rows fp32
 * power-of-two row scales (qie_fp8_weight_bytes); every dequantised value is exactly a
 * bf16.  qie_linear reads such weights when args.flags has QIE_LINEAR_FP8. */
#define QIE_LINEAR_FP8 1
/* Prefill GEMM tile override (tests / tuning; M >= 256, K % 32 == 0): the LDS-DMA kernel
 * with 256x256 (TILE256) or 256x128 (TILE128) block tiles instead of the tile-count choice. */
#define QIE_LINEAR_TILE256 2
#define QIE_LINEAR_TILE128 4
/* ... or the stream-K form of the 256x256 kernel (K % 64 == 0, K >= 256): one workgroup
 * per CU, (tile, k-tile) units in contiguous ranges, shared tiles summed in k order. */
#define QIE_LINEAR_STREAMK 8
int64_t qie_fp8_weight_bytes(int64_t rows, int64_t cols);
int qie_quantize_fp8(const void* w_bf16, int64_t rows, int64_t cols, void* out, void* stream);
int qie_quantize_fp8_host(const void* w_bf16, int64_t rows, int64_t cols, void* out);
/* The inverse, on device: rows x cols bf16 (exact — every dequantised value is a bf16).
 * The engine's fp8 prefill (M >= 256 rows) expands each weight into a scratch with it and
 * runs the bf16 LDS-DMA GEMM: at prefill sizes the GEMM is MFMA-bound and the expansion
 * (1 + 2 bytes per weight) is ~2 % of it. */
int qie_dequantize_fp8(const void* w_fp8, int64_t rows, int64_t cols, void* out_bf16, void* stream);
/* 16-row tiled fp8 layout (QIE_LINEAR_FP8_T16): the codes of rows [16t, 16t + 16) are stored
 * as K/64 consecutive 1-KiB blocks, block j holding row 16t + (l % 16), columns
 * 64j + 16(l / 16) + [0, 16) at bytes [16 l, 16 l + 16) (l = 0..63) — exactly the B fragments
 * of one 64-column unit of the batched-decode MFMA kernel, so each of its 1-KiB wave loads
 * is contiguous (8 whole 128-B lines instead of 16 rows x 64 B); the row scales follow the
 * codes as in the plain layout.  rows % 16 == 0, cols % 64 == 0.  qie_linear reads such
 * weights with args.flags QIE_LINEAR_FP8 | QIE_LINEAR_FP8_T16 (the batched-decode kernel
 * only: M <= 16 rows; the engine tiles its own decode projections, tiled weights are not
 * read by the prefill GEMMs, which take the dequantised bf16 copy). */
#define QIE_LINEAR_FP8_T16 16
/* Block-scaled fp8 ACTIVATIONS — the CDNA4 fp8 MFMA path (v_mfma_scale_f32_16x16x128_
 * f8f6f4), an explicit numerics choice (the engine's qie_engine_opts.prefill_fp8): x holds
 * e4m3 codes [M, K] with row stride ldx BYTES and x_exps their per-row e8m0 exponents, row m
 * standing for 2^(x_exps[m] - 127) * e4m3(code) (qie_quantize_rows_fp8).  The weights must be
 * fp8 (QIE_LINEAR_FP8, plain or QIE_LINEAR_FP8_T16 tiled); their power-of-two row scales are
 * the MFMA's other e8m0 operand: the kernel takes ONLY the exponent field of each fp32 row scale
 * (bits >> 23), so the scales must be positive normal powers of two -- a mantissa or a sign is
 * ignored, not applied (qie_quantize_fp8 writes nothing else; a prefill_fp8 engine checks the
 * scales it makes).  K % 128 == 0, ldx % 16 == 0, no fused norm / arg-max, any
 * M (the batched-decode row limit of the tiled layout does not apply).  Replaces the
 * reference's matrix_mul (matrix_mul.cu:165-288) for a model whose prefill activations are
 * quantised; the oracle runs the same model (or_set_act_fp8). */
#define QIE_LINEAR_ACT_FP8 32
/* Per-row activation quantisation for QIE_LINEAR_ACT_FP8: s[m] = the smallest power of two
 * with max_k |x[m, k]| / s[m] <= 448 (1 for an all-zero row; e4m3_row_scale), codes
 * q[m, k] = e4m3(x[m, k] / s[m]) rounded to nearest even (|x / s| <= 448: nothing saturates),
 * exps[m] = log2(s[m]) + 127.  x bf16 [rows, cols], row stride ldx elements; q row stride ldq
 * bytes.  cols % 8 == 0, ldx % 8 == 0, ldq % 16 == 0. */
int qie_quantize_rows_fp8(const void* x, int64_t ldx, int64_t rows, int64_t cols, void* q, int64_t ldq,
                          void* exps, void* stream);
int qie_fp8_tile16(const void* w_fp8, int64_t rows, int64_t cols, void* out, void* stream);
/* Test probe: out_dev[i] = the device decode of e4m3 code i (i < 256). */
int qie_debug_fp8_decode(float* out_dev);
/* Test probe: out_dev[i] = the bf16 bits the fp8 MFMA GEMV decodes e4m3 code i to (i < 256). */
int qie_debug_fp8_decode_bf16(uint16_t* out_dev);

/* ---------------------------------------------------------- MXFP4 weights
 * A linear weight [rows, cols] (cols % 32 == 0) in MXFP4 (OCP microscaling: e2m1 codes in
 * 32-element blocks along a row, one e8m0 scale per block), plain layout:
 *   rows * cols / 2 code bytes: byte b of a row holds column 2b in its low nibble and column
 *     2b + 1 in its high nibble; a code is a sign bit (8) + the index of its magnitude in
 *     {0, 0.5, 1, 1.5, 2, 3, 4, 6};
 *   rows * cols / 32 e8m0 bytes follow: byte (row, j) = e stands for 2^(e - 127), the scale of
 *     columns [32 j, 32 j + 32) of that row.
 * qie_fp4_weight_bytes = rows * cols / 2 + rows * cols / 32.
 * Quantiser (qie_quantize_fp4 on device, qie_quantize_fp4_host; bit-identical), per block:
 *   s = the smallest power of two with max|w| / s <= 6, clamped to [2^-125, 2^125], 1 for an
 *   all-zero block; code = w / s rounded to the nearest grid value, ties to the even code index
 *   (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); a magnitude that rounds
 *   to 0 gets code 0 (no negative zero).  The lower clamp makes every non-zero dequantised value a
 *   normal bf16.  The upper clamp makes finite input give finite output: 6 * 2^125 = 1.5 * 2^127 is
 *   the largest code x scale that is a finite bf16, so a block whose maximum lies above it (the
 *   top 0.4 octave of bf16, up to the largest finite value) keeps s = 2^125 and its elements
 *   beyond 6 s take code 6 -- the one case in which the quantiser saturates (at s = 2^126 the
 *   nearest code of such a maximum would be 4 x 2^126 = inf).  Everywhere else nothing saturates.
 * Every code x 2^k is exactly a bf16, so qie_dequantize_fp4 (bf16 [rows, cols] out) is exact and
 * an fp4 engine computes the products of the bf16 model whose weights are those values.
 *
 * qie_linear reads such weights with args.flags QIE_LINEAR_FP4, through ONE kernel
 * (k_decode_fp4.hip): 1 <= M <= 16 rows, K % 128 == 0, N <= 32,768, segments of whole 16-column
 * tiles; K <= 8,192 with every epilogue and a fused norm, longer K (up to 32,768) by split-K:
 * one segment, no norm, no SWIGLU.  Anything else — M > 16, another K, a combination with
 * QIE_LINEAR_FP8 / _FP8_T16 / _ACT_FP8 — returns -22: there is no other fp4 kernel to fall back
 * to.  A split-K launch needs a per-stream workspace that cannot be allocated during a graph
 * capture: the first such launch of a stream (or qie_batch_create of an fp4 engine) makes it.
 * Numerics: products of the bf16 activations and the exactly dequantised bf16 weights, summed
 * in fp32 in one fixed order (per wave over its K slice, 128-column unit by unit, four 32-product
 * MFMA steps per unit; then the slices in wave order, split parts in part order); no float
 * atomics; two runs are bit-identical and row m does not depend on M.
 *
 * 16-row tiled layout (QIE_LINEAR_FP4 | QIE_LINEAR_FP4_T16; qie_fp4_tile16; rows % 16 == 0,
 * cols % 128 == 0): the codes of rows [16t, 16t + 16) x columns [128j, 128j + 128) form the
 * 1-KiB block t * (cols / 128) + j; bytes [16 l, 16 l + 16) of a block (l = 0..63) are row
 * 16t + l % 16, columns 128j + 32 (l / 16) + [0, 32): one whole MX block per lane per 16-B load.
 * The scales follow all code blocks, tiled the same way: 64 bytes per (t, j), byte l = the scale
 * of that lane's MX block — one contiguous 64-B read per wave load.  Same total size. */
#define QIE_LINEAR_FP4 64
#define QIE_LINEAR_FP4_T16 128
int64_t qie_fp4_weight_bytes(int64_t rows, int64_t cols);
int qie_quantize_fp4(const void* w_bf16, int64_t rows, int64_t cols, void* out, void* stream);
int qie_quantize_fp4_host(const void* w_bf16, int64_t rows, int64_t cols, void* out);
int qie_dequantize_fp4(const void* w_fp4, int64_t rows, int64_t cols, void* out_bf16, void* stream);
int qie_fp4_tile16(const void* w_fp4, int64_t rows, int64_t cols, void* out, void* stream);
/* Test probe: out_dev[16 i + c] = the bf16 bits the fp4 kernel's conversion gives code c
 * (c < 16) under the e8m0 exponent exps[i] (host, 1 <= n_exps <= 16).  Synchronises. */
int qie_debug_fp4_decode_bf16(const uint8_t* exps, int32_t n_exps, uint16_t* out_dev);

/* Tensor-parallel shard of the same synthetic tensor: dev[i][j] = element
 * (row0 + i) * full_cols + col0 + j of the full tensor, rows x cols, row-major. */
int qie_synthetic_fill_slice(void* dev, int64_t rows, int64_t cols, int64_t full_cols, int64_t row0,
                             int64_t col0, uint32_t tensor_id, uint64_t seed, float scale, float offset,
                             void* stream);
/* Rows r of a bf16 [rows, cols] matrix with (row0 + r) % every == 0 multiplied by 2^log2f
 * in place (exact while finite).  Used to give a synthetic lm_head a peaked, trained-model-
 * like top-1 margin for the end-to-end greedy parity runs (tests/parity.py, bench.py). */
int qie_scale_rows_pow2(void* w, int64_t rows, int64_t cols, int64_t row0, int64_t every, int32_t log2f,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QIE_OPS_H */
