/*
 * qie_engine.h — engine-level C ABI of libqie.so: weights, KV cache,
 * prefill and hipGraph-captured decode.
 *
 * Replaces the reference's driver / step API:
 *   llm()                               layers/src/qwen_main.cu:64-417, iengine.cuh:51
 *       -> qie_prefill() (state == prefill) / qie_decode_step() (state == decode)
 *   create_new_sequence()               layers/src/iengine.cu:25-47
 *   initialize_model_buffers()          layers/src/utills.cu:4-129
 *   destroy_model_buffers()             layers/src/utills.cu:142-205
 *       -> qie_batch_create() / qie_batch_destroy()
 *   create_page_list / allocate_page_buffers / free_page_list
 *                                       layers/src/iengine.cu:73-109
 *       -> the KV cache owned by qie_batch (contiguous per (layer, kv head))
 *   load_all_weights_to_gpu_chunked()   layers/src/iengine.cu:117-223
 *       -> qie_engine_load_weights_bin()
 *   parsed_tensors / build_indexed_tensors (tensor_parser.cpp:31-165)
 *       -> qie_index_* (reference-compatible weights.bin index)
 *
 * All functions return 0 on success; qie_last_error() (qie_ops.h) has the text.
 */
#ifndef QIE_ENGINE_H
#define QIE_ENGINE_H

#include "qie_types.h"
#include "qie_ops.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qie_engine qie_engine;
typedef struct qie_comm qie_comm;
typedef struct qie_batch qie_batch;
typedef struct qie_index qie_index;

/* ------------------------------------------------------------------ index
 * Reference-compatible tensor index (tensor_parser.hh:204-210):
 * {tensor_name, shape, data_offsets (bytes, re-based into one contiguous
 * weights.bin), layer_index (-1 for globals), short_name}; lm_head.weight
 * has short_name "logits". */
int qie_index_load_meta(const char* meta_data_txt, qie_index** out);   /* meta_data.txt format */
int qie_index_synthetic(const qie_model_spec* spec, qie_index** out);  /* HF names, sorted, one shard */
int qie_index_count(const qie_index* idx);
int qie_index_get(const qie_index* idx, int i, const char** name, const char** short_name,
                  int32_t* layer, int64_t* off0, int64_t* off1, int32_t* ndim, int64_t* shape4);
int64_t qie_index_total_bytes(const qie_index* idx);
int qie_index_write_meta(const qie_index* idx, const char* path);
void qie_index_destroy(qie_index* idx);

/* ----------------------------------------------------------------- engine */
/* ------------------------------------------------------ tensor parallelism
 * One communicator per rank.  RCCL: rank 0 calls qie_comm_unique_id() and ships the
 * QIE_COMM_ID_BYTES bytes to every rank (any host channel), then every rank calls
 * qie_comm_create_rccl() with its device (blocks until all ranks joined).  Local:
 * qie_comm_create_local(world, out[world]) makes `world` ranks of ONE process on one
 * device, driven by one host thread each (test backend; engines on it run without
 * hipGraphs).  Pass the handle as qie_engine_opts.tp_comm; the engine then holds
 * only its shard and every collective call of a step must be made by
 * all ranks (prefill, decode, qie_batch_logits). */
#define QIE_COMM_ID_BYTES 128
int qie_comm_unique_id(void* id_out);
int qie_comm_create_rccl(const void* id, int32_t world, int32_t rank, int32_t device, qie_comm** out);
int qie_comm_create_local(int32_t world, qie_comm** out);
/* Peer backend: every rank's exchange buffer mapped into every rank, one
 * kernel per collective (push + per-block generation flags + rank-ordered reduce, the
 * residual add fused into the row-parallel all-reduce); graph-capturable.  Across
 * processes: qie_comm_create_peer() returns this rank's QIE_COMM_PEER_HANDLE_BYTES IPC
 * handle, the host ships all handles to every rank (handles[r] = rank r's), then
 * qie_comm_peer_connect().  Ranks of one process on one device (world <= 2: the
 * process's hardware queues must give every rank its own):
 * qie_comm_create_peer_local(world, out[world]).  A rank that waited ~10 s for a peer
 * sets the error word qie_comm_peer_error() reads (no kernel waits forever); it then stores
 * no result, the communicator stays poisoned (later exchanges return at once) and the
 * engine's next synchronising call fails. */
#define QIE_COMM_PEER_HANDLE_BYTES 128
int qie_comm_create_peer(int32_t world, int32_t rank, int32_t device, qie_comm** out, void* handle_out);
int qie_comm_peer_connect(qie_comm* c, const void* handles);
int qie_comm_create_peer_local(int32_t world, qie_comm** out);
int qie_comm_peer_error(const qie_comm* c, int32_t* err);
/* Peer backend exchange form, set identically on every rank between steps
 * (a captured decode graph keeps the form it was captured with): tagged = 1 sends
 * row-parallel exchanges of <= 131,072 elements as {generation tag, f32} words that the
 * readers poll directly (no flags, no system fences), 0 the flagged form; push = 1 (with
 * tagged) lets a batch-1 projection's GEMV epilogue write those words itself, so the
 * exchange kernel only waits and reduces.  Results are bit-identical in every form.
 * Defaults: env QIE_PEER_TAGGED / QIE_PEER_PUSH, else 1 / 1. */
int qie_comm_peer_set_mode(qie_comm* c, int32_t tagged, int32_t push);
/* x (bf16 [n]) = bf16(x + bf16(sum over ranks of part)), in place on x (part may be
 * overwritten): the exchange after a row-parallel projection */
int qie_comm_allreduce_residual_bf16(qie_comm* c, const float* part, void* x, int64_t n, void* stream);
/* Measurement: `count` row-parallel exchanges of n elements captured in one hipGraph on
 * `stream` and replayed `reps` times (after one warm replay); *us_out = microseconds per
 * exchange (hipEvents).  form 0: as the engine runs them (the current mode), 1: the flagged
 * form, 2: the flagged form with n = 0 (the synchronisation alone at the same grid).  Every
 * rank must call it with the same arguments. */
int qie_comm_time_exchange(qie_comm* c, const float* part, void* x, int64_t n, int32_t count, int32_t reps,
                           int32_t form, void* stream, float* us_out);
int qie_comm_rank(const qie_comm* c, int32_t* world, int32_t* rank);
int qie_comm_allreduce_sum_f32(qie_comm* c, float* buf, int64_t n, void* stream);
/* in place: element-wise max over ranks of u64 words (the greedy arg-max keys) */
int qie_comm_allreduce_max_u64(qie_comm* c, uint64_t* buf, int64_t n, void* stream);
void qie_comm_destroy(qie_comm* c);

typedef struct qie_engine_opts {
    int32_t device;          /* HIP device ordinal                                   */
    int32_t max_ctx;         /* RoPE table rows (reference CONTEXT_SIZE = 32786)     */
    int32_t use_graph;       /* 1: decode steps replay a captured hipGraph           */
    int32_t tp_rank, tp_size;/* informational; taken from tp_comm when it is set     */
    void* tp_comm;           /* qie_comm* (tensor parallel over its ranks) or NULL   */
    int32_t weight_fp8;      /* 1: linear weights + lm_head quantised to OCP e4m3 with
                                power-of-two row scales after loading (qie_ops.h)     */
    int32_t comm_always;     /* 1: run the exchange steps (row-parallel all-reduces, the
                                greedy key max, the logit gather) through tp_comm even at
                                world 1 — the captured-collective path on one GPU (tests) */
    int32_t prefill_fp8;     /* 1 (with weight_fp8): the prefill projections run on the
                                block-scaled fp8 MFMA (QIE_LINEAR_ACT_FP8) — activations
                                quantised per row to e4m3 before each projection, a
                                different model from the bf16-activation one (numerics flag) */
    int32_t weight_fp4;      /* 1: the seven layer projections quantised to MXFP4 after loading
                                (qie_ops.h: e2m1 codes, 32-element blocks, e8m0 scales).  Every
                                M <= 16 launch of a projection (decode, verify, short prefills
                                and appends) reads the codes, every larger one their exact bf16
                                dequantisation, which the engine keeps beside the codes: memory
                                GROWS by ~0.27x the bf16 projections.  lm_head, embeddings, norms
                                and biases stay bf16; with weight_fp8 the lm_head alone is fp8.
                                -22 from qie_engine_create with tensor parallelism, prefill_fp8,
                                or a hidden / q dim / ffn the MXFP4 kernel does not take; the
                                persistent decode mode refuses such an engine                  */
    int32_t reserved[4];
} qie_engine_opts;

int qie_engine_create(const qie_model_spec* spec, const qie_engine_opts* opts, qie_engine** out);
/* Synthetic checkpoint at real shapes (no weights ship here): reference-layout
 * arena (qie_index_synthetic), every tensor filled by qie_synthetic_fill with
 * tensor_id = qie_tensor_id(name): linear weights offset 0 / scale w_scale,
 * norm weights 1 + norm_scale*u, biases bias_scale*u. */
int qie_engine_init_synthetic(qie_engine* e, uint64_t seed, float w_scale, float norm_scale,
                              float bias_scale);
/* Reference flat weights.bin + meta_data.txt index, read in chunks through a
 * pinned staging buffer (load_all_weights_to_gpu_chunked semantics). */
int qie_engine_load_weights_bin(qie_engine* e, const char* weights_bin, const char* meta_data_txt,
                                int64_t chunk_bytes);
/* Caller-owned device weights (e.g. torch tensors); not freed by qie. */
int qie_engine_set_weights(qie_engine* e, const qie_model_weights* w);
int qie_engine_weights(const qie_engine* e, qie_model_weights* out, const qie_layer_weights** layers);
int qie_engine_spec(const qie_engine* e, qie_model_spec* out);
void* qie_engine_stream(qie_engine* e);
int qie_engine_sync(qie_engine* e);
void qie_engine_destroy(qie_engine* e);

/* ------------------------------------------------------------------ batch
 * B independent sequences decoded together (weights streamed once per step).
 * KV cache [B][L][nkv][max_ctx][hd] bf16; token history [B][max_ctx]. */
int qie_batch_create(qie_engine* e, int32_t batch, int32_t max_ctx, qie_batch** out);
void qie_batch_destroy(qie_batch* b);

/* Paged KV cache with a device block table.  Replaces the
 * reference's per-sequence linked page list — create_page_list /
 * allocate_page_buffers / free_page_list (iengine.cu:73-109) walked by
 * kv_copy_layer_to_cache_prefill/decode (include_cuda.cu:165-279) and the
 * batch_metadata slots (iengine.cuh:27-37).  A pool of n_pages pages of
 * page_tokens tokens (a power of two >= 128; 0 = 128) shared by the B slots;
 * n_pages 0 = enough for every slot at max_ctx.  Pages are taken on demand by
 * qie_prefill / qie_decode* / qie_batch_set_position and returned by
 * qie_batch_release; running out of pages fails the call with nothing launched and nothing
 * changed: -28 from qie_prefill_append, qie_prefill_ragged, qie_score at pos0 >= 1, qie_verify, qie_verify_batch, qie_batch_fork
 * and a qie_batch_set_position into a shared page; -22 from qie_prefill, qie_prefill_batch,
 * qie_score at pos0 = 0, qie_decode_step, qie_decode, qie_batch_reserve and a
 * qie_batch_set_position that only grows.
 * Page 0 is a scratch page that idle slots write into. */
int qie_batch_create_paged(qie_engine* e, int32_t batch, int32_t max_ctx, int32_t page_tokens,
                           int32_t n_pages, qie_batch** out);
/* Ends sequence `seq`: its pages go back to the pool (paged; a page another holder shares, see
 * "forks and prefix handles" below, stays with that holder) and the slot idles —
 * it still runs through every decode step on the scratch page, its outputs are
 * meaningless — until the next qie_prefill into it.  Any batch. */
int qie_batch_release(qie_batch* b, int32_t seq);
/* Pool state: free pages, pages per slot (host [B], may be NULL), page_tokens. */
int qie_batch_page_stats(qie_batch* b, int32_t* free_pages, int32_t* pages_per_seq, int32_t* page_tokens);
/* The n first block-table entries of `seq` (host copy); paged batches only. */
int qie_batch_block_table(qie_batch* b, int32_t seq, int32_t* host_pages, int32_t n);

/* Prefill sequence `seq` with n prompt ids (host array); writes its KV rows
 * 0..n-1, samples the first generated token (host *next_id, may be NULL) and
 * makes it the sequence's current token at position n. */
int qie_prefill(qie_batch* b, int32_t seq, const int32_t* ids, int32_t n, const qie_sampling* s,
                int32_t* next_id);
/* qie_prefill of n_seqs prompts of len ids each (host [n_seqs][len], laid end to end)
 * into slots seq0 .. seq0+n_seqs-1 in one pass: every projection GEMM runs once over
 * the n_seqs*len rows (the reference prefills one sequence per call, iengine.cu
 * prefill path; this is the batch-admission form of it).  next_ids: host [n_seqs]
 * or NULL.  Paged batches: all-or-nothing on the pool, as qie_prefill. */
int qie_prefill_batch(qie_batch* b, int32_t seq0, int32_t n_seqs, const int32_t* ids, int32_t len,
                      const qie_sampling* s, int32_t* next_ids);
/* Extends live sequence `seq`: n ids (host) at positions pos0 .. pos0+n-1, attending to the
 * cached rows [0, pos0) and to each other causally; writes their KV rows, samples the next
 * token from the last row (host *next_id, may be NULL) and makes it the current token at
 * position pos0 + n.  1 <= pos0 <= the sequence's current position: rows >= pos0 (a pending
 * current token, rows written by decode steps since) are overwritten, as with
 * qie_batch_set_position.  The sequence's pages are kept and grown.  The sampling step
 * counter restarts as after a fresh qie_prefill (the sampled token is step 0's).
 * All-or-nothing: bad arguments, an idle or released slot, pos0 above the current position
 * and pos0 + n >= max_ctx return -22, a page pool that cannot hold the new rows returns -28,
 * both before anything is launched — the sequence continues as if the call had not been
 * made.  Engines created with prefill_fp8 return -22: their block-scaled activation
 * numerics are defined for a prefill from position 0 only. */
int qie_prefill_append(qie_batch* b, int32_t seq, const int32_t* ids, int32_t n, int32_t pos0,
                       const qie_sampling* s, int32_t* next_id);
/* Ragged prefill: up to QIE_RAGGED_MAX_SEGS segments — each its own slot, length
 * and start position, fresh prompts and appends mixed — in ONE pass over the weights.  ids: host,
 * the segments' ids laid end to end.  Segment z with pos0 == 0 does to slot seq what qie_prefill
 * does (a new sequence; the pages only that slot holds go back to the pool first), with
 * pos0 >= 1 what qie_prefill_append does (a live slot, pos0 <= its position, rows from pos0 on
 * overwritten, shared pages of the write range made private first).  Every integer is exactly
 * what the sequence of single calls leaves: positions, history, the current token, the step
 * counter, pages per slot, free pages and holder counts; per-slot sampling entries are honoured;
 * row seq of qie_batch_logits holds the logits behind the segment's token, next_ids[z] (host
 * [n_segs] or NULL: then nothing is synchronised) is segment z's token.  Logits and K/V are NOT
 * bit-equal to the single calls (the GEMM kernels are picked by the total row count and the
 * attention split follows it); they meet the same oracle parity bar.  A segment's results do not
 * depend on the other segments' ids.
 * Preconditions: seq strictly increasing across segments, 1 <= n_segs <= B, n >= 1,
 * pos0 + n < max_ctx, ids in range.  All-or-nothing, before anything is launched or allocated:
 * -22 for bad arguments, an append segment on an idle or released slot, pos0 past the slot's
 * position, an engine created with prefill_fp8, and a batch in decode mode 1 with n_segs > 1;
 * -28 when the pool cannot hold every segment's rows together.  After either every slot continues
 * as if the call had not been made.  Collective under tensor parallelism, like qie_prefill. */
typedef struct qie_prefill_seg { int32_t seq, n, pos0; } qie_prefill_seg;
int qie_prefill_ragged(qie_batch* b, const qie_prefill_seg* segs, int32_t n_segs, const int32_t* ids,
                       const qie_sampling* s, int32_t* next_ids);
/* Scoring: the log-probability of a given text (numerics contract in qie_ops.h,
 * "scoring").  qie_score IS qie_prefill (pos0 == 0) or qie_prefill_append (pos0 >= 1) of the n
 * ids in every effect on the sequence — KV rows, pages, history, position, the current token, the
 * step counter, qie_batch_logits row `seq`, *next_id, the error codes and the all-or-nothing
 * rules are those of the plain call, bit for bit (the same launches run; the scoring head is
 * added after them).  In addition every row i is scored: logprobs[i] (host [n]) = the log-
 * probability the model gives targets[i] (host [n], a token id, or -1 for "none": 0.0f) as the
 * token after ids[0..i], and greedy_ids[i] (host [n], may be NULL) = the arg-max of row i's logits
 * under the reference tie rule.  A target outside [-1, V) returns -22 before anything is launched.
 * One sequence per call; the call synchronises; collective under tensor parallelism.
 * Head path: a bf16 head with hidden % 64 == 0 and hidden >= 256 on a single-rank engine runs the
 * fused qie_score_rows (no logit row is materialised); fp8 heads, engines on the exchange path
 * and flags = QIE_SCORE_UNFUSED run rows [0, n - 1) in pieces of <= 16 through the head launch of
 * decode and qie_verify (their logits, bit for bit) and qie_logprob_rows, and take row n - 1 from
 * the logits the prefill's own head wrote (qie_batch_logits row `seq`).  That path uses the verify
 * step's logit rows: qie_verify_logits afterwards needs a new qie_verify.  prefill_fp8 engines
 * score at pos0 == 0 (the head reads bf16 rows there, as it does in qie_prefill). */
#define QIE_SCORE_UNFUSED 1
int qie_score(qie_batch* b, int32_t seq, const int32_t* ids, int32_t n, int32_t pos0,
              const int32_t* targets, const qie_sampling* s, int32_t flags, float* logprobs,
              int32_t* greedy_ids, int32_t* next_id);
/* Log-probability of ids[m] (host [B]; -1 = skip: 0.0f) under the logits qie_batch_logits would
 * return for slot m: out host float [B].  Runs qie_logprob_rows on the engine's stream, outside
 * any captured graph; no [B][V] host copy.  Works wherever qie_batch_logits does (collective
 * under tensor parallelism). */
int qie_batch_logprobs(qie_batch* b, const int32_t* ids, float* out);
/* Speculative decoding: verify up to QIE_VERIFY_MAX_ROWS - 1 drafted tokens in one weight pass
 * (DESIGN.md §16).  `seq` is a live slot of any batch (contiguous or paged, any B) at position
 * p with a pending current token c; draft holds 0 <= n_draft <= 15 ids d1 .. dn (host).  One
 * pass runs the M = n_draft + 1 rows c, d1 .. dn at positions p .. p+n through the decode-form
 * layer, writes their K/V rows and picks one token t_i per row: greedy from the fused arg-max
 * keys (the reference tie rule), sampled by qie_sample with row i's counter = the sequence's
 * step counter + i — the id a plain qie_decode_step would draw from the same logits.  The
 * accepted length a is the largest a with d_j == t_(j-1) for all 1 <= j <= a; out_ids (host,
 * n_draft + 1 slots) receives t_0 .. t_a and *n_out = a + 1 >= 1.  The sequence is left exactly
 * as after a + 1 decode steps: position p + a + 1, current token t_a, history [p+1 .. p+a+1] =
 * t_0 .. t_a, step counter + (a + 1), qie_batch_logits row `seq` = the logits that produced
 * t_a.  K/V rows of rejected drafts lie at or past the new position and are overwritten before
 * anything reads them (the qie_batch_set_position rule); other slots are untouched.  The call
 * synchronises.  With use_graph the step is captured once per (slot, rows, sampling) and
 * replayed.  Collective under tensor parallelism, like qie_prefill.
 * All-or-nothing, nothing launched: -22 for bad arguments, an idle or released slot, a draft
 * id out of range, p + n_draft + 1 >= max_ctx, an engine created with prefill_fp8, a batch in
 * decode mode 1; -28 when the page pool cannot hold positions up to p + n_draft (pages taken
 * for rows that end up rejected stay with the slot until it is released). */
#define QIE_VERIFY_MAX_ROWS 16   /* the M <= 16 linear planner's range */
int qie_verify(qie_batch* b, int32_t seq, const int32_t* draft, int32_t n_draft,
               const qie_sampling* s, int32_t* out_ids, int32_t* n_out);
/* Logits of every row of the last qie_verify: host bf16 [n_draft + 1][V].  Works wherever
 * qie_batch_logits does (collective under tensor parallelism). */
int qie_verify_logits(qie_batch* b, void* host_out);
/* qie_verify for several slots in ONE weight pass.  Segment z runs the rows c_z,
 * d1 .. dn of slot seq_z (n = n_draft_z >= 0) at positions p_z .. p_z + n; row0[z], the running
 * sum of n_draft + 1, is its first row and M = row0[n_segs] <= QIE_VERIFY_MAX_ROWS.  draft: host,
 * the segments' drafts laid end to end (may be NULL when there are none).  Per segment the
 * semantics are exactly qie_verify's: the choices t_i (fused arg-max keys, or sampled with row i's
 * counter = the slot's step counter + i; a slot's sampling entry is honoured, row i seeing that
 * slot's history and that segment's d1 .. di), the accepted length a_z, and the slot left as after
 * a_z + 1 decode steps — position, current token, history, step counter, the next input row, the
 * current-position RoPE row, and qie_batch_logits row seq_z = the step's row row0[z] + a_z.
 * out_ids (host [M]) receives segment z's t_0 .. t_a at out_ids[row0[z] ..], n_out (host [n_segs])
 * a_z + 1 >= 1.  Slots that are not in the call are untouched, bit for bit: they do not advance.
 * K/V rows of rejected drafts fall under the qie_batch_set_position rule.  qie_verify_logits
 * afterwards returns the M rows in row order.  A segment's results do not depend on the other
 * segments' ids; a call of one segment equals qie_verify of that slot bit for bit (the same M,
 * hence the same kernels and split length).  The call synchronises once, with one device-to-host
 * copy of every segment's {n_out, ids}.  With use_graph the step is captured once per (segment
 * table, sampling kind, entries) in qie_verify's bounded cache and replayed.  Collective under
 * tensor parallelism, like qie_verify.
 * Preconditions: 1 <= n_segs <= min(B, QIE_RAGGED_MAX_SEGS), seq strictly increasing, n_draft >= 0.
 * All-or-nothing, before anything is allocated or launched: -22 for a bad table, an idle or
 * released slot, a draft id out of range, any segment with p + n_draft + 1 >= max_ctx, M > 16, an
 * engine created with prefill_fp8, a batch in decode mode 1; -28 when the pool cannot hold all
 * segments' rows together (one reservation over n_segs spans, private copies of shared pages of
 * the write ranges included).  After either code every slot continues as if the call had not been
 * made. */
typedef struct qie_verify_seg { int32_t seq, n_draft; } qie_verify_seg;
int qie_verify_batch(qie_batch* b, const qie_verify_seg* segs, int32_t n_segs, const int32_t* draft,
                     const qie_sampling* s, int32_t* out_ids, int32_t* n_out);
/* qie_batch_logprobs over the rows qie_verify_logits would return: out[m] (host float [rows]) =
 * the log-probability of ids[m] (host [rows]; -1 = skip: 0.0f) under row m of the last qie_verify
 * or qie_verify_batch (qie_logprob_rows on the step's logits; gathered under tensor parallelism:
 * collective).  -22 when no verify step's rows are held. */
int qie_verify_logprobs(qie_batch* b, const int32_t* ids, float* out);
/* Diagnostics: how many verify steps (qie_verify and qie_verify_batch together) this batch has
 * captured so far; stays 0 without use_graph.  A call that replays a captured step leaves it
 * unchanged.  -22 for a NULL batch. */
int qie_batch_debug_verify_captures(const qie_batch* b);
/* One decode step for all B sequences (hipGraph replay when enabled);
 * next_ids: host [B] or NULL (then nothing is synchronised). */
int qie_decode_step(qie_batch* b, const qie_sampling* s, int32_t* next_ids);
/* n_steps decode steps back to back; out_ids host [n_steps][B] (may be NULL). */
int qie_decode(qie_batch* b, int32_t n_steps, const qie_sampling* s, int32_t* out_ids);
/* Last logits of every sequence: host bf16 [B][V]. */
int qie_batch_logits(qie_batch* b, void* host_out);
/* Current positions (host int32 [B]) and token history row of `seq`. */
int qie_batch_positions(qie_batch* b, int32_t* host_pos);
int qie_batch_history(qie_batch* b, int32_t seq, int32_t* host_ids, int32_t n);
/* Rewind/set sequence `seq` to position pos with current token `token`
 * (KV rows >= pos are simply overwritten later).  When pos lies in a page another holder shares
 * ("forks and prefix handles" below) the slot first gets a private page holding that page's rows
 * below pos only (-28 if the pool has none, nothing changed): the slot's rows at or past pos of
 * that page are then gone, so a later set_position forward over them without a write in between
 * finds undefined rows where a rewind within the slot's own pages finds the old ones. */
int qie_batch_set_position(qie_batch* b, int32_t seq, int32_t pos, int32_t token);

/* ------------------------------------------------- forks and prefix handles
 * Sequences that begin alike share KV pages instead of prefilling the same ids twice (DESIGN.md
 * §18).  Paged batches count the holders of every page: a page returns to the pool when the last
 * holder (a slot or a prefix handle) lets go of it; qie_batch_release and qie_prefill drop
 * references.  Every writer of the engine tier — the decode steps, qie_verify, qie_prefill_append /
 * qie_score at pos0 >= 1, qie_batch_set_position — first replaces the pages of its write range that
 * another holder shares by private ones (copying the rows below its first position), counted in
 * its all-or-nothing pool check (-28, the decode steps -22: the list at qie_batch_create_paged);
 * the other holder's pages are never touched.  The operator
 * tier's raw descriptors (qie_batch_kv_cache, qie_kv_write, qie_batch_reserve) do none of this:
 * writing through one into a page qie_batch_page_refs shows shared is the caller's doing.
 *
 * qie_batch_fork: src is a live slot at position p, dst != src any slot (a live dst is released
 * first; the pages only it holds count towards the check), 1 <= n_tokens <= p.  Afterwards dst is a
 * live sequence at position n_tokens whose K/V rows [0, n_tokens) equal src's bit for bit, with
 * src's history [0 .. n_tokens], current token = src's history[n_tokens] (for n_tokens == p the
 * pending current token, and then row dst of qie_batch_logits equals row src and a decode step
 * produces in dst exactly what it produces in src) and step counter = src's + step_offset (the
 * sampler draws from seed + step: forks that should sample differently get different offsets).
 * Paged: the n_tokens / page_tokens full pages are shared, the remaining rows copied into one fresh
 * page (qie_kv_copy); contiguous: all rows copied.  -22 for bad arguments or an idle src, -28 when
 * the pool cannot supply the tail page; nothing has changed in either case.  Synchronises;
 * collective under tensor parallelism (every rank decides alike). */
typedef struct qie_kv_prefix qie_kv_prefix;
int qie_batch_fork(qie_batch* b, int32_t src, int32_t dst, int32_t n_tokens, int32_t step_offset);

/* ------------------------------------------------------- per-slot sampling
 * Every slot may hold its own sampling entry (qie_slot_sampling, qie_types.h; the numerics
 * contract is stated at qie_sample_rows in qie_ops.h): top-k / temperature /
 * top-p / min-p / seed, repetition, presence and frequency penalties over a window of the slot's
 * own token history, and a logit bias list.  set: slot seq's entry := *p, NULL clears it.  -22
 * with nothing changed for seq out of range, n_bias outside [0, QIE_SLOT_BIAS_MAX], a bias id
 * outside [0, vocab) or listed twice, a bias that is NaN or +inf, a non-finite temperature or
 * penalty, repetition_penalty <= 0, min_p outside [0, 1], a negative penalty_start or
 * penalty_last_n.  get: the entry (zeroes without one) and whether one is set.
 *
 * An entry belongs to the slot until it is replaced or cleared: qie_batch_release, qie_prefill
 * and qie_batch_prefix_load leave it alone; qie_batch_fork gives dst what src has (its entry, or
 * none), so a decode step still produces in dst exactly what it produces in src, and
 * step_offset still moves the draw.  Every call that samples honours it — qie_prefill, _batch,
 * _append, qie_score (its sampled last row), qie_decode_step, qie_decode, qie_verify,
 * qie_batch_debug_step: a row whose slot has an entry samples under it (window end q: the
 * position of the row's input token; verify row i sees the history up to the pending token and
 * the drafts d1 .. di, exactly what a decode step there would see); a row whose slot has none
 * uses the call's qie_sampling.  When no row of a launch has an entry the launches are exactly
 * those of a batch that never had one.
 *
 * The entries live in a device table made at the first set (one fixed allocation, with the
 * sampler's own workspace beside it); a set is a copy ordered on the engine's stream.  The
 * captured decode graph and captured verify steps READ the table: changing an entry's values
 * never re-captures; "some slot has an entry" flipping does, as a change of the call's
 * qie_sampling does.  Tensor parallelism / comm_always: rows of a launch with an entry take the
 * gathered-row path of the sampled head, every rank samples the same full row — the caller
 * sets the same entries on every rank. */
int qie_batch_set_slot_sampling(qie_batch* b, int32_t seq, const qie_slot_sampling* p);
int qie_batch_slot_sampling(const qie_batch* b, int32_t seq, qie_slot_sampling* out, int32_t* is_set);
/* Paged batches: the holder count of pool pages 0 .. n-1 (host; 0 = free; page 0, the scratch
 * page, is always 0). */
int qie_batch_page_refs(qie_batch* b, int32_t* host_refs, int32_t n);
/* Prefix handles (paged batches; -22 on a contiguous one) keep a prefix alive after its slot is
 * gone.  save: a reference on the pages of [0, n_tokens) of live slot seq (n_tokens a positive
 * multiple of page_tokens, <= its position) and a host copy of those ids; takes no page, launches
 * nothing.  load: releases dst, shares the handle's first n_tokens / page_tokens pages with it
 * (n_tokens a positive multiple of page_tokens, <= the handle's length) and leaves it live at
 * position n_tokens with current token `token` and the history filled, as qie_batch_set_position
 * would; it takes no page (the page of position n_tokens is drawn by the append or decode step
 * that writes it), so it cannot return -28.  The caller appends the rest at pos0 = n_tokens.
 * tokens: the handle's first n ids (n <= its length) into host_ids, returning 0; host_ids NULL
 * returns the length.  drop releases the references; qie_batch_destroy drops open handles. */
int qie_batch_prefix_save(qie_batch* b, int32_t seq, int32_t n_tokens, qie_kv_prefix** out);
int qie_batch_prefix_load(qie_batch* b, const qie_kv_prefix* p, int32_t dst, int32_t n_tokens, int32_t token);
int qie_batch_prefix_tokens(const qie_kv_prefix* p, int32_t* host_ids, int32_t n);
int qie_batch_prefix_drop(qie_batch* b, qie_kv_prefix* p);

/* Decode structure of the batch's steps: 0 = five launches per layer (the reference path:
 * QKV GEMV, attention, O GEMV, gate/up GEMV, down GEMV, hipGraph-captured); 1 = the whole
 * layer stack as ONE persistent launch (one workgroup per CU, weight streams running ahead of
 * the layer's dependency edges, tagged hand-offs between CUs; bit-identical outputs).  Mode 1
 * covers batch 1, bf16 weights, one device, head_dim 64 or 128 and a contiguous KV cache;
 * other batches return an error (QIE_EINVAL) naming what is not covered.  The next step
 * re-captures the decode graph.  qie_batch_decode_mode returns the current mode.  Mode 1 is
 * SLOWER on MI355X (Qwen2-7B 317.5 vs 370.9 tok/s, Qwen2-0.5B 1,065 vs 1,566: its cross-CU
 * hand-offs cost more than the kernel boundaries they replace); mode 0 is
 * the default and the measured path. */
int qie_batch_set_decode_mode(qie_batch* b, int32_t mode);
int qie_batch_decode_mode(const qie_batch* b);
/* Diagnostics of decode mode 1: enable != 0 makes the persistent step record s_memrealtime
 * stamps (100 MHz, chip-wide) at its phase boundaries, [n_cu][n_layers][12] uint64 (slots:
 * 0 layer start, 1 x gathered, 2 QKV done, 3 attention done (attention CUs), 4 attention
 * output gathered (other CUs), 5 O done, 6 x' gathered + norm, 7 gate/up done, 8 h gathered,
 * 9 down done); host_out (n >= that count) receives the last step's stamps; enable = 0
 * frees the buffer.  Changing it re-captures the decode graph. */
int qie_batch_pk_trace(qie_batch* b, int32_t enable, uint64_t* host_out, int64_t n);
/* Batch geometry: B slots, max_ctx positions per slot. */
int qie_batch_dims(const qie_batch* b, int32_t* batch, int32_t* max_ctx);
/* KV descriptor of slot `seq` for the operator tier (qie_kv_write, qie_attention with
 * sequence index 0): contiguous -> that slot's region; paged -> the pool with the
 * slot's block-table row.  Valid until the batch is destroyed. */
int qie_batch_kv_cache(const qie_batch* b, int32_t seq, qie_kv_cache* out);
/* Operator tier: make slot `seq` a live sequence holding the KV pages for positions
 * [0, n_tokens) (paged: taken from the pool, all-or-nothing; contiguous: a bounds
 * check).  allocate_page_buffers (iengine.cu:90-100) in the reference's terms. */
int qie_batch_reserve(qie_batch* b, int32_t seq, int32_t n_tokens);
/* The engine's weight arena (load_all_weights_to_gpu_chunked's d_base_out /
 * total_bytes_out, iengine.cu:117) and its RoPE tables (fp32 [rows][head_dim/2]). */
int qie_engine_arena(const qie_engine* e, void** base, int64_t* bytes);
int qie_engine_rope_tables(const qie_engine* e, const float** rope_cos, const float** rope_sin,
                           int32_t* rows);
/* Time `iters` launches of one of the decode step's kernels with hipEvents on
 * the engine stream (which: 0 = gate/up GEMV, 1 = down GEMV, 2 = QKV GEMV,
 * 3 = O GEMV, 4 = lm_head GEMV, 5 = attention; the layer GEMVs cycle through
 * layers 1..L-1 so no weight stays cache-resident; 6 = the persistent layer stack of decode
 * mode 1, all layers per launch, the sequence state restored afterwards).  Returns the average
 * microseconds per launch and the algorithmic bytes per launch. */
int qie_batch_time_kernel(qie_batch* b, int32_t which, int32_t iters, double* avg_us,
                          double* bytes);
/* One decode step run eagerly (as qie_decode_step) that also copies the residual stream
 * into host_x: bf16 [2 n_layers + 1][batch][hidden], slot 0 = the step's input row, slot
 * 2l + 1 = after layer l's attention block (O-proj + residual), 2l + 2 = after its MLP
 * block (down-proj + residual).  Parity diagnostics (tools/flip_attrib.py). */
int qie_batch_debug_step(qie_batch* b, const qie_sampling* smp, int32_t* next_ids, void* host_x);

#ifdef __cplusplus
}
#endif

#endif /* QIE_ENGINE_H */
