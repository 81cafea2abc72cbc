// verify.hpp — the two kernels that frame a speculative verify step (k_verify.hip; the step
// itself is engine.hip's enqueue_verify).  One sequence `seq` of a batch at
// position p with a pending current token runs M = n_draft + 1 rows (the current token and the
// drafted ids) through the decode-form layer loop; verify_rows builds the rows, verify_commit
// accepts a prefix of the drafts and leaves the batch as after that many decode steps.
// Below them: the batched step's pair (qie_verify_batch), whose rows are segments
// of several slots, and the tree step's pair (qie_verify_tree; k_verify_tree.hip),
// whose rows are the nodes of a draft tree.
#pragma once

#include "qie_common.hpp"
#include "../../include/qie/qie_ops.h"

namespace qie {

constexpr int kVerifyMaxRows = 16;   // QIE_VERIFY_MAX_ROWS: the M <= 16 linear planner's range

struct VerifyRowsArgs {
    int seq, M;
    const int32_t* draft;   // [M - 1] drafted ids (device)
    int32_t vocab;
    const uint4* E;         // embedding table, H8 16-byte words per row
    const uint4* x_res;     // [B][H8]: row seq = the pending current token's embedding
    int64_t H8;
    const int32_t* pos;     // [B]
    const int32_t* step;    // [B]
    uint4* vx;              // [M][H8] the step's residual rows
    int32_t* vpos;          // [M] = pos[seq] + i
    int32_t* vstep;         // [M] = step[seq] + i
};

struct VerifyCommitArgs {
    int seq, M;
    unsigned long long* keys;   // greedy: [M] fused arg-max keys (left zero), else null
    const int32_t* ids;         // sampled: [M] chosen ids
    const int32_t* draft;       // [M - 1]
    int32_t vocab;
    int32_t* pos;               // [B]
    int32_t* step;              // [B]
    int32_t* hist;              // [B][hist_stride]
    int hist_stride;
    int32_t* ids_out;           // [B] the batch's last ids
    const uint4* E;
    uint4* x_res;               // [B][H8]
    int64_t H8;
    RopeCurArgs rca;
    const uint16_t* vlogits;    // [M][Vl] the step's logits (this rank's vocabulary shard)
    uint16_t* logits;           // [B][Vl] the batch's logits
    int64_t Vl;
    int32_t* res;               // [1 + M]: n_out, then the M chosen ids
};

// ---- the batched step (qie_verify_batch): the rows are segments, segment z the
// rows c, d1 .. dn of slot seq[z].  The table travels by value (the ragged layer's qie_row_segs);
// the drafts lie end to end, so segment z's begin at draft[row0[z] - z].
constexpr int kVerifyMaxSegs = QIE_RAGGED_MAX_SEGS;

// The batched step's result words: [z] = n_out of segment z, [kVerifyMaxSegs + m] = row m's id
constexpr int kVerifyBatchResWords = kVerifyMaxSegs + kVerifyMaxRows;

struct VerifyBatchRowsArgs {
    qie_row_segs segs;      // entries past n repeat M (as the ragged layer takes it)
    const int32_t* draft;   // [M - n] the segments' drafts end to end (device)
    int32_t vocab;
    const uint4* E;
    const uint4* x_res;     // [B][H8]
    int64_t H8;
    const int32_t* pos;     // [B]
    const int32_t* step;    // [B]
    uint4* vx;              // [M][H8]
    int32_t* vpos;          // [M] = pos[seq] + i (i: the row's index within its segment)
    int32_t* vstep;         // [M] = step[seq] + i
    int32_t* row_slot;      // [M] = seq: the slot whose entry and history the row samples under
    int32_t* tail_off;      // [M] = row0[z] - z: where the row's segment begins in draft
    int32_t* tail_len;      // [M] = i: the drafts d1 .. di before the row
};

struct VerifyBatchCommitArgs {
    qie_row_segs segs;
    unsigned long long* keys;   // greedy: [M] fused arg-max keys (left zero), else null
    const int32_t* ids;         // sampled: [M]
    const int32_t* draft;       // [M - n]
    int32_t vocab;
    int32_t* pos;
    int32_t* step;
    int32_t* hist;
    int hist_stride;
    int32_t* ids_out;
    const uint4* E;
    uint4* x_res;
    int64_t H8;
    RopeCurArgs rca;
    const uint16_t* vlogits;    // [M][Vl]
    uint16_t* logits;           // [B][Vl]
    int64_t Vl;
    int32_t* res;               // [kVerifyBatchResWords]
};

// n bf16 elements src -> dst in 16-byte words where the two rows share their offset within a
// 16-byte line (element-wise up to the first boundary and past the last), else element-wise
__device__ __forceinline__ void copy_row_bf16(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int64_t n) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const uintptr_t so = (uintptr_t)src & 15, dof = (uintptr_t)dst & 15;
    if (so != dof) {
        for (int64_t j = tid; j < n; j += nt) dst[j] = src[j];
        return;
    }
    const int64_t head = so ? min((int64_t)((16 - so) / 2), n) : 0;
    const int64_t body = (n - head) / 8;
    for (int64_t j = tid; j < head; j += nt) dst[j] = src[j];
    const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
    uint4* d4 = reinterpret_cast<uint4*>(dst + head);
    for (int64_t j = tid; j < body; j += nt) d4[j] = s4[j];
    for (int64_t j = head + body * 8 + tid; j < n; j += nt) dst[j] = src[j];
}

// ---- the tree step (qie_verify_tree; k_verify_tree.hip): the M rows are the nodes
// of a draft tree, node 0 the pending current token, node i >= 1 the id draft[i - 1] under node
// parent[i - 1] < i.  The tree's shape is device data: the step's words are one int32 block whose
// first 32 words (drafts, parents) are the call's one host-to-device copy, the rest what the rows
// kernel derives from them and the commit kernel leaves for the host and for qie_kv_compact.
constexpr int kVtDraft = 0;       // [16] draft[i - 1]: node i's id
constexpr int kVtParent = 16;     // [16] parent[i - 1]: node i's parent
constexpr int kVtRow = 32;        // [16] vrow[i] = p + i: the cache row of node i's K/V
constexpr int kVtAnc = 48;        // [16] anc[i]: bit j set iff j is i or an ancestor of i
constexpr int kVtDepth = 64;      // [16] depth(i): the sampler's tail_len
constexpr int kVtTailOff = 80;    // [16] 16 i: the sampler's tail_off into kVtIds
constexpr int kVtSlot = 96;       // [16] seq: the sampler's row_slot
constexpr int kVtRes = 112;       // [17] n_out, then the emitted ids
constexpr int kVtPath = 144;      // [16] path[d]: the accepted node of depth d, d = 0 .. a
constexpr int kVtAcc = 160;       // [1]  a: the depth reached
constexpr int kVtIds = 176;       // [16][16] row i: the ids on i's root path below the root, by depth
constexpr int kVtWords = kVtIds + 16 * 16;

struct VerifyTreeRowsArgs {
    int seq, M;
    int32_t* vt;            // the step's words (above)
    int32_t vocab;
    const uint4* E;
    const uint4* x_res;     // [B][H8]
    int64_t H8;
    const int32_t* pos;     // [B]
    const int32_t* step;    // [B]
    uint4* vx;              // [M][H8]
    int32_t* vpos;          // [M] = pos[seq] + depth(i): the RoPE position and the sampler's window end
    int32_t* vstep;         // [M] = step[seq] + depth(i)
};

struct VerifyTreeCommitArgs {
    int seq, M;
    unsigned long long* keys;   // greedy: [M] fused arg-max keys (left zero), else null
    const int32_t* ids;         // sampled: [M]
    int32_t* vt;
    int32_t vocab;
    int32_t* pos;
    int32_t* step;
    int32_t* hist;
    int hist_stride;
    int32_t* ids_out;
    const uint4* E;
    uint4* x_res;
    int64_t H8;
    RopeCurArgs rca;
    const uint16_t* vlogits;    // [M][Vl]
    uint16_t* logits;           // [B][Vl]
    int64_t Vl;
};

int launch_verify_tree_rows(const VerifyTreeRowsArgs& a, hipStream_t st);
int launch_verify_tree_commit(const VerifyTreeCommitArgs& a, hipStream_t st);

int launch_verify_rows(const VerifyRowsArgs& a, hipStream_t st);
int launch_verify_commit(const VerifyCommitArgs& a, hipStream_t st);
int launch_verify_batch_rows(const VerifyBatchRowsArgs& a, hipStream_t st);
int launch_verify_batch_commit(const VerifyBatchCommitArgs& a, hipStream_t st);

}  // namespace qie
