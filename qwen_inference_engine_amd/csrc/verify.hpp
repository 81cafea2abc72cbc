// verify.hpp — the two kernels that frame a speculative verify step (k_verify.hip; the step
// itself is engine.hip's enqueue_verify).  One sequence `seq` of a batch at
// position p with a pending current token runs M = n_draft + 1 rows (the current token and the
// drafted ids) through the decode-form layer loop; verify_rows builds the rows, verify_commit
// accepts a prefix of the drafts and leaves the batch as after that many decode steps.
#pragma once

#include "qie_common.hpp"

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

int launch_verify_rows(const VerifyRowsArgs& a, hipStream_t st);
int launch_verify_commit(const VerifyCommitArgs& a, hipStream_t st);

}  // namespace qie
