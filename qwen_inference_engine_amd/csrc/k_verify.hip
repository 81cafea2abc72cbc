// k_verify.hip — the kernels that frame a speculative verify step (verify.hpp).
// Plain HIP, vector stores only; every position and id they use comes from device memory, so
// the whole step replays from a captured hipGraph.
#include "verify.hpp"

namespace qie {

// Block i builds row i of the step: row 0 is the sequence's pending current token (its
// embedding already sits in x_res[seq], as finalize_kernel left it), row i >= 1 the embedding
// of draft i - 1; positions and sampling counters continue the sequence's.
__global__ __launch_bounds__(256) void verify_rows_kernel(VerifyRowsArgs a) {
    const int i = blockIdx.x;
    const uint4* src = a.x_res + (int64_t)a.seq * a.H8;
    if (i > 0) {
        int32_t tok = a.draft[i - 1];
        if (tok < 0 || tok >= a.vocab) tok = 0;   // (the host refused such a draft; never read out of bounds)
        src = a.E + (int64_t)tok * a.H8;
    }
    uint4* dst = a.vx + (int64_t)i * a.H8;
    for (int64_t j = threadIdx.x; j < a.H8; j += 256) dst[j] = src[j];
    if (threadIdx.x == 0) {
        a.vpos[i] = a.pos[a.seq] + i;
        a.vstep[i] = a.step[a.seq] + i;
    }
}

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

// One block.  Row i chose token t_i (fused arg-max keys or sampled ids, clamped as
// finalize_kernel clamps); the accepted length is the largest a with draft[j - 1] == t_(j - 1)
// for all 1 <= j <= a.  The sequence is left exactly as after a + 1 decode steps: history
// [p + 1 .. p + a + 1] = t_0 .. t_a, position p + a + 1 (and its RoPE row), counter + a + 1,
// x_res[seq] = E[t_a], the batch's logits row = the step's row a; the key slots are left zero.
__global__ __launch_bounds__(1024) void verify_commit_kernel(VerifyCommitArgs a) {
    __shared__ int32_t s_tok[kVerifyMaxRows];
    __shared__ int s_acc;
    const int tid = threadIdx.x;
    const int32_t p = a.pos[a.seq];
    if (tid < a.M) {
        int32_t tok = a.keys ? key_idx(a.keys[tid]) : a.ids[tid];
        if (tok < 0 || tok >= a.vocab) tok = 0;
        s_tok[tid] = tok;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        while (acc < a.M - 1 && a.draft[acc] == s_tok[acc]) acc++;
        s_acc = acc;
        int32_t* hist = a.hist + (int64_t)a.seq * a.hist_stride;
        for (int i = 0; i <= acc; i++)
            if (p + 1 + i < a.hist_stride) hist[p + 1 + i] = s_tok[i];
        a.pos[a.seq] = p + acc + 1;
        a.step[a.seq] = a.step[a.seq] + acc + 1;
        a.ids_out[a.seq] = s_tok[acc];
        a.res[0] = acc + 1;
    }
    if (tid < a.M) {
        a.res[1 + tid] = s_tok[tid];
        if (a.keys) a.keys[tid] = 0ull;
    }
    __syncthreads();
    const int acc = s_acc;
    write_rope_cur(a.rca, a.seq, p + acc + 1);
    const uint4* src = a.E + (int64_t)s_tok[acc] * a.H8;
    uint4* dst = a.x_res + (int64_t)a.seq * a.H8;
    for (int64_t j = tid; j < a.H8; j += blockDim.x) dst[j] = src[j];
    copy_row_bf16(a.vlogits + (int64_t)acc * a.Vl, a.logits + (int64_t)a.seq * a.Vl, a.Vl);
}

// ------------------------------------------------------------ the batched step
// The segment that holds row m: its index, slot, first row and row count.  Constant indices
// only (a by-value array indexed by a register is copied to scratch); the comparisons go
// through the table's own words, which keeps the chain a chain of selects.
struct SegOf {
    int z, seq, row0, rows;
};
__device__ __forceinline__ SegOf seg_of_row(const qie_row_segs& t, int m) {
    SegOf s{0, t.seq[0], 0, t.row0[1]};
#pragma unroll
    for (int k = 1; k < kVerifyMaxSegs; k++)
        if (k < t.n && m >= t.row0[k]) s = SegOf{k, t.seq[k], t.row0[k], t.row0[k + 1] - t.row0[k]};
    return s;
}

// Block m builds row m: verify_rows_kernel's row i = m - row0[z] of slot seq[z], and what the
// sampler needs to find that slot's entry and history and the segment's drafts before the row.
__global__ __launch_bounds__(256) void verify_batch_rows_kernel(VerifyBatchRowsArgs a) {
    const int m = blockIdx.x;
    const SegOf s = seg_of_row(a.segs, m);
    const int i = m - s.row0, d0 = s.row0 - s.z;   // the segments before hold row0 - z drafts
    const uint4* src = a.x_res + (int64_t)s.seq * a.H8;
    if (i > 0) {
        int32_t tok = a.draft[d0 + i - 1];
        if (tok < 0 || tok >= a.vocab) tok = 0;   // (the host refused such a draft; never read out of bounds)
        src = a.E + (int64_t)tok * a.H8;
    }
    uint4* dst = a.vx + (int64_t)m * a.H8;
    for (int64_t j = threadIdx.x; j < a.H8; j += 256) dst[j] = src[j];
    if (threadIdx.x == 0) {
        a.vpos[m] = a.pos[s.seq] + i;
        a.vstep[m] = a.step[s.seq] + i;
        a.row_slot[m] = s.seq;
        a.tail_off[m] = d0;
        a.tail_len[m] = i;
    }
}

// verify_commit_kernel's body per segment (kept beside it: sharing the body moved the single
// kernel's register allocation).  The grid has one block per ROW and the block of a segment's
// first row commits the segment, the others leave at once — the block finds its segment with
// seg_of_row, where a table indexed by the block id would go through scratch.  A block touches
// its slot's words, its segment's rows and result words only; the slots are distinct, so no
// block reads what another writes.
__global__ __launch_bounds__(1024) void verify_batch_commit_kernel(VerifyBatchCommitArgs a) {
    __shared__ int32_t s_tok[kVerifyMaxRows];
    __shared__ int s_acc;
    const SegOf s = seg_of_row(a.segs, blockIdx.x);
    if ((int)blockIdx.x != s.row0) return;   // uniform per block
    const int tid = threadIdx.x, seq = s.seq, M = s.rows;
    unsigned long long* keys = a.keys ? a.keys + s.row0 : nullptr;
    const int32_t* draft = a.draft + (s.row0 - s.z);
    const int32_t p = a.pos[seq];
    if (tid < M) {
        int32_t tok = keys ? key_idx(keys[tid]) : a.ids[s.row0 + tid];
        if (tok < 0 || tok >= a.vocab) tok = 0;
        s_tok[tid] = tok;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        while (acc < M - 1 && draft[acc] == s_tok[acc]) acc++;
        s_acc = acc;
        int32_t* hist = a.hist + (int64_t)seq * a.hist_stride;
        for (int i = 0; i <= acc; i++)
            if (p + 1 + i < a.hist_stride) hist[p + 1 + i] = s_tok[i];
        a.pos[seq] = p + acc + 1;
        a.step[seq] = a.step[seq] + acc + 1;
        a.ids_out[seq] = s_tok[acc];
        a.res[s.z] = acc + 1;
    }
    if (tid < M) {
        a.res[kVerifyMaxSegs + s.row0 + tid] = s_tok[tid];
        if (keys) keys[tid] = 0ull;
    }
    __syncthreads();
    const int acc = s_acc;
    write_rope_cur(a.rca, seq, p + acc + 1);
    const uint4* src = a.E + (int64_t)s_tok[acc] * a.H8;
    uint4* dst = a.x_res + (int64_t)seq * a.H8;
    for (int64_t j = tid; j < a.H8; j += blockDim.x) dst[j] = src[j];
    copy_row_bf16(a.vlogits + (int64_t)(s.row0 + acc) * a.Vl, a.logits + (int64_t)seq * a.Vl, a.Vl);
}

// 1 .. kVerifyMaxSegs segments of >= 1 row each, at most kVerifyMaxRows rows, entries past n = M
static bool verify_table_ok(const qie_row_segs& t) {
    if (t.n < 1 || t.n > kVerifyMaxSegs || t.row0[0] != 0) return false;
    for (int z = 0; z < kVerifyMaxSegs; z++)
        if (z < t.n ? (t.row0[z + 1] <= t.row0[z] || t.seq[z] < 0) : t.row0[z + 1] != t.row0[t.n]) return false;
    return t.row0[t.n] <= kVerifyMaxRows;
}

int launch_verify_batch_rows(const VerifyBatchRowsArgs& a, hipStream_t st) {
    QIE_REQUIRE(verify_table_ok(a.segs), "verify_batch_rows: malformed segment table");
    hipLaunchKernelGGL(verify_batch_rows_kernel, dim3(a.segs.row0[a.segs.n]), dim3(256), 0, st, a);
    QIE_LAUNCH_CHECK();
    return 0;
}

int launch_verify_batch_commit(const VerifyBatchCommitArgs& a, hipStream_t st) {
    QIE_REQUIRE(verify_table_ok(a.segs), "verify_batch_commit: malformed segment table");
    hipLaunchKernelGGL(verify_batch_commit_kernel, dim3(a.segs.row0[a.segs.n]), dim3(1024), 0, st, a);
    QIE_LAUNCH_CHECK();
    return 0;
}

int launch_verify_rows(const VerifyRowsArgs& a, hipStream_t st) {
    QIE_REQUIRE(a.M >= 1 && a.M <= kVerifyMaxRows, "verify_rows: %d rows", a.M);
    hipLaunchKernelGGL(verify_rows_kernel, dim3(a.M), dim3(256), 0, st, a);
    QIE_LAUNCH_CHECK();
    return 0;
}

int launch_verify_commit(const VerifyCommitArgs& a, hipStream_t st) {
    QIE_REQUIRE(a.M >= 1 && a.M <= kVerifyMaxRows, "verify_commit: %d rows", a.M);
    hipLaunchKernelGGL(verify_commit_kernel, dim3(1), dim3(1024), 0, st, a);
    QIE_LAUNCH_CHECK();
    return 0;
}

}  // namespace qie
