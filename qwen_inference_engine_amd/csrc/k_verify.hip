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
