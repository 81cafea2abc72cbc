// k_gemv.hip — bandwidth-bound skinny GEMM (M <= 8 rows) for the decode step.
//
// Replaces matrix_mul (layers/src/matrix_mul.cu:165-288) at M = 1 / small M,
// where the reference runs 16x16 WMMA tiles with 15 of 16 rows wasted and
// 2-byte loads.  Here (gfx950, wave64):
//   * each wave owns RPW weight rows and streams them along K with 16-byte
//     non-temporal loads (64 lanes x 16 B = 1 KiB per wave-instruction),
//     U chunks in flight per row;
//   * the activation rows live in LDS (optionally produced by a fused RMSNorm
//     prologue — the reference's launch_rms + proj pair in one launch);
//   * fp32 accumulation, wave butterfly reduction, one bf16 rounding;
//   * fused epilogues: bias (Qwen2), residual add (launch_resadd), SwiGLU
//     (launch_act + launch_elem: gate/up row j handled by the same wave), and a
//     greedy arg-max key (logit_decode.cu:15-33 tie rule) for lm_head.
// Grid is persistent-ish: min(tasks/4, CUs * blocks_per_cu) blocks of 4 waves
// that grid-stride over row tasks, so the norm prologue runs once per block.
#include "qie_common.hpp"
#include "launch_util.hpp"
#include "linear_epilogue.hpp"
#include "linear_plan.hpp"
#include "plan_format.hpp"
#include "../../include/qie/qie_ops.h"

#include <cstdlib>
#include <cstring>

namespace qie {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct GemvParams {
    const uint16_t* x;
    int64_t ldx;
    const uint16_t* w0;
    const uint16_t* w1;
    const uint16_t* w2;
    const uint16_t* b0;
    const uint16_t* b1;
    const uint16_t* b2;
    int64_t n0, n01;   // rows in seg0, seg0+seg1
    int64_t K, N;      // N = output columns
    uint16_t* y;
    int64_t ldy;
    const uint16_t* norm_w;
    float eps;
    int numerics;
    int M;             // runtime rows (<= MT)
    int xlds;          // 1: x staged in LDS
    unsigned long long* keys;
    int64_t key_col0;
    int64_t n_tasks;
    int dbg;           // skinny kernel timing experiments (QIE_SKINNY_DBG): 1 plain x copy instead of the
                       // fused norm, 2 stop after the prologue, 4 no prologue at all
    // interleaved RoPE in the STORE epilogue (decode QKV, M = 1, REF numerics, no qk-norm):
    // output rows [0, rope_rows) are (q | k) head rows of rope_hd; pair (2j, 2j + 1) of a
    // head is rotated by the fp32 table row of position rope_pos[0] (RoPE.cu:6-22)
    const int32_t* rope_pos;
    const float* rope_cs;
    const float* rope_sn;
    int rope_hd;
    int64_t rope_rows;
    int epre;          // M = 1: the first task's epilogue operands (bias / residual) loaded up front
    int mkdiv;         // x-first fused norm: REF quotient by the FMA-corrected reciprocal (dev A/B)
    int t16;           // skinny kernel, fp8: weights in the 16-row tiled layout (qie_fp8_tile16)
    // F32 epilogue under tensor parallelism (peer backend, M = 1): push = {tag, value} words
    // straight into every rank's tagged exchange slot (push.world > 0) instead of y
    PeerPush push;
};

// uniform loads through the scalar cache (constant address space): the RoPE coefficients
// wait on lgkmcnt, not behind the weight stream's in-order vmcnt
template <class T>
__device__ __forceinline__ T sload(const T* p, int64_t i) {
    return ((const __attribute__((address_space(4))) T*)p)[i];
}

__device__ __forceinline__ void fma8(float& acc, const float* xf, u32x4 w) {
    acc = fmaf(xf[0], bf_lo(w.x), acc);
    acc = fmaf(xf[1], bf_hi(w.x), acc);
    acc = fmaf(xf[2], bf_lo(w.y), acc);
    acc = fmaf(xf[3], bf_hi(w.y), acc);
    acc = fmaf(xf[4], bf_lo(w.z), acc);
    acc = fmaf(xf[5], bf_hi(w.z), acc);
    acc = fmaf(xf[6], bf_lo(w.w), acc);
    acc = fmaf(xf[7], bf_hi(w.w), acc);
}

__device__ __forceinline__ void unpack8(u32x4 v, float* f) {
    f[0] = bf_lo(v.x); f[1] = bf_hi(v.x);
    f[2] = bf_lo(v.y); f[3] = bf_hi(v.y);
    f[4] = bf_lo(v.z); f[5] = bf_hi(v.z);
    f[6] = bf_lo(v.w); f[7] = bf_hi(v.w);
}

// fp8 weights (WT = 1): 16 codes per 16-byte lane load (1024 weights per wave-load),
// decoded with v_cvt_pk_f32_fp8; the power-of-two row scale multiplies the fp32 sum
// once in the epilogue (exact: the same value as summing the dequantised products).
__device__ __forceinline__ const float* fp8_scales(const uint16_t* w, int64_t rows, int64_t K) {
    return reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(w) + rows * K);
}

template <int MT, int RPW, int EPI, int U, int XCH, int WT, int LB = 256>
__global__ __launch_bounds__(LB) void gemv_kernel(GemvParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* xs = reinterpret_cast<uint16_t*>(smem);
    float* red = reinterpret_cast<float*>(smem + (p.xlds ? (size_t)MT * p.K * 2 : 0));
    // wave index made provably wave-uniform: every task / row pointer below derives from
    // it, so the weight rows' buffer resources stay in SGPRs
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NWv = blockDim.x >> 6;         // waves per block: 4, or 5..9 for the one-block-per-CU grid
    const int64_t TS = (int64_t)blockDim.x * 8;   // x elements per block-wide 16-byte pass
    const int64_t K = p.K;
    constexpr int EB = WT ? 1 : 2;     // bytes per weight
    constexpr int EL = 16 / EB;        // weights per 16-byte lane load
    constexpr int WS = 64 * EL;        // weights per wave-load
    // Weight rows and x are read with buffer loads: one VGPR offset per lane plus a constant
    // per chunk (no 64-bit address per chunk), and a chunk past the row end (K not a multiple
    // of a wave-load) reads zeros from the hardware range check instead of a clamped re-read.
    auto rsrc = [](const void* base, int64_t bytes) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
    };
    constexpr int kNT = 2;   // buffer-load cache policy: nt (weights stream once)

    // ---------------- task -> weight rows / output columns
    auto task_ptrs = [&](int64_t task, const u32x4* (&wr)[RPW]) {
        const uint8_t* w0 = reinterpret_cast<const uint8_t*>(p.w0);
        const uint8_t* w1 = reinterpret_cast<const uint8_t*>(p.w1);
        const uint8_t* w2 = reinterpret_cast<const uint8_t*>(p.w2);
        if constexpr (EPI == QIE_EPI_SWIGLU) {
            constexpr int P2 = RPW / 2;
#pragma unroll
            for (int i = 0; i < P2; i++) {
                int64_t j = task * P2 + i;
                if (j >= p.N) j = p.N - 1;
                wr[i] = reinterpret_cast<const u32x4*>(w0 + j * K * EB);
                wr[P2 + i] = reinterpret_cast<const u32x4*>(w1 + j * K * EB);
            }
        } else {
#pragma unroll
            for (int i = 0; i < RPW; i++) {
                int64_t r = task * RPW + i;
                if (r >= p.N) r = p.N - 1;
                const uint8_t* base;
                if (r < p.n0) base = w0 + r * K * EB;
                else if (r < p.n01) base = w1 + (r - p.n0) * K * EB;
                else base = w2 + (r - p.n01) * K * EB;
                wr[i] = reinterpret_cast<const u32x4*>(base);
            }
        }
    };
    // fp8: the row scale of output column c (segment-resolved like task_ptrs)
    auto row_scale = [&](int64_t c, int i) -> float {
        if constexpr (WT == 0) {
            return 1.f;
        } else if constexpr (EPI == QIE_EPI_SWIGLU) {
            constexpr int P2 = RPW / 2;
            return i < P2 ? fp8_scales(p.w0, p.N, K)[c] : fp8_scales(p.w1, p.N, K)[c];
        } else {
            if (c < p.n0) return fp8_scales(p.w0, p.n0, K)[c];
            if (c < p.n01) return fp8_scales(p.w1, p.n01 - p.n0, K)[c - p.n0];
            return fp8_scales(p.w2, p.N - p.n01, K)[c - p.n01];
        }
    };
    auto task_cols = [&](int64_t task, int64_t (&col)[RPW]) {
        if constexpr (EPI == QIE_EPI_SWIGLU) {
            constexpr int P2 = RPW / 2;
#pragma unroll
            for (int i = 0; i < P2; i++) col[i] = col[P2 + i] = task * P2 + i;
        } else {
#pragma unroll
            for (int i = 0; i < RPW; i++) col[i] = task * RPW + i;
        }
    };
    // Chunk slots past K re-read the row's last 16 B and are skipped by compute_chunk.  A
    // load under a condition (even a per-lane one) is branched around, and at the join
    // the waitcnt pass can no longer count it, so every later wait degrades to vmcnt(0).
    // XCH == 1 (MT = 1, no norm): x is not staged; each lane loads the 16 B of x that its
    // weight chunk multiplies together with that chunk (L1/L2 hits: every wave of the
    // block reads the same row), so no prologue or barrier precedes the weight stream.
    uint4 xg[XCH == 1 ? U : 1];
    // XCH == 3 (MT = 1, fused RMSNorm, K <= 512 U): the 64 lanes of a wave load all of x
    // between them (U 16-B chunks per lane), so every wave reduces the sum of squares itself
    // (wave_sum, no cross-wave exchange); wave w then normalises chunks w, w + NW, ... into
    // LDS — one barrier in all, instead of the x-first prologue's two around a block reduction.
    uint4 xr[XCH == 3 ? U : 1];
    // XCH == 4 (MT = 1, fused RMSNorm, K <= 512 U): as XCH == 3, but every wave also
    // normalises ITS OWN chunks in registers — lane l's x chunk u is exactly the 8 elements
    // its weight chunk u multiplies — so there is no LDS image, no barrier and no LDS read
    // in the weight loop; the norm's divisions are repeated per wave (56 per lane at
    // K = 3,584) while the weight stream is in flight.
    uint4 xq[XCH == 4 ? U : 1];
    // Epilogue operands of the wave's FIRST task (M = 1: bias values of STORE rows, the old
    // residual values of RESIDUAL rows) loaded before its weight stream, so the epilogue of a
    // one-task wave — every small decode GEMV — has no dependent load after the reduction.
    // Unconditional buffer loads (a missing bias reads element 0 of x; the epilogue ignores it).
    constexpr bool EPRE = MT == 1 && (EPI == QIE_EPI_RESIDUAL || EPI == QIE_EPI_STORE);
    uint32_t epre_v[EPRE ? RPW : 1];
    // the loads are issued WITHOUT a branch: a load under a (even uniform) condition makes the
    // waitcnt pass fall back to vmcnt(0) at every later wait, and the weight stream stops
    // pipelining (the first, branched form measured QKV 10.0 -> 10.7, O 6.4 -> 6.9 us)
    constexpr bool EPRE_ON = EPRE && XCH > 0;
    const bool epre_on = EPRE_ON && p.M == 1 && p.epre != 0;   // uniform; p.epre = 0 (dev A/B): reload
    auto epre_issue = [&](int64_t task) {
        if constexpr (EPRE) {
#pragma unroll
            for (int i = 0; i < RPW; i++) {
                int64_t c = task * RPW + i;
                c = c < p.N ? c : p.N - 1;
                if constexpr (EPI == QIE_EPI_RESIDUAL) {
                    const auto ry = rsrc(p.y, p.N * 2);
                    epre_v[i] = __builtin_amdgcn_raw_buffer_load_b16(ry, (int)(c * 2), 0, 0);
                } else {
                    const uint16_t* b = c < p.n0 ? p.b0 : (c < p.n01 ? p.b1 : p.b2);
                    const int64_t bi = c < p.n0 ? c : (c < p.n01 ? c - p.n0 : c - p.n01);
                    const auto rb = rsrc(b ? (const void*)b : (const void*)p.x, b ? (bi + 1) * 2 : 2);
                    epre_v[i] = __builtin_amdgcn_raw_buffer_load_b16(rb, b ? (int)(bi * 2) : 0, 0, 0);
                }
            }
        }
    };
    auto load_chunk = [&](const u32x4* const (&wr)[RPW], int64_t k0, u32x4 (&wv)[U][RPW]) {
        const int voff = (int)(k0 * EB);   // this lane's byte offset in the row (< 2^31)
        const auto rx = rsrc(p.x, K * 2);
#pragma unroll
        for (int u = 0; u < U; u++) {
            if constexpr (XCH == 1) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(k0 * 2), u * WS * 2, 0);
                xg[u] = make_uint4(v.x, v.y, v.z, v.w);
            }
#pragma unroll
            for (int i = 0; i < RPW; i++)   // unconditional loads (a chunk past K reads zeros)
                wv[u][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc(wr[i], K * EB), voff, u * WS * EB, kNT);
        }
    };
    auto x_at = [&](int m, int64_t k) -> uint4 {
        return p.xlds ? *reinterpret_cast<const uint4*>(xs + (int64_t)m * K + k)
                      : (m < p.M ? *reinterpret_cast<const uint4*>(p.x + (int64_t)m * p.ldx + k)
                                 : make_uint4(0, 0, 0, 0));
    };
    auto compute_chunk = [&](int64_t k0, const u32x4 (&wv)[U][RPW], float (&acc)[MT][RPW]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t k = k0 + u * WS;
            if (k < K) {
                if constexpr (WT == 0) {
#pragma unroll
                    for (int m = 0; m < MT; m++) {
                        const uint4 xv = XCH == 1 ? xg[XCH == 1 ? u : 0] : (XCH == 4 ? xq[XCH == 4 ? u : 0] : x_at(m, k));
                        float xf[8];
                        unpack8(u32x4{xv.x, xv.y, xv.z, xv.w}, xf);
#pragma unroll
                        for (int i = 0; i < RPW; i++) fma8(acc[m][i], xf, wv[u][i]);
                    }
                } else {
                    float wf[RPW][16];
#pragma unroll
                    for (int i = 0; i < RPW; i++) {
                        fp8x4_to_f32(wv[u][i].x, wf[i]);
                        fp8x4_to_f32(wv[u][i].y, wf[i] + 4);
                        fp8x4_to_f32(wv[u][i].z, wf[i] + 8);
                        fp8x4_to_f32(wv[u][i].w, wf[i] + 12);
                    }
#pragma unroll
                    for (int m = 0; m < MT; m++) {
                        const uint4 x0 = x_at(m, k), x1 = x_at(m, k + 8);
                        float xf[16];
                        unpack8(u32x4{x0.x, x0.y, x0.z, x0.w}, xf);
                        unpack8(u32x4{x1.x, x1.y, x1.z, x1.w}, xf + 8);
#pragma unroll
                        for (int i = 0; i < RPW; i++)
#pragma unroll
                            for (int j = 0; j < 16; j++) acc[m][i] = fmaf(xf[j], wf[i][j], acc[m][i]);
                    }
                }
            }
        }
    };

    const int64_t tstride = (int64_t)gridDim.x * NWv;
    const int64_t task0 = (int64_t)blockIdx.x * NWv + wave;
    // RoPE epilogue: the position goes out first (one scalar load), its table row for the
    // first task after the prologue, so neither round trip lands after the weight stream
    constexpr bool ROPE = EPI == QIE_EPI_STORE && RPW % 2 == 0 && MT == 1;
    const bool rope = ROPE && p.rope_rows > 0;
    int32_t rpos = 0;   // loaded right after the first weight issue (an lgkmcnt wait before it would hold the issue)
    const u32x4* wr[RPW];
    u32x4 wv[U][RPW];
    constexpr bool PF = XCH > 0;

    if constexpr (XCH == 1) {
        if constexpr (EPRE_ON) epre_issue(task0 < p.n_tasks ? task0 : p.n_tasks - 1);
        task_ptrs(task0 < p.n_tasks ? task0 : p.n_tasks - 1, wr);
        load_chunk(wr, (int64_t)lane * EL, wv);
    } else if constexpr (XCH == 3) {
        // x chunks first, then the wave's first weight chunks, THEN the norm arithmetic
        // (vmcnt retires in order: the x loads must be the older ones)
        const auto rx = rsrc(p.x, K * 2), rn = rsrc(p.norm_w, K * 2);
#pragma unroll
        for (int u = 0; u < U; u++) {   // a chunk past K reads zeros (range check)
            const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rx, lane * 16, u * 1024, 0);
            xr[u] = make_uint4(a.x, a.y, a.z, a.w);
        }
        // the norm weights of the (at most NWC) chunks this wave normalises, also before the
        // weight stream: a load issued after it could only be waited for behind all of it
        constexpr int NWC = (U + 3) / 4;   // chunks per wave at >= 4 waves per block
        u32x4 nvw[NWC];
#pragma unroll
        for (int c = 0; c < NWC; c++) {
            const int u = wave + c * NWv;   // wave-uniform; past U: a harmless in-range re-read
            nvw[c] = __builtin_amdgcn_raw_buffer_load_b128(rn, lane * 16, (u < U ? u : 0) * 1024, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (EPRE_ON) epre_issue(task0 < p.n_tasks ? task0 : p.n_tasks - 1);
        task_ptrs(task0 < p.n_tasks ? task0 : p.n_tasks - 1, wr);
        load_chunk(wr, (int64_t)lane * EL, wv);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; u++)   // opaque: the x math cannot be hoisted above the weight issue
            asm volatile("" : "+v"(xr[u].x), "+v"(xr[u].y), "+v"(xr[u].z), "+v"(xr[u].w));
#pragma unroll
        for (int c = 0; c < NWC; c++) asm volatile("" : "+v"(nvw[c]));
        float ss = 0.f;
#pragma unroll
        for (int u = 0; u < U; u++) {
            float f[8];
            unpack8(u32x4{xr[u].x, xr[u].y, xr[u].z, xr[u].w}, f);
#pragma unroll
            for (int j = 0; j < 8; j++) ss += f[j] * f[j];
        }
        ss = wave_sum(ss);
        const float rms = sqrtf((ss / (float)K) + p.eps);
        const float inv = 1.0f / rms;
        const bool hf = p.numerics == QIE_NUMERICS_HF;
        const int nch = (int)((K + WS - 1) / WS);
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
        for (int c = 0; c < NWC; c++) {   // static indices into xr / nvw: no scratch
            if (u != wave + c * NWv || u >= nch) continue;   // wave-uniform
            float f[8], wf[8];
            unpack8(xr[u], f);
            unpack8(nvw[c], wf);
            const int64_t k = (int64_t)lane * EL + u * WS;
            if (k < K) *reinterpret_cast<uint4*>(xs + k) = rms_apply8(f, wf, rms, inv, hf, false);
        }
        __syncthreads();
    } else if constexpr (XCH == 4) {
        // x and the norm weights first (one 16-B chunk per wave-load slot u, a chunk past K
        // reads zeros), then the first task's weight stream, THEN the norm arithmetic
        const auto rx = rsrc(p.x, K * 2), rn = rsrc(p.norm_w, K * 2);
        u32x4 xa[U], na[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            xa[u] = __builtin_amdgcn_raw_buffer_load_b128(rx, lane * 16, u * 1024, 0);
            na[u] = __builtin_amdgcn_raw_buffer_load_b128(rn, lane * 16, u * 1024, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (EPRE_ON) epre_issue(task0 < p.n_tasks ? task0 : p.n_tasks - 1);
        task_ptrs(task0 < p.n_tasks ? task0 : p.n_tasks - 1, wr);
        load_chunk(wr, (int64_t)lane * EL, wv);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; u++) asm volatile("" : "+v"(xa[u]), "+v"(na[u]));
        float ss = 0.f;
#pragma unroll
        for (int u = 0; u < U; u++) {
            float f[8];
            unpack8(xa[u], f);
#pragma unroll
            for (int j = 0; j < 8; j++) ss += f[j] * f[j];
        }
        ss = wave_sum(ss);
        const float rms = sqrtf((ss / (float)K) + p.eps);
        const float inv = 1.0f / rms;
        const bool hf = p.numerics == QIE_NUMERICS_HF;
#pragma unroll
        for (int u = 0; u < U; u++) {
            float f[8], wf[8];
            unpack8(xa[u], f);
            unpack8(na[u], wf);
            xq[u] = rms_apply8(f, wf, rms, inv, hf, p.mkdiv != 0);
        }
    } else if constexpr (XCH > 0) {
        // ---------------- x-first prologue (MT = 1, x staged in LDS, K <= 2048 * XCH; the
        // host guarantees it).  Order of issue: this thread's x chunks (+ norm weights),
        // then the first weight chunk of the wave's first task, THEN the x arithmetic — so
        // the weight stream's first HBM round trip overlaps the x round trip instead of
        // following it (vmcnt retires in order: x must be issued first).
        constexpr int NV = XCH <= 5 ? XCH : 1;   // norm weights: fused-norm variants only (XCH <= 5)
        const bool nrm = NV == XCH && p.norm_w != nullptr && !QIE_DBG(p.dbg & 1);   // dev: 1 skips the norm
        uint4 xv[XCH], nv[NV];
#pragma unroll
        for (int c = 0; c < XCH; c++) {
            const int64_t k = (int64_t)tid * 8 + c * TS;
            const int64_t kc = k < K ? k : K - 8;   // clamped: loads stay unconditional
            xv[c] = *reinterpret_cast<const uint4*>(p.x + kc);
            if (c < NV) nv[c] = *reinterpret_cast<const uint4*>((nrm ? p.norm_w : p.x) + kc);
        }
        __builtin_amdgcn_sched_barrier(0);
        // unconditional (a wave without a task re-reads the last row): a load under a
        // branch makes the vmcnt bookkeeping at the join wait for everything
        if constexpr (EPRE_ON) epre_issue(task0 < p.n_tasks ? task0 : p.n_tasks - 1);
        task_ptrs(task0 < p.n_tasks ? task0 : p.n_tasks - 1, wr);
        load_chunk(wr, (int64_t)lane * EL, wv);
        __builtin_amdgcn_sched_barrier(0);
        if (rope) rpos = sload(p.rope_pos, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < XCH; c++) {   // opaque: x math cannot be hoisted above the weight issue
            asm volatile("" : "+v"(xv[c].x), "+v"(xv[c].y), "+v"(xv[c].z), "+v"(xv[c].w));
            if (c < NV) asm volatile("" : "+v"(nv[c].x), "+v"(nv[c].y), "+v"(nv[c].z), "+v"(nv[c].w));
        }
        bool staged = false;
        if constexpr (NV == XCH) if (nrm) {
            staged = true;
            float ss = 0.f;
#pragma unroll
            for (int c = 0; c < XCH; c++) {
                if ((int64_t)tid * 8 + c * TS >= K) continue;
                float f[8];
                unpack8(u32x4{xv[c].x, xv[c].y, xv[c].z, xv[c].w}, f);
#pragma unroll
                for (int j = 0; j < 8; j++) ss += f[j] * f[j];
            }
            ss = wave_sum(ss);
            if (lane == 0) red[wave] = ss;
            __syncthreads();
            ss = 0.f;
            for (int w = 0; w < NWv; w++) ss += red[w];
            const float rms = sqrtf((ss / (float)K) + p.eps);
            const float inv = 1.0f / rms;
            const bool hf = p.numerics == QIE_NUMERICS_HF;
#pragma unroll
            for (int c = 0; c < XCH; c++) {
                const int64_t k = (int64_t)tid * 8 + c * TS;
                if (k >= K) continue;
                *reinterpret_cast<uint4*>(xs + k) = rms_apply8(xv[c], nv[c], rms, inv, hf, p.mkdiv != 0);
            }
        }
        if (!staged) {
#pragma unroll
            for (int c = 0; c < XCH; c++) {
                const int64_t k = (int64_t)tid * 8 + c * TS;
                if (k < K) *reinterpret_cast<uint4*>(xs + k) = xv[c];
            }
        }
        __syncthreads();
    } else if (p.xlds) {
        // ---------------- prologue: activation rows -> LDS (optionally RMS-normed)
        for (int m = 0; m < MT; m++) {
            const uint16_t* xr = p.x + (int64_t)m * p.ldx;
            uint16_t* xo = xs + (int64_t)m * K;
            if (m >= p.M) {
                for (int64_t k = tid * 8; k < K; k += TS)
                    *reinterpret_cast<uint4*>(xo + k) = make_uint4(0, 0, 0, 0);
                continue;
            }
            if (p.norm_w) {
                float ss = 0.f;
                for (int64_t k = tid * 8; k < K; k += TS) {
                    uint4 v = *reinterpret_cast<const uint4*>(xr + k);
                    float f[8];
                    unpack8(u32x4{v.x, v.y, v.z, v.w}, f);
#pragma unroll
                    for (int j = 0; j < 8; j++) ss += f[j] * f[j];
                }
                ss = wave_sum(ss);
                if (lane == 0) red[wave] = ss;
                __syncthreads();
                ss = 0.f;
                for (int w = 0; w < NWv; w++) ss += red[w];
                __syncthreads();
                const float rms = sqrtf((ss / (float)K) + p.eps);
                const float inv = 1.0f / rms;
                const bool hf = p.numerics == QIE_NUMERICS_HF;
                for (int64_t k = tid * 8; k < K; k += TS) {
                    const uint4 v = *reinterpret_cast<const uint4*>(xr + k);
                    const uint4 nw = *reinterpret_cast<const uint4*>(p.norm_w + k);
                    *reinterpret_cast<uint4*>(xo + k) = rms_apply8(v, nw, rms, inv, hf, false);
                }
            } else {
                for (int64_t k = tid * 8; k < K; k += TS)
                    *reinterpret_cast<uint4*>(xo + k) = *reinterpret_cast<const uint4*>(xr + k);
            }
        }
        __syncthreads();
    }
    if constexpr (XCH == 0 || XCH == 1 || XCH == 3 || XCH == 4)   // prologues without the early position load
        if (rope) rpos = sload(p.rope_pos, 0);
    float rc[ROPE ? RPW / 2 : 1], rs[ROPE ? RPW / 2 : 1];
    auto rope_coef = [&](int64_t task, float* c_out, float* s_out) {
#pragma unroll
        for (int i = 0; i < (ROPE ? RPW / 2 : 0); i++) {
            const int64_t c = task * RPW + 2 * i;   // STORE: rows of a task are consecutive
            const int64_t j = (int64_t)rpos * (p.rope_hd / 2) + (c % p.rope_hd) / 2;
            const bool ok = c + 1 < p.rope_rows;
            c_out[i] = ok ? sload(p.rope_cs, j) : 1.f;
            s_out[i] = ok ? sload(p.rope_sn, j) : 0.f;
        }
    };
    if (rope) rope_coef(task0 < p.n_tasks ? task0 : 0, rc, rs);

    // Running arg-max key per row (lane 0 of each wave); reduced over the block and
    // published with ONE atomicMax per block after the task loop — an atomic per task
    // serialises ~76k atomics on one address for a 152k-row lm_head (0.9 ms).
    unsigned long long kbest[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) kbest[m] = 0ull;

    // ---------------- main loop over row tasks.  Software-pipelined across tasks: the
    // first weight chunk of a wave's NEXT task is issued before this task's reduction
    // and epilogue (and the first task's before the prologue above), so a wave with one
    // or two tasks — every small decode GEMV — pays one HBM round trip, not three.
    for (int64_t task = task0; task < p.n_tasks; task += tstride) {
        int64_t col[RPW];
        task_cols(task, col);
        if constexpr (!PF) {
            task_ptrs(task, wr);
            load_chunk(wr, (int64_t)lane * EL, wv);
        }
        float acc[MT][RPW];
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int i = 0; i < RPW; i++) acc[m][i] = 0.f;
        compute_chunk((int64_t)lane * EL, wv, acc);
        for (int64_t k0 = (int64_t)lane * EL + WS * U; k0 < K; k0 += WS * U) {
            load_chunk(wr, k0, wv);
            compute_chunk(k0, wv, acc);
        }
        if (PF && task + tstride < p.n_tasks) {
            task_ptrs(task + tstride, wr);
            load_chunk(wr, (int64_t)lane * EL, wv);
        }
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int i = 0; i < RPW; i++) acc[m][i] = wave_sum(acc[m][i]);
        if constexpr (WT != 0) {   // fp8: the power-of-two row scale, once per output
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < RPW; i++) {
                    const float sc = row_scale(col[i] < p.N ? col[i] : p.N - 1, i);
#pragma unroll
                    for (int m = 0; m < MT; m++) acc[m][i] *= sc;
                }
            }
        }

        // ---------------- epilogue (lane 0 writes; outputs are tiny)
        if (lane == 0) {
#pragma clang fp contract(off)
#pragma unroll
            for (int m = 0; m < MT; m++) {
                if (m >= p.M) continue;
                uint16_t* yr = p.y + (int64_t)m * p.ldy;
                if constexpr (EPI == QIE_EPI_SWIGLU) {
                    constexpr int P2 = RPW / 2;
#pragma unroll
                    for (int i = 0; i < P2; i++) {
                        if (col[i] >= p.N) continue;
                        yr[col[i]] = swiglu_bf16(acc[m][i], acc[m][P2 + i]);
                    }
                } else if constexpr (EPI == QIE_EPI_F32) {
                    if (p.push.world > 0) {
                        // the row-parallel exchange's send, issued as each row finishes
                        // (comm.hip peer_tag_kernel<true> waits for and reduces it)
                        const unsigned e = __hip_atomic_load(p.push.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                        for (int i = 0; i < RPW; i++) {
                            if (col[i] >= p.N) continue;
                            const uint64_t w = (uint64_t)(e + 1) | ((uint64_t)__float_as_uint(acc[m][i]) << 32);
                            const int64_t at = (int64_t)m * p.ldy + col[i];
#pragma unroll
                            for (int q = 0; q < kPeerTagMaxWorld; q++)
                                if (q < p.push.world)
                                    __hip_atomic_store(peer_tag_slot(p.push.tb[q], e, p.push.rank) + at, w,
                                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        }
                    } else {
                        float* yf = reinterpret_cast<float*>(p.y) + (int64_t)m * p.ldy;
#pragma unroll
                        for (int i = 0; i < RPW; i++)
                            if (col[i] < p.N) yf[col[i]] = acc[m][i];
                    }
                } else if constexpr (EPI == QIE_EPI_RESIDUAL) {
                    const bool pre = epre_on && task == task0;
#pragma unroll
                    for (int i = 0; i < RPW; i++) {
                        if (col[i] >= p.N) continue;
                        const float old = pre ? bf2f(epre_v[EPRE ? i : 0]) : bf2f(yr[col[i]]);
                        yr[col[i]] = f2bf(old + rbf(acc[m][i]));
                    }
                } else {
                    unsigned long long best = kbest[m];
                    float vv[RPW];
#pragma unroll
                    for (int i = 0; i < RPW; i++) {
                        const int64_t c = col[i] < p.N ? col[i] : p.N - 1;
                        float v = acc[m][i];
                        const uint16_t* b = c < p.n0 ? p.b0 : (c < p.n01 ? p.b1 : p.b2);
                        if (QIE_DBG(p.dbg & 2)) {   // dev: 2 skips the bias
                        } else if (epre_on && task == task0) {
                            if (b) v = v + bf2f(epre_v[EPRE ? i : 0]);
                        } else if (b) {
                            int64_t bi = c < p.n0 ? c : (c < p.n01 ? c - p.n0 : c - p.n01);
                            v = v + bf2f(b[bi]);
                        }
                        vv[i] = rbf(v);   // the projection's bf16 output
                    }
                    if constexpr (ROPE) {
                        if (rope) {   // uniform: (2j, 2j + 1) pairs of q / k head rows
                            float tc[RPW / 2], ts[RPW / 2];
                            if (task != task0) rope_coef(task, tc, ts);
#pragma unroll
                            for (int i = 0; i < RPW / 2; i++) {
                                const int64_t c = col[2 * i];
                                if (c + 1 >= p.rope_rows || c + 1 >= p.N) continue;
                                const float cs = task == task0 ? rc[i] : tc[i];
                                const float sn = task == task0 ? rs[i] : ts[i];
                                const float x0 = vv[2 * i], x1 = vv[2 * i + 1];
                                vv[2 * i] = x0 * cs - x1 * sn;
                                vv[2 * i + 1] = x1 * cs + x0 * sn;
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < RPW; i++) {
                        const int64_t c = col[i];
                        if (c >= p.N) continue;
                        uint16_t o = f2bf(vv[i]);
                        yr[c] = o;
                        if (p.keys) {
                            unsigned long long kk = sel_key(bf2f(o), (uint32_t)(c + p.key_col0));
                            best = kk > best ? kk : best;
                        }
                    }
                    kbest[m] = best;
                }
            }
        }
    }
    if constexpr (EPI == QIE_EPI_STORE) {
        if (p.keys) {
            __shared__ unsigned long long kb_s[16][MT];
            if (lane == 0) {
#pragma unroll
                for (int m = 0; m < MT; m++) kb_s[wave][m] = kbest[m];
            }
            __syncthreads();
            if (tid < MT && tid < p.M) {
                unsigned long long b = kb_s[0][tid];
#pragma unroll
                for (int w = 1; w < NWv; w++) b = kb_s[w][tid] > b ? kb_s[w][tid] : b;
                if (b) atomicMax(p.keys + tid, b);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Skinny MFMA GEMM for 2 <= M <= 16 (batched decode, short prefills): the M activation
// rows are the 16 rows of v_mfma_f32_16x16x32_bf16's A operand (rows >= M compute
// garbage that is never stored), a block owns 16 output columns (16 weight rows; 16
// gate + 16 up for SwiGLU) and its 4 waves split K, so the weights stream exactly once
// as B fragments (16 B per lane per MFMA step, one weight row per lane column) and the
// per-element VALU work of the GEMV (M FMAs per weight) moves to the matrix cores.  fp8
// weights: a 16-B load holds 16 codes = two k-steps; decoded to bf16 (exact) for the
// bf16 MFMA, the row scale applied to the fp32 result.  Partial C tiles of the 4 waves
// are summed in LDS, then the epilogue (bias / arg-max keys / residual / SwiGLU / f32).
// Persistent over column tiles (grid <= 4 blocks per CU) so arg-max keys merge per block.
template <int EPI, int WT, int XL, int NW, int UO = 0>
__global__ __launch_bounds__(NW * 64) void skinny_mfma_kernel(GemvParams p) {
#pragma clang fp contract(off)
    constexpr int NB = EPI == QIE_EPI_SWIGLU ? 2 : 1;   // B tiles per block (gate, up)
    // A unit = 64 k of each of the tile's 16 weight rows: a lane loads 32 contiguous bytes
    // of its row (bf16: two 16-B vectors, two MFMA k-steps; fp8: one 16-B vector of 16
    // codes), so one unit reads whole 128-B lines per row (bf16; fp8 64 B) instead of the
    // 64-B half lines of a 32-k unit.
    constexpr int KSTEP = 64;
    constexpr int WV = WT ? 1 : 2;                        // 16-B weight vectors per lane per unit
    // units per step (UO: sized to the wave's K range, so no step slot is a dead unit)
    constexpr int U = UO ? UO : (WT ? ((XL && NB == 1) ? 8 : 4) : ((XL && NB == 1) ? 4 : 2));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int64_t K = p.K;
    const int M = p.M;
    // [M][K + 8]: the 16-B row pad puts the 16 A rows of an MFMA fragment read on
    // distinct LDS banks (an unpadded 7168-B row stride maps every row to one bank)
    const int64_t KP = K + 8;
    uint16_t* xs = reinterpret_cast<uint16_t*>(smem);
    float* red = reinterpret_cast<float*>(smem + (XL ? (size_t)M * KP * 2 : 0));            // [NW - 1][NB][256]
    __shared__ unsigned long long kb_s[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const int arow = fr < M ? fr : M - 1;   // A row of this lane (rows >= M: garbage, never stored)

    auto xa = [&](int64_t k) -> uint4 {   // 8 activations of this lane's A row at k
        return XL ? *reinterpret_cast<const uint4*>(xs + (int64_t)arow * KP + k)
                  : *reinterpret_cast<const uint4*>(p.x + (int64_t)arow * p.ldx + k);
    };

    // segment pointers as laundered byte offsets from one base (see issue()): the
    // result stays a global-address-space pointer derived from that base
    const uint8_t* const wbase = reinterpret_cast<const uint8_t*>(p.w0);
    const uint64_t dw1 = launder_u64((uint64_t)p.w1 - (uint64_t)p.w0);
    const uint64_t dw2 = launder_u64((uint64_t)p.w2 - (uint64_t)p.w0);
    const uint8_t* const bbase = reinterpret_cast<const uint8_t*>(p.x);
    auto boff = [&](const uint16_t* b) { return launder_u64(b ? (uint64_t)b - (uint64_t)p.x : 0ull); };
    const uint64_t db0 = boff(p.b0), db1 = boff(p.b1), db2 = boff(p.b2);
    const uint64_t hb0 = launder_u64(p.b0 ? ~0ull : 0ull), hb1 = launder_u64(p.b1 ? ~0ull : 0ull),
                   hb2 = launder_u64(p.b2 ? ~0ull : 0ull);   // segment has a bias (all-ones mask)
    // this wave's K range, in 16-byte load units; a tile is NBAT steps of U units
    const int64_t units = K / KSTEP;
    const int64_t uw = (units + NW - 1) / NW;
    const int64_t ub = wave * uw, ue = ub + uw < units ? ub + uw : units;
    const int64_t nbat = (uw + U - 1) / U;
    const int64_t n_tiles = (p.N + 15) / 16;
    if ((int64_t)blockIdx.x >= n_tiles) return;   // block-uniform, before any barrier
    const int64_t my_tiles = (n_tiles - 1 - blockIdx.x) / gridDim.x + 1;
    const int64_t S = my_tiles * nbat;            // steps of this block (same for every wave)
    unsigned long long kbest[4] = {0ull, 0ull, 0ull, 0ull};   // rows 4 g + r

    // One step = U units of every B tile of one column tile, plus that tile's epilogue
    // operands (row scales, bias / residual values), all loaded unconditionally so no
    // global load sits under a branch: the steps form one stream per wave, double-
    // buffered in registers, so the next step's loads (next tile included) are in
    // flight while this step's MFMAs, the cross-wave reduction and the epilogue run.
    constexpr int AW = KSTEP / 32;   // 16-B A fragments per unit (8 k each, from k KSTEP/4 * g)
    constexpr int EB = WT ? 1 : 2;
    struct Step {
        u32x4 wv[U][NB][WV];
        uint4 av[XL ? 1 : U][AW];
        float wsc[NB];
        float ep[4];       // residual values (rows 4 g + r) or the bias (ep[0])
        int64_t u0, tile;
        bool last;         // last step of its tile
    };
    auto issue = [&](Step& st, int64_t s) {
        s = s < S ? s : S - 1;
        const int32_t tl = (int32_t)s / (int32_t)nbat, j = (int32_t)s - tl * (int32_t)nbat;   // < 2^31 steps
        st.tile = blockIdx.x + tl * gridDim.x;
        st.u0 = ub + j * U;
        st.last = j == nbat - 1;
        const int64_t n = st.tile * 16 + fr;
        const int64_t nc = n < p.N ? n : p.N - 1;
        const uint8_t* wrow[NB];
        const uint8_t* wseg[NB];   // segment bases (the 16-row tiled fp8 layout)
        const float* scp[NB];
        int64_t r = nc;    // row within the column's segment
        if constexpr (NB == 2) {
            wseg[0] = wbase;
            wseg[1] = wbase + dw1;
            wrow[0] = wbase + nc * K * EB;
            wrow[1] = wbase + dw1 + nc * K * EB;
            scp[0] = reinterpret_cast<const float*>(wbase + p.N * K) + nc;
            scp[1] = reinterpret_cast<const float*>(wbase + dw1 + p.N * K) + nc;
        } else {
            // segment resolved by integer selects on laundered (register) pointers: a
            // select between two kernel-argument loads would become a per-lane load
            const bool s0 = nc < p.n0, s1 = !s0 && nc < p.n01;
            r = s0 ? nc : (s1 ? nc - p.n0 : nc - p.n01);
            const uint64_t m0 = 0ull - (uint64_t)s0, m1 = 0ull - (uint64_t)s1, m2 = ~(m0 | m1);
            const uint8_t* wb = wbase + ((dw1 & m1) | (dw2 & m2));
            (void)m0;
            const int64_t rows = s0 ? p.n0 : (s1 ? p.n01 - p.n0 : p.N - p.n01);
            wseg[0] = wb;
            wrow[0] = wb + r * K * EB;
            scp[0] = reinterpret_cast<const float*>(wb + rows * K) + r;
        }
        if constexpr (WT != 0) {
#pragma unroll
            for (int b = 0; b < NB; b++) st.wsc[b] = *scp[b];
        }
        if constexpr (EPI == QIE_EPI_RESIDUAL) {
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int i = 4 * g + rr < M ? 4 * g + rr : M - 1;
                st.ep[rr] = bf2f(p.y[(int64_t)i * p.ldy + nc]);
            }
        } else if constexpr (EPI == QIE_EPI_STORE) {
            // bias: always loaded (a missing segment bias reads x[0] and is multiplied by 0)
            const bool s0 = nc < p.n0, s1 = !s0 && nc < p.n01;
            const uint64_t m0 = 0ull - (uint64_t)s0, m1 = 0ull - (uint64_t)s1, m2 = ~(m0 | m1);
            const uint8_t* bb = bbase + ((db0 & m0) | (db1 & m1) | (db2 & m2));
            const uint64_t hb = (hb0 & m0) | (hb1 & m1) | (hb2 & m2);
            const uint16_t v = *(reinterpret_cast<const uint16_t*>(bb) + (r & (int64_t)hb));
            st.ep[0] = __uint_as_float((uint32_t)hb & __float_as_uint(bf2f(v)));
        }
        // fp8: lane (fr, g)'s 16 codes of unit uu — plain rows: bytes uu * 64 + 16 g of its row;
        // 16-row tiled (p.t16): bytes (fr + 16 g) * 16 of the unit's 1-KiB block, so one load
        // instruction reads 8 whole lines instead of 16 rows x 64 B (tiles start at segment
        // starts; a clamped row past N stays inside its segment's last tile)
        const uint8_t* lb[NB];
        int64_t ls = KSTEP * EB;
        if constexpr (WT != 0) {
#pragma unroll
            for (int b = 0; b < NB; b++)
                lb[b] = p.t16 ? wseg[b] + (r >> 4) * 16 * K + ((r & 15) + 16 * g) * 16 : wrow[b] + 16 * g;
            ls = p.t16 ? 1024 : KSTEP;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t uu = st.u0 + u < ue ? st.u0 + u : ue - 1;
#pragma unroll
            for (int b = 0; b < NB; b++)   // bytes [uu * KSTEP * EB + 16 WV g, +16 WV) of the row
#pragma unroll
                for (int h = 0; h < WV; h++) {
                    if constexpr (WT != 0)
                        st.wv[u][b][h] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(lb[b] + uu * ls));
                    else
                        st.wv[u][b][h] =
                            __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[b]) + uu * (4 * WV) + WV * g + h);
                }
            if constexpr (!XL) {
                const int64_t kk = uu * KSTEP + (KSTEP / 4) * g;
#pragma unroll
                for (int h = 0; h < AW; h++) st.av[u][h] = xa(kk + 8 * h);
            }
        }
    };
    f32x4_t acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // full: every unit of the step is inside this wave's K range (all but a range's last
    // step), so no per-unit masking; otherwise dead units multiply a zero A fragment
    auto compute = [&](const Step& st, bool full) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool live = full || st.u0 + u < ue;
            const int64_t uu = live ? st.u0 + u : ue - 1;
            const int64_t kk = uu * KSTEP + (KSTEP / 4) * g;
            uint4 ar[AW];
#pragma unroll
            for (int h = 0; h < AW; h++) {
                const uint4 v = XL ? xa(kk + 8 * h) : st.av[XL ? 0 : u][h];
                ar[h] = live ? v : make_uint4(0, 0, 0, 0);
            }
            if constexpr (WT == 0) {
                const bf16x8_t a0 = __builtin_bit_cast(bf16x8_t, ar[0]);
                const bf16x8_t a1 = __builtin_bit_cast(bf16x8_t, ar[1]);
#pragma unroll
                for (int b = 0; b < NB; b++) {
                    acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, __builtin_bit_cast(bf16x8_t, st.wv[u][b][0]),
                                                                     acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, __builtin_bit_cast(bf16x8_t, st.wv[u][b][1]),
                                                                     acc[b], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int h = 0; h < WV; h++) {   // 16 codes: A fragments 2h (codes 0..7), 2h + 1 (8..15)
                    const bf16x8_t a0 = __builtin_bit_cast(bf16x8_t, ar[2 * h]);
                    const bf16x8_t a1 = __builtin_bit_cast(bf16x8_t, ar[2 * h + 1]);
#pragma unroll
                    for (int b = 0; b < NB; b++) {
                        const uint2 c0 = fp8x4_to_bf16x4(st.wv[u][b][h].x), c1 = fp8x4_to_bf16x4(st.wv[u][b][h].y);
                        const uint2 c2 = fp8x4_to_bf16x4(st.wv[u][b][h].z), c3 = fp8x4_to_bf16x4(st.wv[u][b][h].w);
                        const uint4 lo = make_uint4(c0.x, c0.y, c1.x, c1.y);
                        const uint4 hi = make_uint4(c2.x, c2.y, c3.x, c3.y);
                        acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, __builtin_bit_cast(bf16x8_t, lo), acc[b],
                                                                         0, 0, 0);
                        acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, __builtin_bit_cast(bf16x8_t, hi), acc[b],
                                                                         0, 0, 0);
                    }
                }
            }
        }
    };
    // ---- end of a tile: sum the 4 waves' partial tiles (C map: col = fr, rows 4 g + r),
    // epilogue by wave 0.  The barriers wait on LDS only (no vmcnt), so the prefetched
    // next step stays in flight.
    auto tile_end = [&](const Step& st) {
        // waves 1.. publish (wave 0 keeps its partial in registers: NW - 1 tiles of LDS,
        // which keeps config 4's staged gate/up launch within 64 KiB of dynamic LDS)
        if (wave > 0) {
#pragma unroll
            for (int b = 0; b < NB; b++)
                *reinterpret_cast<float4*>(&red[((wave - 1) * NB + b) * 256 + lane * 4]) =
                    make_float4(acc[b][0], acc[b][1], acc[b][2], acc[b][3]);
        }
        __syncthreads();
        if (wave == 0) {
            const int64_t n = st.tile * 16 + fr;
            float c[NB][4];
#pragma unroll
            for (int b = 0; b < NB; b++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                {
                    float t = acc[b][r];   // same order as before: wave 0, then 1 .. NW - 1
#pragma unroll
                    for (int w = 1; w < NW; w++) t += red[((w - 1) * NB + b) * 256 + lane * 4 + r];
                    c[b][r] = t;
                }
            if constexpr (WT != 0) {
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int r = 0; r < 4; r++) c[b][r] *= st.wsc[b];
            }
            emit_tile16<EPI>(c, st.ep, p.y, p.ldy, M, p.N, n, g, p.keys, p.key_col0, kbest);
        }
#pragma unroll
        for (int b = 0; b < NB; b++) acc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        __syncthreads();   // red[] reused by the next tile
    };

    // steady state issues unconditionally (a load under a branch costs a vmcnt(0) at the
    // join); the last one or two steps are peeled so nothing past step S - 1 is fetched
    Step sa, sb;
    issue(sa, 0);
    // ---------------- prologue: the M activation rows -> LDS (optionally RMS-normed).  It runs
    // AFTER the first step's weight loads are issued (weights do not depend on x), so the
    // weight stream's first HBM round trip overlaps the prologue's loads and reductions.
    if (XL && !QIE_DBG(p.dbg & 4)) {
        if (p.norm_w && !QIE_DBG(p.dbg & 1)) {
            // pass 1: every row's sum of squares at once (loads of all rows in flight,
            // clamped rows past M), ONE exchange — not a barrier pair per row
            float ss[16];
#pragma unroll
            for (int m = 0; m < 16; m++) ss[m] = 0.f;
            for (int64_t k = tid * 8; k < K; k += NW * 512) {
                uint4 v[16];
#pragma unroll
                for (int m = 0; m < 16; m++)
                    v[m] = *reinterpret_cast<const uint4*>(p.x + (int64_t)(m < M ? m : M - 1) * p.ldx + k);
#pragma unroll
                for (int m = 0; m < 16; m++) {
                    if (m >= M) continue;   // uniform, ALU only (the loads are above)
                    float f[8];
                    unpack8(u32x4{v[m].x, v[m].y, v[m].z, v[m].w}, f);
#pragma unroll
                    for (int j = 0; j < 8; j++) ss[m] += f[j] * f[j];
                }
            }
#pragma unroll
            for (int m = 0; m < 16; m++) {
                if (m >= M) continue;
                const float t = wave_sum(ss[m]);
                if (lane == 0) red[wave * 16 + m] = t;
            }
            __syncthreads();
            const bool hf = p.numerics == QIE_NUMERICS_HF;
            float rms[16], inv[16];
#pragma unroll
            for (int m = 0; m < 16; m++) {
                const int mm = m < M ? m : 0;
                float sm = red[mm];
#pragma unroll
                for (int w = 1; w < NW; w++) sm += red[16 * w + mm];
                rms[m] = sqrtf((sm / (float)K) + p.eps);
                inv[m] = 1.0f / rms[m];
            }
            // pass 2: all rows of a chunk at once (loads unconditional and clamped; the
            // per-row math under uniform branches).  REF's f / rms is div_mk (qie_common.hpp).
            for (int64_t k = tid * 8; k < K; k += NW * 512) {
                const uint4 nw = *reinterpret_cast<const uint4*>(p.norm_w + k);
                uint4 v[16];
#pragma unroll
                for (int m = 0; m < 16; m++)
                    v[m] = *reinterpret_cast<const uint4*>(p.x + (int64_t)(m < M ? m : M - 1) * p.ldx + k);
                float wf[8];
                unpack8(u32x4{nw.x, nw.y, nw.z, nw.w}, wf);
#pragma unroll
                for (int m = 0; m < 16; m++) {
                    if (m >= M) continue;
                    float f[8];
                    unpack8(v[m], f);
                    *reinterpret_cast<uint4*>(xs + (int64_t)m * KP + k) = rms_apply8(f, wf, rms[m], inv[m], hf, true);
                }
            }
        } else {
            for (int m = 0; m < M; m++)
                for (int64_t k = tid * 8; k < K; k += NW * 512)
                    *reinterpret_cast<uint4*>(xs + (int64_t)m * KP + k) =
                        *reinterpret_cast<const uint4*>(p.x + (int64_t)m * p.ldx + k);
        }
        __syncthreads();
    }
    if (QIE_DBG(p.dbg & 2)) {
        if (tid == 0 && p.dbg == 0x7fffffff) p.y[0] = xs[0];
        return;
    }
    auto run = [&](const Step& st) {   // the full/tail choice is wave-uniform
        if (st.u0 + U <= ue) compute(st, true);
        else compute(st, false);
    };
    int64_t s = 0;
    for (; s + 2 < S; s += 2) {
        issue(sb, s + 1);
        run(sa);
        if (sa.last) tile_end(sa);
        issue(sa, s + 2);
        run(sb);
        if (sb.last) tile_end(sb);
    }
    if (S - s == 2) {
        issue(sb, s + 1);
        run(sa);
        if (sa.last) tile_end(sa);
        run(sb);
        tile_end(sb);
    } else {
        run(sa);
        tile_end(sa);
    }
    if constexpr (EPI == QIE_EPI_STORE) {
        if (p.keys && wave == 0) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                unsigned long long v = kbest[r];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {   // max over the 16 columns of row 4 g + r
                    const unsigned long long t = __shfl_xor(v, o, 64);
                    v = t > v ? t : v;
                }
                if (fr == 0 && 4 * g + r < M && v) atomicMax(p.keys + 4 * g + r, v);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Host side: plan_linear (linear_plan.hpp) decides, the launchers below map the plan to an
// instantiation and launch it on launch_geometry's grid.

// The dev knobs of the plan, read in one place (development build: the environment at every
// call, so a tool may change a knob between launches; shipped library: the defaults).
static Knobs dev_knobs() {
    Knobs k;
    k.epre = dev_env("QIE_GEMV_EPRE", k.epre);
    k.mkdiv = dev_env("QIE_GEMV_MKDIV", k.mkdiv);
    k.gemv_dbg = dev_env("QIE_GEMV_DBG", k.gemv_dbg);
    k.blocks_per_cu = dev_env("QIE_GEMV_BLOCKS_PER_CU", k.blocks_per_cu);
    k.xfirst = dev_env("QIE_GEMV_XFIRST", k.xfirst);
    k.xreg = dev_env("QIE_GEMV_XREG", k.xreg);
    k.xreg4 = dev_env("QIE_GEMV_XREG4", k.xreg4);
    k.xreg4_lm = dev_env("QIE_GEMV_XREG4_LM", k.xreg4_lm);
    k.xreg4_sw = dev_env("QIE_GEMV_XREG4_SW", k.xreg4_sw);
    k.swiglu_bpc = dev_env("QIE_GEMV_SWIGLU_BPC", k.swiglu_bpc);
    k.lm_bpc = dev_env("QIE_GEMV_LM_BPC", k.lm_bpc);
    k.res_bpc = dev_env("QIE_GEMV_RES_BPC", k.res_bpc);
    k.qkv_bpc = dev_env("QIE_GEMV_QKV_BPC", k.qkv_bpc);
    k.balanced = dev_env("QIE_GEMV_BALANCED", k.balanced);
    k.rpw1 = dev_env("QIE_GEMV_RPW1", k.rpw1);
    k.skinny_mfma = dev_env("QIE_SKINNY_MFMA", k.skinny_mfma);
    k.skinny_lds64 = dev_env("QIE_SKINNY_LDS64", k.skinny_lds64);
    k.skinny_xl = dev_env("QIE_SKINNY_XL", k.skinny_xl);
    k.skinny_dbg = dev_env("QIE_SKINNY_DBG", k.skinny_dbg);
    k.skinny_bpc = dev_env("QIE_SKINNY_BPC", k.skinny_bpc);
    k.dec8 = dev_env("QIE_DEC8", k.dec8);
    k.dec8_split = dev_env("QIE_DEC8_SPLIT", k.dec8_split);
    k.dec8_split_ku = dev_env("QIE_DEC8_SPLIT_KU", k.dec8_split_ku);
    k.t16_skinny = dev_env("QIE_T16_SKINNY", k.t16_skinny);
    return k;
}

// dynamic LDS above 64 KiB (x staged at K > 32 Ki): the kernels' limit is raised to 160 KiB
static size_t gemv_lds_limit(size_t shm) { return shm > 65536 ? 160 * 1024 : 0; }

template <int MT, int RPW, int EPI, int XCH, int WT, int UO = 0>
static int launch_gemv_t(const GemvParams& p, const LinearPlan& pl, hipStream_t st) {
    constexpr int U = UO ? UO : 8;
    const void* fn = (const void*)gemv_kernel<MT, RPW, EPI, U, XCH, WT>;
    if (pl.block_waves) {   // one block per CU: the instantiation bounded at its block size
        if constexpr (MT == 1 && WT == 0 && EPI != QIE_EPI_SWIGLU) {
            constexpr int LBB = RPW == 1 ? 1024 : kGemvBalancedThreads;
            const LaunchGeom g = launch_geometry(pl, device_cu_count(), 0);
            QIE_TRY(raise_dynamic_lds((const void*)gemv_kernel<MT, RPW, EPI, U, XCH, WT, LBB>, gemv_lds_limit(g.lds_bytes)));
            hipLaunchKernelGGL((gemv_kernel<MT, RPW, EPI, U, XCH, WT, LBB>), dim3(g.grid), dim3(g.threads), g.lds_bytes,
                               st, p);
            QIE_LAUNCH_CHECK();
            return 0;
        }
    }
    QIE_TRY(raise_dynamic_lds(fn, gemv_lds_limit(pl.lds_bytes)));
    const int nb = pl.needs_occupancy() ? resident_blocks_per_cu(fn, 256, pl.lds_bytes, 2) : 0;
    const LaunchGeom g = launch_geometry(pl, device_cu_count(), nb);
    hipLaunchKernelGGL((gemv_kernel<MT, RPW, EPI, U, XCH, WT>), dim3(g.grid), dim3(g.threads), g.lds_bytes, st, p);
    QIE_LAUNCH_CHECK();
    return 0;
}

template <int MT, int XCH, int WT = 0, int UO = 0>
static int launch_gemv_m(const GemvParams& p, const LinearPlan& pl, hipStream_t st) {
    if constexpr (MT == 1 && XCH == 1 && WT == 0) {   // one row per wave (O / down, x beside the weights)
        if (pl.rpw == 1 && pl.epi == QIE_EPI_RESIDUAL) return launch_gemv_t<1, 1, QIE_EPI_RESIDUAL, 1, 0, UO>(p, pl, st);
        if (pl.rpw == 1 && pl.epi == QIE_EPI_STORE) return launch_gemv_t<1, 1, QIE_EPI_STORE, 1, 0, UO>(p, pl, st);
    }
    return dispatch_epi(pl.epi, [&](auto E) {
        constexpr int EPI = decltype(E)::value;
        return launch_gemv_t<MT, 2, EPI, XCH, WT, UO>(p, pl, st);
    });
}

// plan -> instantiation: every <MT, XCH, WT, UO> the library compiles (rows per wave and the
// epilogue are launch_gemv_m's)
constexpr int gemv_key(int mt, int xch, int wt, int uo) { return ((mt * 16 + xch) * 2 + wt) * 16 + uo; }
static int launch_gemv(const GemvParams& p, const LinearPlan& pl, hipStream_t st) {
#define QIE_GEMV_CASE(MT, XCH, WT, UO) \
    case gemv_key(MT, XCH, WT, UO): return launch_gemv_m<MT, XCH, WT, UO>(p, pl, st)
    switch (gemv_key(pl.mt, pl.xch, pl.wt, pl.uo)) {
        // fp8 weights, and 2..8 bf16 rows: the generic prologue
        QIE_GEMV_CASE(1, 0, 1, 0);
        QIE_GEMV_CASE(2, 0, 1, 0);
        QIE_GEMV_CASE(4, 0, 1, 0);
        QIE_GEMV_CASE(8, 0, 1, 0);
        QIE_GEMV_CASE(2, 0, 0, 0);
        QIE_GEMV_CASE(4, 0, 0, 0);
        QIE_GEMV_CASE(8, 0, 0, 0);
        // one bf16 row: the x-first variants (XCH 2048-element x chunks per thread), x beside
        // the weights (1), x in registers (3, 4); UO as gemv_uo sizes it
        QIE_GEMV_CASE(1, 0, 0, 0);
        QIE_GEMV_CASE(1, 1, 0, 0);
        QIE_GEMV_CASE(1, 1, 0, 7);
        QIE_GEMV_CASE(1, 2, 0, 0);
        QIE_GEMV_CASE(1, 2, 0, 2);
        QIE_GEMV_CASE(1, 2, 0, 7);
        QIE_GEMV_CASE(1, 3, 0, 2);
        QIE_GEMV_CASE(1, 3, 0, 7);
        QIE_GEMV_CASE(1, 3, 0, 8);
        QIE_GEMV_CASE(1, 4, 0, 2);
        QIE_GEMV_CASE(1, 4, 0, 7);
        QIE_GEMV_CASE(1, 4, 0, 8);
        QIE_GEMV_CASE(1, 5, 0, 0);
        QIE_GEMV_CASE(1, 5, 0, 5);
        QIE_GEMV_CASE(1, 10, 0, 0);
        QIE_GEMV_CASE(1, 10, 0, 5);
        QIE_GEMV_CASE(1, 10, 0, 7);
    }
#undef QIE_GEMV_CASE
    return fail(-22, "qie_linear: internal: no GEMV instantiation for MT=%d XCH=%d WT=%d UO=%d", pl.mt, pl.xch, pl.wt,
                pl.uo);
}

template <int EPI, int WT, int XL, int NW, int UO = 0>
static int launch_skinny_x(const GemvParams& p, const LinearPlan& pl, hipStream_t st) {
    const void* fn = (const void*)skinny_mfma_kernel<EPI, WT, XL, NW, UO>;
    QIE_TRY(raise_dynamic_lds(fn, gemv_lds_limit(pl.lds_bytes)));
    const int nb = pl.needs_occupancy() ? resident_blocks_per_cu(fn, NW * 64, pl.lds_bytes, 1) : 0;
    const LaunchGeom g = launch_geometry(pl, device_cu_count(), nb);
    hipLaunchKernelGGL((skinny_mfma_kernel<EPI, WT, XL, NW, UO>), dim3(g.grid), dim3(NW * 64), g.lds_bytes, st, p);
    QIE_LAUNCH_CHECK();
    return 0;
}
// 4 waves per block: 8 (2,304 waves for Qwen2-7B QKV) measured 1-9 % slower at config 4,
// 16 spills (128 VGPRs at 1,024 threads)
static int launch_skinny(const GemvParams& p, const LinearPlan& pl, hipStream_t st) {
    return dispatch_epi(pl.epi, [&](auto E) {
        constexpr int EPI = decltype(E)::value;
        if (pl.wt && pl.uo == 7)
            return pl.xlds ? launch_skinny_x<EPI, 1, 1, 4, 7>(p, pl, st) : launch_skinny_x<EPI, 1, 0, 4, 7>(p, pl, st);
        if (pl.wt) return pl.xlds ? launch_skinny_x<EPI, 1, 1, 4>(p, pl, st) : launch_skinny_x<EPI, 1, 0, 4>(p, pl, st);
        return pl.xlds ? launch_skinny_x<EPI, 0, 1, 4>(p, pl, st) : launch_skinny_x<EPI, 0, 0, 4>(p, pl, st);
    });
}

int gemm(const qie_linear_args* a, hipStream_t st);
int dec8_linear(const qie_linear_args* a, const LinearPlan& pl, hipStream_t st, bool* done);
int dec4_linear(const qie_linear_args* a, const LinearPlan& pl, hipStream_t st);

// true when the MXFP4 kernel takes this projection (the engine then skips its separate norm)
bool dec4_applies(const qie_linear_args* a) {
    int ku, ks, parts;
    return dec4_plan(*a, &ku, &ks, &parts) == PlanError::None;
}

// true when the fp8 batched-decode kernel takes this projection (the engine then skips its
// separate norm)
bool dec8_applies(const qie_linear_args* a) {
    int ku, ks, parts;
    return dec8_plan(*a, dev_knobs(), &ku, &ks, &parts);
}

// qie_debug_linear_plan: the launch qie_linear would make of *a on the current device (its CU
// count, this library's knobs), in plan_format.hpp's wording.  No launch and no occupancy query:
// a grid that depends on one prints as "grid=?".  (A split-K workspace that cannot be had
// during a graph capture makes gemv() / gemm() plan again without one; this is the first plan.)
int linear_plan_text(const qie_linear_args* a, char* out, int cap) {
    QIE_REQUIRE(a && out && cap > 0, "qie_debug_linear_plan: bad arguments");
    const std::string s = format_linear_plan(*a, dev_knobs(), dev_gemm_knobs(), device_cu_count(), 0);
    QIE_REQUIRE((size_t)cap > s.size(), "qie_debug_linear_plan: %zu bytes needed", s.size() + 1);
    memcpy(out, s.c_str(), s.size() + 1);
    return 0;
}

// M <= 16: plan, fill the kernel's argument block, launch the plan's instantiation
static int gemv(const qie_linear_args* a, const LinearExtras& ex, hipStream_t st) {
    if (ex.push_taken) *ex.push_taken = false;
    const Knobs k = dev_knobs();
    const int cus = device_cu_count();
    LinearPlan pl = plan_linear(*a, ex, cus, k);
    if (pl.family == LinearFamily::Dec4) {   // MXFP4 weights: one kernel or a refusal
        switch (pl.error) {
            case PlanError::None: return dec4_linear(a, pl, st);
            case PlanError::Fp4Flags:
                return fail(-22, "qie_linear: fp4 weights: flags %d combine QIE_LINEAR_FP4 with fp8 weights / activations "
                                 "(or name the tiled layout without QIE_LINEAR_FP4)", a->flags);
            case PlanError::Fp4Rows:
                return fail(-22, "qie_linear: fp4 weights are read at 1 <= M <= 16 rows only (M=%lld): larger M runs on "
                                 "the dequantised bf16 weights", (long long)a->M);
            case PlanError::Fp4K:
                return fail(-22, "qie_linear: fp4 weights need K %% 128 == 0 (K=%lld)", (long long)a->K);
            default:
                return fail(-22, "qie_linear: fp4 weights: the MXFP4 kernel does not take M=%lld K=%lld N=%lld epilogue %d "
                                 "(N <= 32768, segments of whole 16-column tiles, K <= 8192 or split-K without norm / "
                                 "SWIGLU / segments up to K 32768)", (long long)a->M, (long long)a->K, (long long)a->N,
                            a->epilogue);
        }
    }
    if (pl.family == LinearFamily::Dec8) {
        bool done = false;
        const int rc = dec8_linear(a, pl, st, &done);
        if (done) return rc;
        pl = plan_linear(*a, ex, cus, k, false);
    }
    switch (pl.error) {
        case PlanError::None: break;
        case PlanError::TiledShape:
            return fail(-22, "qie_linear: tiled fp8 weights: the skinny kernel cannot take M=%lld K=%lld", (long long)a->M,
                        (long long)a->K);
        case PlanError::NormLds:
            return fail(-22, "qie_linear: fused RMSNorm needs M*K*2 <= %zu bytes (M=%lld K=%lld)", kGemvLdsCap,
                        (long long)a->M, (long long)a->K);
        case PlanError::Fp8K16:
            return fail(-22, "qie_linear: fp8 weights need K %% 16 == 0 (K=%lld)", (long long)a->K);
        case PlanError::NormRouted:
            return fail(-22, "qie_linear: internal: fused norm routed to a variant without one");
        default: return fail(-22, "qie_linear: internal: plan error %d", (int)pl.error);
    }
    if (pl.family == LinearFamily::Gemm) return gemm(a, st);
    GemvParams p;
    p.x = (const uint16_t*)a->x;
    p.ldx = a->ldx;
    p.w0 = (const uint16_t*)a->w[0];
    p.w1 = (const uint16_t*)a->w[1];
    p.w2 = (const uint16_t*)a->w[2];
    p.b0 = (const uint16_t*)a->bias[0];
    p.b1 = (const uint16_t*)a->bias[1];
    p.b2 = (const uint16_t*)a->bias[2];
    p.n0 = a->seg_rows[0];
    p.n01 = a->seg_rows[0] + a->seg_rows[1];
    p.K = a->K;
    p.N = a->N;
    p.y = (uint16_t*)a->y;
    p.ldy = a->ldy;
    p.norm_w = (const uint16_t*)a->norm_w;
    p.eps = a->norm_eps;
    p.numerics = a->numerics;
    p.M = (int)a->M;
    p.xlds = pl.xlds;
    p.keys = (unsigned long long*)a->argmax_keys;
    p.key_col0 = a->key_col0;
    p.n_tasks = pl.n_tasks;
    p.dbg = pl.dbg;
    p.rope_pos = ex.rope.pos;
    p.rope_cs = ex.rope.cs;
    p.rope_sn = ex.rope.sn;
    p.rope_hd = ex.rope.hd;
    p.rope_rows = ex.rope.rows;
    p.epre = k.epre;
    p.mkdiv = k.mkdiv;
    p.t16 = pl.t16 ? 1 : 0;
    p.push = PeerPush{};
    if (pl.push) {
        p.push = *ex.push;
        if (ex.push_taken) *ex.push_taken = true;
    }
    return pl.family == LinearFamily::Skinny ? launch_skinny(p, pl, st) : launch_gemv(p, pl, st);
}

// qie_linear behind its C entry: validates, then routes.  Callers inside the library pass what
// the public argument block cannot hold in `ex`: the decode QKV projection's fused RoPE (M = 1,
// REF numerics, no qk-norm: the interleaved RoPE of its q and k rows in the STORE epilogue,
// RoPE.cu:6-22 on the projection's bf16 output — the decode attention then takes q / k as they
// are, QIE_ATTN_PREROPED) and the row-parallel projections' peer push.
int linear(const qie_linear_args* a, const LinearExtras& ex, hipStream_t st) {
    QIE_REQUIRE(a && a->x && a->y && a->w[0] && a->M > 0 && a->K > 0 && a->N > 0, "qie_linear: bad arguments");
    QIE_REQUIRE(a->K % 8 == 0 && a->ldx >= a->K && a->ldx % 8 == 0, "qie_linear: K and ldx must be multiples of 8");
    QIE_REQUIRE(((uintptr_t)a->x % 16) == 0, "qie_linear: x must be 16-byte aligned");
    for (int i = 0; i < 3; i++)
        QIE_REQUIRE(((uintptr_t)a->w[i] % 16) == 0, "qie_linear: weight segment %d must be 16-byte aligned", i);
    if (a->epilogue == QIE_EPI_SWIGLU) {
        QIE_REQUIRE(a->w[1] && a->seg_rows[0] == a->N && a->seg_rows[1] == a->N && a->ldy >= a->N,
                    "qie_linear: SWIGLU needs w[0]=gate, w[1]=up with N rows each");
    } else {
        QIE_REQUIRE(a->seg_rows[0] + a->seg_rows[1] + a->seg_rows[2] == a->N && a->ldy >= a->N,
                    "qie_linear: seg_rows must sum to N");
        QIE_REQUIRE(a->seg_rows[1] == 0 || a->w[1], "qie_linear: missing weight segment 1");
        QIE_REQUIRE(a->seg_rows[2] == 0 || a->w[2], "qie_linear: missing weight segment 2");
    }
    QIE_REQUIRE(a->epilogue >= 0 && a->epilogue <= 3, "qie_linear: bad epilogue");
    QIE_REQUIRE(a->epilogue != QIE_EPI_F32 || (a->bias[0] == nullptr && a->bias[1] == nullptr && a->bias[2] == nullptr),
                "qie_linear: F32 (partial-sum) epilogue takes no bias");
    QIE_REQUIRE(a->argmax_keys == nullptr || a->epilogue == QIE_EPI_STORE, "qie_linear: arg-max needs STORE");
    QIE_REQUIRE(!(ex.rope.pos || ex.rope.rows) ||
                    (a->M == 1 && a->epilogue == QIE_EPI_STORE && ex.rope.rows % 2 == 0 && ex.rope.hd % 2 == 0 &&
                     ex.rope.pos && ex.rope.cs && ex.rope.sn),
                "qie_linear: fused RoPE: M = 1 STORE projections only");
    if (ex.push_taken) *ex.push_taken = false;
    // MXFP4 weights have one reader: the planner takes the launch or names the refusal, at any M
    if (a->flags & (QIE_LINEAR_FP4 | QIE_LINEAR_FP4_T16)) {
        // (a peer push in the extras is left untaken, as the fp8 kernels leave it: *push_taken stays
        // false and the caller runs its exchange; a fused RoPE would be dropped silently, so it is
        // refused -- the engine does not ask for one on fp4 weights, rope_in_projection)
        QIE_REQUIRE(!(ex.rope.pos || ex.rope.rows), "qie_linear: fp4 weights take no fused RoPE");
        return gemv(a, ex, st);
    }
    if (a->flags & QIE_LINEAR_ACT_FP8) return gemm(a, st);   // fp8 activations: the block-scaled MFMA GEMM at every M
    QIE_REQUIRE(!(a->flags & QIE_LINEAR_FP8_T16) ||
                    ((a->flags & QIE_LINEAR_FP8) && a->M >= 1 && a->M <= 16 && a->K % 64 == 0 &&
                     (a->epilogue == QIE_EPI_SWIGLU ? a->N % 16 == 0
                                                    : a->seg_rows[0] % 16 == 0 && a->seg_rows[1] % 16 == 0 &&
                                                          a->seg_rows[2] % 16 == 0)),
                "qie_linear: 16-row tiled fp8 weights are read by the batched-decode kernels only (M <= 16, K %% 64 == 0, "
                "segments of whole 16-row tiles) and, with fp8 activations, the block-scaled GEMM");
    if (a->M <= 16) return gemv(a, ex, st);   // GEMV (M = 1..8) or the skinny MFMA kernel (2..16)
    return gemm(a, st);
}

}  // namespace qie

