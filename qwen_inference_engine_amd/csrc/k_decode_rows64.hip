// k_decode_rows64.hip — decode projections of 17 <= M <= 64 rows (QIE_LINEAR_ROWS64): a
// weight-streaming MFMA GEMM for the batched decode step of more than 16 slots.
//
// Replaces matrix_mul (layers/src/matrix_mul.cu:165-288) where the M <= 16 kernels (k_gemv.hip,
// k_decode_fp8.hip) stop and the prefill GEMMs (k_gemm.hip, tiled for M >= 256) would re-stage
// the weights through LDS for at most 64 useful rows.  Here a weight byte goes from HBM into a
// register once per launch and is an MFMA operand for every row tile:
//   * a workgroup of 4 waves owns 64 output columns; wave w owns the 16-column tile w (SWIGLU:
//     its gate and its up tile) for ALL M rows: MT = 2, 3 or 4 accumulator tiles of 16 rows, so one
//     weight fragment (16 rows x 16 k per lane quarter) feeds 2 MT MFMAs;
//   * weights: non-temporal 16-B buffer loads straight into registers, one chunk (256 columns)
//     ahead of the MFMAs in a second register set — bf16 [N, K] (two loads per 64-k unit), fp8
//     codes (one), or the 16-row tiled fp8 layout whose 1-KiB blocks ARE the fragments of a unit;
//     fp8 codes become bf16 by v_cvt_scalef32_pk_bf16_fp8 and the power-of-two row scale multiplies the sum;
//   * x: the chunk's M x 256 slice is loaded by the whole workgroup (2 MT 16-B vectors per
//     thread, one chunk ahead, rows past M - 1 never read), stored to LDS (row stride 528 B) and
//     read by the four waves as A fragments — x crosses L2 -> CU once per 64 columns instead of
//     once per 16;
//   * K is split over `parts` workgroups (rows64_plan.hpp); parts >= 2: every wave publishes its
//     partial tiles to slab [tile][part] write-through, takes its tile's ticket, and the last
//     arriver adds the parts in part order (whoever it is), resets the ticket and runs the
//     epilogue.  No float atomics, no waiting on another workgroup: two runs are bit-identical.
// Numerics: products of the bf16 rows and the (exactly dequantised) bf16 weights, fp32 sums per
// part in k order (64-column units, two 32-product MFMA steps each), parts in part order, times
// the row scale; the epilogues round as linear_epilogue.hpp's (bf16 after each op).  Row m does
// not depend on M beyond the choice of parts, which depends on the shape only.
#include "qie_common.hpp"
#include "launch_util.hpp"
#include "linear_epilogue.hpp"
#include "rows64_plan.hpp"
#include "../../include/qie/qie_ops.h"

#include <algorithm>
#include <map>
#include <mutex>

namespace qie {

typedef unsigned int r64_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 r64_bf16x8 __attribute__((ext_vector_type(8)));
typedef float r64_f32x4 __attribute__((ext_vector_type(4)));

struct Rows64Params {
    const uint16_t* x;         // [M][ldx] bf16 rows (already normed)
    int64_t ldx;
    const uint8_t* w[3];       // segment bases (bf16 [rows][K]; fp8: codes, then rows fp32 scales)
    const uint16_t* bias[3];   // per segment, may be null
    int32_t seg_rows[3];
    int32_t t01[2];            // tiles in segment 0, in segments 0 + 1
    int32_t K, N, M, n_tiles;
    uint16_t* y;               // [M][ldy]
    int64_t ldy;
    int32_t chunks, parts, cpp;   // rows64_plan.hpp
    float* slab;               // parts >= 2: [tile][part][NB][MT][256] fp32
    unsigned* cnt;             // one ticket per tile, zero at rest
};

// WT: 0 bf16, 1 fp8 plain, 2 fp8 16-row tiled.  Two workgroups per CU (256 VGPRs).
template <int EPI, int WT, int MT>
__global__ __launch_bounds__(kR64Threads, 2) void rows64_kernel(Rows64Params p) {
#pragma clang fp contract(off)
    constexpr int NB = EPI == QIE_EPI_SWIGLU ? 2 : 1;   // weight tiles per column tile (gate, up)
    constexpr int WL = WT == 0 ? 2 : 1;                  // 16-B loads per lane, unit and weight tile
    constexpr int UST = WT == 0 ? 128 : (WT == 1 ? 64 : 1024);   // bytes between a lane's units
    constexpr int kNT = 2;                               // buffer-load policy: nt (streamed once)
    constexpr int kOut = 0x7ffffff0;                     // past every buffer range: the load gives 0
    constexpr int XV = 2 * MT;                           // x vectors per thread and chunk
    __shared__ __attribute__((aligned(16))) uint8_t xs[MT * 16 * kR64RowStride];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int M = p.M, K = p.K, units = K / 64;
    const int part = (int)blockIdx.x % p.parts, cb = (int)blockIdx.x / p.parts;
    // a wave past the last tile (a ragged column block) walks the last tile's weights with the
    // others — it shares their barriers — and leaves before the merge and the epilogue
    const bool live = cb * kR64Waves + wave < p.n_tiles;
    const int tile = live ? cb * kR64Waves + wave : p.n_tiles - 1;
    const int sg = NB == 2 ? 0 : (tile < p.t01[0] ? 0 : (tile < p.t01[1] ? 1 : 2));
    const int tb0 = sg == 0 ? 0 : (sg == 1 ? p.t01[0] : p.t01[1]);
    const int rows = p.seg_rows[sg];
    int r = (tile - tb0) * 16 + fr;   // this lane's weight row in its segment (a ragged last tile: clamped)
    r = r < rows ? r : rows - 1;
    const int c0 = part * p.cpp, c1 = c0 + p.cpp < p.chunks ? c0 + p.cpp : p.chunks;

    // lane (fr, g) of unit u: weight row r, columns 64 u + 16 g + [0, 16)
    const int wbase = WT == 0 ? (r * K + 16 * g) * 2 : (WT == 1 ? r * K + 16 * g : (tile - tb0) * 16 * K + lane * 16);
    auto rsrc = [&](int b) {   // weight tile b's segment as a buffer: loads past it give 0
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.w[NB == 2 ? b : sg]), (short)0,
                                                 (int)((int64_t)rows * (WT == 0 ? 2 * K : K + 4)), 0x00020000);
    };
    struct Step {
        r64_u32x4 wv[NB][4][WL];
    };
    // every load unconditional: a unit past K reads out of the buffer range (zeros)
    auto issue_w = [&](Step& t, int c) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const bool ok = 4 * c + u < units;
            const int off = wbase + (4 * c + u) * UST;
#pragma unroll
            for (int b = 0; b < NB; b++)
#pragma unroll
                for (int h = 0; h < WL; h++)
                    t.wv[b][u][h] = __builtin_amdgcn_raw_buffer_load_b128(rsrc(b), ok ? off + 16 * h : kOut, 0, kNT);
        }
    };
    // thread t's vectors of a chunk: v = t + 256 j -> row v / 32, columns 8 (v % 32) + [0, 8);
    // rows past M - 1 repeat row M - 1 (their accumulator rows are never stored), columns past K are 0
    auto issue_x = [&](r64_u32x4 (&xr)[XV], int c) {
#pragma unroll
        for (int j = 0; j < XV; j++) {
            const int v = tid + kR64Threads * j;
            const int row = (v >> 5) < M ? (v >> 5) : M - 1;
            const int k = c * kR64ChunkK + 8 * (v & 31);
            const r64_u32x4 val = *reinterpret_cast<const r64_u32x4*>(p.x + (int64_t)row * p.ldx + (k < K ? k : K - 8));
            xr[j] = k < K ? val : r64_u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto store_x = [&](const r64_u32x4 (&xr)[XV]) {
#pragma unroll
        for (int j = 0; j < XV; j++) {
            const int v = tid + kR64Threads * j;
            *reinterpret_cast<r64_u32x4*>(xs + (v >> 5) * kR64RowStride + (v & 31) * 16) = xr[j];
        }
    };

    r64_f32x4 acc[NB][MT];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int t = 0; t < MT; t++) acc[b][t] = r64_f32x4{0.f, 0.f, 0.f, 0.f};
    // one chunk from LDS and registers: per unit the weight fragment once, then MT row tiles
    auto compute = [&](const Step& t) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            r64_bf16x8 lo[NB], hi[NB];
#pragma unroll
            for (int b = 0; b < NB; b++) {
                if constexpr (WT == 0) {
                    lo[b] = __builtin_bit_cast(r64_bf16x8, t.wv[b][u][0]);
                    hi[b] = __builtin_bit_cast(r64_bf16x8, t.wv[b][u][WL - 1]);
                } else {
                    const r64_u32x4 wv = t.wv[b][u][0];
                    const uint2 q0 = fp8x4_to_bf16x4(wv.x), q1 = fp8x4_to_bf16x4(wv.y);
                    const uint2 q2 = fp8x4_to_bf16x4(wv.z), q3 = fp8x4_to_bf16x4(wv.w);
                    lo[b] = __builtin_bit_cast(r64_bf16x8, r64_u32x4{q0.x, q0.y, q1.x, q1.y});
                    hi[b] = __builtin_bit_cast(r64_bf16x8, r64_u32x4{q2.x, q2.y, q3.x, q3.y});
                }
            }
#pragma unroll
            for (int tt = 0; tt < MT; tt++) {
                const uint8_t* ap = xs + (16 * tt + fr) * kR64RowStride + (64 * u + 16 * g) * 2;
                const r64_bf16x8 a0 = __builtin_bit_cast(r64_bf16x8, *reinterpret_cast<const r64_u32x4*>(ap));
                const r64_bf16x8 a1 = __builtin_bit_cast(r64_bf16x8, *reinterpret_cast<const r64_u32x4*>(ap + 16));
#pragma unroll
                for (int b = 0; b < NB; b++) {
                    acc[b][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, lo[b], acc[b][tt], 0, 0, 0);
                    acc[b][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, hi[b], acc[b][tt], 0, 0, 0);
                }
            }
        }
    };

    // the walk: chunk c's x goes registers -> LDS between two barriers, the next chunk's x and
    // weights are issued before chunk c is computed (the last step re-issues its own chunk: no
    // load sits under a branch)
    Step sa, sb;
    r64_u32x4 xr[XV];
    issue_x(xr, c0);
    issue_w(sa, c0);
    auto step = [&](const Step& cur, Step& nxt, int c) {
        __syncthreads();   // the waves are done with the previous chunk's rows
        store_x(xr);
        __syncthreads();
        const int cn = c + 1 < c1 ? c + 1 : c;
        issue_x(xr, cn);
        issue_w(nxt, cn);
        compute(cur);
    };
    for (int c = c0;;) {
        step(sa, sb, c);
        if (++c >= c1) break;
        step(sb, sa, c);
        if (++c >= c1) break;
    }
    if (!live) return;   // wave-uniform, after the last barrier

    // ---- split-K: publish, take the ticket; the last arriver sums the parts in part order
    if (p.parts > 1) {
        float* tb = p.slab + (int64_t)tile * p.parts * (NB * MT * 256);
        const auto ss = __builtin_amdgcn_make_buffer_rsrc(tb, (short)0, p.parts * (NB * MT * 1024), 0x00020000);
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int t = 0; t < MT; t++)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(r64_u32x4, acc[b][t]), ss,
                                                       ((part * NB + b) * MT + t) * 1024 + lane * 16, 0, 16);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned old = 0;
        if (lane == 0) old = __hip_atomic_fetch_add(p.cnt + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        old = __shfl(old, 0, 64);
        if (old != (unsigned)p.parts - 1) return;   // wave-uniform
        for (int q = 0; q < p.parts; q++) {
#pragma unroll
            for (int b = 0; b < NB; b++)
#pragma unroll
                for (int t = 0; t < MT; t++) {
                    const r64_f32x4 v = __builtin_bit_cast(
                        r64_f32x4, __builtin_amdgcn_raw_buffer_load_b128(ss, ((q * NB + b) * MT + t) * 1024 + lane * 16, 0, 16));
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[b][t][j] = q == 0 ? v[j] : acc[b][t][j] + v[j];
                }
        }
        if (lane == 0) __hip_atomic_store(p.cnt + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    // ---- epilogue: column n of this lane, rows 16 t + 4 g + [0, 4) of every row tile
    float sc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++)
        sc[b] = WT == 0 ? 1.f : __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc(b), rows * K + r * 4, 0, 0));
    const int n = tile * 16 + fr;
    const int nc = n < p.N ? n : p.N - 1;
    float bias = 0.f;
    if constexpr (EPI == QIE_EPI_STORE) {
        const uint16_t* bp = p.bias[sg];
        if (bp) bias = bf2f(bp[r]);
    }
    unsigned long long kbest[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
    for (int t = 0; t < MT; t++) {
        const int m0 = 16 * t;
        if (m0 >= M) break;   // uniform
        float c[NB][4], ep[4] = {bias, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int j = 0; j < 4; j++) c[b][j] = WT == 0 ? acc[b][t][j] : acc[b][t][j] * sc[b];
        if constexpr (EPI == QIE_EPI_RESIDUAL) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = m0 + 4 * g + j < M ? m0 + 4 * g + j : M - 1;
                ep[j] = bf2f(p.y[(int64_t)i * p.ldy + nc]);
            }
        }
        emit_tile16<EPI>(c, ep, p.y + (int64_t)m0 * p.ldy, p.ldy, M - m0, p.N, n, g, nullptr, 0, kbest);
    }
}

// Split-K workspace (slab + tickets), one per stream, sized for the largest plan
// (kR64SlabTiles) and made outside any capture: qie_batch_create reserves it for a batch of more
// than 16 slots so that the captured step finds it; tickets are zero at rest.
namespace {
struct Rows64Ws {
    float* slab = nullptr;
    unsigned* cnt = nullptr;
};
std::mutex g_r64_mu;
std::map<hipStream_t, Rows64Ws> g_r64_ws;

__global__ void rows64_clear_kernel(unsigned* cnt, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cnt[i] = 0u;
}
}  // namespace

int rows64_reserve(hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_r64_mu);
    Rows64Ws& w = g_r64_ws[st];
    if (w.slab) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    QIE_REQUIRE(hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone,
                "qie_linear: QIE_LINEAR_ROWS64 split-K workspace cannot be made during a graph capture: "
                "launch once (or create the batch) before capturing");
    float* slab = nullptr;
    unsigned* cnt = nullptr;
    QIE_HIP(hipMalloc((void**)&slab, (size_t)kR64SlabTiles * 4 * 1024));
    if (hipMalloc((void**)&cnt, (size_t)kR64MaxTiles * 4) != hipSuccess) {
        (void)hipFree(slab);
        return fail(2, "qie_linear: QIE_LINEAR_ROWS64: out of memory for the ticket array");
    }
    hipLaunchKernelGGL(rows64_clear_kernel, dim3(kR64MaxTiles / 256), dim3(256), 0, st, cnt, kR64MaxTiles);
    QIE_LAUNCH_CHECK();
    QIE_HIP(hipStreamSynchronize(st));
    w.slab = slab;
    w.cnt = cnt;
    return 0;
}

template <int EPI, int WT>
static int rows64_launch(const Rows64Params& p, const Rows64Plan& pl, hipStream_t st) {
    if (pl.mt == 2) hipLaunchKernelGGL((rows64_kernel<EPI, WT, 2>), dim3(pl.grid), dim3(kR64Threads), 0, st, p);
    else if (pl.mt == 3) hipLaunchKernelGGL((rows64_kernel<EPI, WT, 3>), dim3(pl.grid), dim3(kR64Threads), 0, st, p);
    else hipLaunchKernelGGL((rows64_kernel<EPI, WT, 4>), dim3(pl.grid), dim3(kR64Threads), 0, st, p);
    QIE_LAUNCH_CHECK();
    return 0;
}

// qie_linear with QIE_LINEAR_ROWS64: plan, refuse what the kernel does not take (-22, naming
// it), fill the argument block, launch.  extras: the caller passed a fused RoPE or a peer push.
int rows64_linear(const qie_linear_args* a, bool extras, hipStream_t st) {
    const Rows64Plan pl = plan_rows64(*a, device_cu_count(), extras);
    QIE_REQUIRE(pl.error == Rows64Error::None,
                "qie_linear: QIE_LINEAR_ROWS64 takes %s (M=%lld K=%lld N=%lld epilogue %d flags %d)",
                rows64_error_text(pl.error), (long long)a->M, (long long)a->K, (long long)a->N, a->epilogue, a->flags);
    Rows64Params p;
    p.x = (const uint16_t*)a->x;
    p.ldx = a->ldx;
    p.K = (int32_t)a->K;
    p.N = (int32_t)a->N;
    p.M = (int32_t)a->M;
    p.n_tiles = pl.n_tiles;
    p.y = (uint16_t*)a->y;
    p.ldy = a->ldy;
    p.chunks = pl.chunks;
    p.parts = pl.parts;
    p.cpp = pl.cpp;
    p.slab = nullptr;
    p.cnt = nullptr;
    for (int s = 0; s < 3; s++) {
        p.w[s] = (const uint8_t*)a->w[s];
        p.bias[s] = (const uint16_t*)a->bias[s];
    }
    if (a->epilogue == QIE_EPI_SWIGLU) {
        p.seg_rows[0] = p.seg_rows[1] = p.seg_rows[2] = (int32_t)a->N;
        p.t01[0] = p.t01[1] = p.n_tiles;
    } else {
        const int64_t r0 = a->seg_rows[0], r1 = a->seg_rows[1], r2 = a->seg_rows[2];
        // (qie_linear checked that the segments sum to N and have their weights; an empty segment
        // owns no tile and is never indexed)
        p.seg_rows[0] = (int32_t)std::max<int64_t>(1, r0);
        p.seg_rows[1] = (int32_t)std::max<int64_t>(1, r1);
        p.seg_rows[2] = (int32_t)std::max<int64_t>(1, r2);
        p.t01[0] = (int32_t)((r0 + (r1 + r2 > 0 ? 0 : 15)) / 16);
        p.t01[1] = (int32_t)((r0 + r1 + (r2 > 0 ? 0 : 15)) / 16);
    }
    if (pl.parts >= 2) {
        QIE_TRY(rows64_reserve(st));
        std::lock_guard<std::mutex> lk(g_r64_mu);
        const Rows64Ws& w = g_r64_ws[st];
        p.slab = w.slab;
        p.cnt = w.cnt;
    }
    return dispatch_epi<QIE_EPI_SWIGLU, QIE_EPI_RESIDUAL, QIE_EPI_STORE>(a->epilogue, [&](auto E) {
        constexpr int EPI = decltype(E)::value;
        if (pl.wt == 2) return rows64_launch<EPI, 2>(p, pl, st);
        if (pl.wt == 1) return rows64_launch<EPI, 1>(p, pl, st);
        return rows64_launch<EPI, 0>(p, pl, st);
    });
}

}  // namespace qie
