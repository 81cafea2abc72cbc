// k_gemm.hip — MFMA GEMMs for the prefill projections (M = prompt rows).
//
// Replaces matrix_mul (layers/src/matrix_mul.cu:165-288) for M > 8: the
// reference computes one 16x16 WMMA tile per warp with scalar 2-byte loads into
// per-warp smem and no pipelining.  Here (gfx950):
//   C[M, N] = A[M, K] . W[N, K]^T   (both operands K-contiguous, "NT")
// Five kernels, chosen by plan_gemm() (gemm_plan.hpp); gemm() at the end of the file validates,
// plans, gets the split-K workspace and launches the plan's instantiation:
//   gemm_kernel      generic 128x128 tile, any K % 8 == 0, bf16 or fp8 weights (below)
//   gemm_big_kernel  256x256 / 256x128 tile, LDS-DMA into a ring of four 32-deep k-tiles
//   gemm8_kernel     256x256 tile, phase-interleaved (gemm8_tile.hpp), optional split-K
//   gemm8sk_kernel   the same tile pipeline over stream-K ranges
//   gemm8mx_kernel   the same schedule on block-scaled e4m3 operands (fp8 activations)
// All of them end in gemm_epilogue() (bias / residual / SwiGLU / fp32).  The generic kernel:
//   * 128x128 block tile, BK = 64, 4 waves as 2x2, 64x64 per wave =
//     4x4 v_mfma_f32_16x16x32_bf16 accumulators (fp32);
//   * 16-byte global loads staged through registers into a double-buffered,
//     XOR-swizzled LDS image (chunk ^= row & 7), fragments by ds_read_b128;
//     one barrier per K-tile, next tile's global loads in flight under the
//     current tile's MFMAs;
//   * fused epilogues: bias, residual add, SwiGLU (tile columns pair gate/up
//     rows of the same output column inside one wave).
//   * blockIdx.x runs over M tiles so the blocks sharing a weight tile are
//     adjacent in dispatch order (weights streamed ~once, activations L2/MALL).
#include "qie_common.hpp"
#include "launch_util.hpp"
#include "gemm_plan.hpp"
#include "gemm8_tile.hpp"
#include "linear_epilogue.hpp"
#include "../../include/qie/qie_ops.h"

#include <map>
#include <mutex>

namespace qie {

struct GemmParams {
    const uint16_t* A;
    int64_t lda;
    const uint16_t* w0;
    const uint16_t* w1;
    const uint16_t* w2;
    const uint16_t* b0;
    const uint16_t* b1;
    const uint16_t* b2;
    int64_t n0, n01;
    int64_t M, K, N;     // N = output columns
    int64_t wrows;       // total weight rows addressable (for clamping)
    uint16_t* C;
    int64_t ldc;
};

constexpr int BM = 128, BN = 128, BK = 64;

// Weight row for tile column c of block tile starting at output column n0; eb = bytes
// per weight; for fp8 (eb = 1) also the row's scale (stored after the segment's codes).
template <int EPI>
__device__ __forceinline__ const uint16_t* w_row(const GemmParams& p, int64_t nblk, int c, bool& valid, int eb,
                                                 int64_t& row, float& scale) {
    auto at = [&](const uint16_t* w, int64_t rows, int64_t r) {
        const uint8_t* b = reinterpret_cast<const uint8_t*>(w);
        scale = eb == 1 ? reinterpret_cast<const float*>(b + rows * p.K)[r] : 1.f;
        row = r;
        return reinterpret_cast<const uint16_t*>(b + r * p.K * eb);
    };
    if constexpr (EPI == QIE_EPI_SWIGLU) {
        // 64 output columns per tile: cols [64wc, 64wc+32) gate, [64wc+32, 64wc+64) up.
        const int64_t j = nblk * 64 + 32 * (c >> 6) + (c & 31);
        valid = j < p.N;
        const int64_t jj = valid ? j : p.N - 1;
        return ((c >> 5) & 1) ? at(p.w1, p.N, jj) : at(p.w0, p.N, jj);
    } else {
        const int64_t r = nblk * BN + c;
        valid = r < p.N;
        const int64_t rr = valid ? r : p.N - 1;
        if (rr < p.n0) return at(p.w0, p.n0, rr);
        if (rr < p.n01) return at(p.w1, p.n01 - p.n0, rr - p.n0);
        return at(p.w2, p.N - p.n01, rr - p.n01);
    }
}

// fp8 weights (WT = 1, QIE_LINEAR_FP8): e4m3 codes + power-of-two row scales after the
// [rows, K] code block; a B chunk (8 weights) is one 8-byte load, decoded and scaled to
// bf16 (exact: 3 mantissa bits x 2^k) before the LDS store, so the MFMA path is the
// bf16 one at half the weight bytes.
__device__ __forceinline__ uint4 fp8x8_to_bf16(uint2 q, float sc) {
    float f[8];
    fp8x4_to_f32(q.x, f);
    fp8x4_to_f32(q.y, f + 4);
    return make_uint4(pack2(f[0] * sc, f[1] * sc), pack2(f[2] * sc, f[3] * sc), pack2(f[4] * sc, f[5] * sc),
                      pack2(f[6] * sc, f[7] * sc));
}

// ---------------- epilogue of every GEMM kernel.  A wave holds NI x NJ accumulator fragments
// (16x16 each; C/D map: col = lane & 15 = fr, row = 4 * (lane >> 4) + r = 4 fq + r) of the rows
// from m0 (tile) + wrow (wave) and the weight rows (tile columns) from col0.  SWIGLU: fragment
// jj is the gate and jj + NJ / 2 the up row of output column swcol0 + 16 jj + fr; STORE adds the
// bias of the column's segment (b0 / b1 / b2, each may be null).
struct EpiOut {
    uint16_t* C;
    int64_t ldc, M, N, n0, n01;
};
template <class P>
__device__ __forceinline__ EpiOut epi_out(const P& p) {
    return EpiOut{p.C, p.ldc, p.M, p.N, p.n0, p.n01};
}

template <int EPI, int NI, int NJ>
__device__ __forceinline__ void gemm_epilogue(const f32x4 (&acc)[NI][NJ], const EpiOut& o, int64_t m0, int wrow, int64_t col0,
                                              int64_t swcol0, int fr, int fq, const uint16_t* b0, const uint16_t* b1,
                                              const uint16_t* b2) {
#pragma clang fp contract(off)
    if constexpr (EPI == QIE_EPI_SWIGLU) {
#pragma unroll
        for (int i = 0; i < NI; i++) {
#pragma unroll
            for (int jj = 0; jj < NJ / 2; jj++) {
                const int64_t col = swcol0 + 16 * jj + fr;
                if (col >= o.N) continue;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = m0 + wrow + i * 16 + fq * 4 + r;
                    if (row >= o.M) continue;
                    o.C[row * o.ldc + col] = swiglu_bf16(acc[i][jj][r], acc[i][jj + NJ / 2][r]);
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int64_t col = col0 + j * 16 + fr;
            if (col >= o.N) continue;
            float bias = 0.f;
            if constexpr (EPI == QIE_EPI_STORE) {
                const uint16_t* b = col < o.n0 ? b0 : (col < o.n01 ? b1 : b2);
                if (b) bias = bf2f(b[col < o.n0 ? col : (col < o.n01 ? col - o.n0 : col - o.n01)]);
            }
#pragma unroll
            for (int i = 0; i < NI; i++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = m0 + wrow + i * 16 + fq * 4 + r;
                    if (row >= o.M) continue;
                    if constexpr (EPI == QIE_EPI_F32) {
                        reinterpret_cast<float*>(o.C)[row * o.ldc + col] = acc[i][j][r];
                        continue;
                    }
                    uint16_t* dst = o.C + row * o.ldc + col;
                    if constexpr (EPI == QIE_EPI_RESIDUAL)
                        *dst = f2bf(bf2f(*dst) + rbf(acc[i][j][r]));
                    else
                        *dst = f2bf(acc[i][j][r] + bias);
                }
            }
        }
    }
}

template <int EPI, int WT>
__global__ __launch_bounds__(256) void gemm_kernel(GemmParams p) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* As = reinterpret_cast<uint16_t*>(smem);                 // [2][BM][BK]
    uint16_t* Bs = reinterpret_cast<uint16_t*>(smem + 2 * BM * BK * 2);  // [2][BN][BK]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t mblk = blockIdx.x, nblk = blockIdx.y;
    const int64_t m0 = mblk * BM;

    // Per-thread staging coordinates: 4 chunks (16 B) of A and of B per K-tile.
    const uint16_t* a_src[4];
    const uint8_t* b_src[4];   // byte address of the row's chunk (bf16: 2 B / weight, fp8: 1)
    float b_sc[4];             // fp8 row scale
    int lds_off[4];
    constexpr int EB = WT ? 1 : 2;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int c = tid + 256 * i;       // chunk id 0..1023
        const int row = c >> 3, ch = c & 7;
        int64_t ar = m0 + row;
        if (ar >= p.M) ar = p.M - 1;
        a_src[i] = p.A + ar * p.lda + ch * 8;
        bool v;
        int64_t wr_row;
        const uint16_t* wbase = w_row<EPI>(p, nblk, row, v, EB, wr_row, b_sc[i]);
        b_src[i] = reinterpret_cast<const uint8_t*>(wbase) + ch * 8 * EB;
        lds_off[i] = row * BK + ((ch ^ (row & 7)) * 8);
    }

    const int nk = (int)((p.K + BK - 1) / BK);
    uint4 ra[4], rb[4];
    uint2 rq[4];
    // Unconditional loads at clamped addresses (chunks past K are re-reads of the last
    // chunk, zeroed by a select): a load under a condition is branched around and the
    // waitcnt pass then waits for everything at the join.
    auto gload = [&](int kt) {
        const int64_t kbase = (int64_t)kt * BK;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int ch = (tid + 256 * i) & 7;
            const bool ok = kbase + ch * 8 < p.K;
            const int64_t kb = ok ? kbase : p.K - 8 - ch * 8;
            ra[i] = *reinterpret_cast<const uint4*>(a_src[i] + kb);
            if constexpr (WT == 0) rb[i] = *reinterpret_cast<const uint4*>(b_src[i] + kb * 2);
            else rq[i] = *reinterpret_cast<const uint2*>(b_src[i] + kb);
            if (!ok) {
                ra[i] = make_uint4(0, 0, 0, 0);
                if constexpr (WT == 0) rb[i] = make_uint4(0, 0, 0, 0);
                else rq[i] = make_uint2(0, 0);
            }
        }
    };
    auto lstore = [&](int buf) {
        uint16_t* a = As + buf * BM * BK;
        uint16_t* b = Bs + buf * BN * BK;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            *reinterpret_cast<uint4*>(a + lds_off[i]) = ra[i];
            if constexpr (WT == 0) *reinterpret_cast<uint4*>(b + lds_off[i]) = rb[i];
            else *reinterpret_cast<uint4*>(b + lds_off[i]) = fp8x8_to_bf16(rq[i], b_sc[i]);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    gload(0);
    lstore(0);
    __syncthreads();

    const int fr = lane & 15, fq = lane >> 4;
    int cur = 0;
    for (int kt = 0; kt < nk; kt++) {
        if (kt + 1 < nk) gload(kt + 1);
        const uint16_t* a = As + cur * BM * BK;
        const uint16_t* b = Bs + cur * BN * BK;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            bf16x8 af[4], bfr[4];
            const int ch = ks * 4 + fq;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int row = wr * 64 + i * 16 + fr;
                af[i] = *reinterpret_cast<const bf16x8*>(a + row * BK + ((ch ^ (row & 7)) * 8));
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int row = wc * 64 + j * 16 + fr;
                bfr[j] = *reinterpret_cast<const bf16x8*>(b + row * BK + ((ch ^ (row & 7)) * 8));
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) lstore(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    gemm_epilogue<EPI, 4, 4>(acc, epi_out(p), m0, wr * 64, nblk * BN + wc * 64, nblk * 64 + 32 * wc, fr, fq, p.b0, p.b1, p.b2);
}

// ---------------------------------------------------------------------------
// Large prefill GEMM (bf16 weights, K % 32 == 0, enough 256x256 tiles to fill the chip):
// 256x256 block tile, 8 waves as 2 (M) x 4 (N), 128x64 per wave = 8x4 accumulators of
// v_mfma_f32_16x16x32_bf16.  Both operands go global -> LDS by LDS-DMA
// (global_load_lds_dwordx4: one wave-instruction = 16 rows x 64 B, the LDS image
// lane-linear, the chunk swizzle applied to the SOURCE address) into a ring of four
// 32-deep k-tiles (4 x 32 KB): three k-tiles stay in flight across the raw s_barrier that
// opens each k-step and are retired by a counted vmcnt, never vmcnt(0) in the main loop
// (cdna_hip_programming.md §5 'Pipelining across barriers', 'What does break it').  One
// workgroup (2 waves per SIMD) per CU; the bijective XCD remap keeps the M tiles that
// share a weight tile on one XCD, so each weight tile comes from HBM into one L2 once.
namespace big {
constexpr int BM = 256, BK = 32, SLOTS = 4;
// slot = A rows then B rows, 64 B each: 32 KB at BN 256, 24 KB at BN 128
constexpr int slot_bytes(int bn) { return (BM + bn) * BK * 2; }
}  // namespace big

// chunk swizzle of 64-B LDS rows: the 16-B chunk c of row r sits at position c ^ swz(r).
// With it the 16 lanes of each ds_read_b128 lane group ({0-3,12-15,20-27}, ...) reading
// rows fr (and chunk g) of a 16-row fragment land on 16 distinct bank slots.
__device__ __forceinline__ int big_swz(int r) { return ((r >> 2) & 1) * 3; }


// weight row feeding tile column c (0..255) of column tile nt; SwiGLU tiles interleave
// 32 gate rows and the 32 up rows of the same outputs per 64-column wave slice
template <int EPI, int BNT>
__device__ __forceinline__ const uint16_t* big_wrow(const GemmParams& p, int64_t nt, int c) {
    if constexpr (EPI == QIE_EPI_SWIGLU) {
        constexpr int HALF = BNT / 8;   // gate (then up) rows per 1/4-tile wave slice
        const int ws = c / (BNT / 4), q = c % (BNT / 4);
        const int64_t j = nt * (BNT / 2) + ws * HALF + (q % HALF);
        const int64_t jj = j < p.N ? j : p.N - 1;
        return (q >= HALF ? p.w1 : p.w0) + jj * p.K;
    } else {
        const int64_t r = nt * BNT + c;
        const int64_t rr = r < p.N ? r : p.N - 1;
        if (rr < p.n0) return p.w0 + rr * p.K;
        if (rr < p.n01) return p.w1 + (rr - p.n0) * p.K;
        return p.w2 + (rr - p.n01) * p.K;
    }
}

template <int EPI, int BNT>
__global__ __launch_bounds__(512) void gemm_big_kernel(GemmParams p, int n_mt) {
#pragma clang fp contract(off)
    constexpr int TM = big::BM, TK = big::BK, NSL = big::SLOTS, SB = big::slot_bytes(BNT);
    constexpr int NJ = BNT / 64;            // 16-column fragments per wave (4 waves along N)
    constexpr int NBI = BNT / 128;          // B wave-instructions per k-tile per wave
    constexpr int LPK = 2 + NBI;            // LDS-DMA instructions per k-tile per wave
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int fr = lane & 15, g = lane >> 4;
    // bijective XCD remap (cdna_hip_programming.md §5 'XCD swizzle must be bijective')
    const int nwg = gridDim.x, orig = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = orig & 7;
    const int wid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
    const int64_t mt = wid % n_mt, nt = wid / n_mt;
    const int64_t m0 = mt * TM;

    // staging: wave-instruction i (0, 1) of this wave moves rows [32 wave + 16 i, +16) of the
    // A tile and of the B tile; lane -> row (lane >> 2), LDS chunk (lane & 3)
    const uint16_t* asrc[2];
    const uint16_t* bsrc[NBI];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int r = 32 * wave + 16 * i + (lane >> 2);
        const int c = (lane & 3) ^ big_swz(r);
        int64_t ar = m0 + r;
        ar = ar < p.M ? ar : p.M - 1;   // rows past M: re-read row M-1, never stored
        asrc[i] = p.A + ar * p.lda + c * 8;
    }
#pragma unroll
    for (int i = 0; i < NBI; i++) {
        const int r = 16 * NBI * wave + 16 * i + (lane >> 2);
        const int c = (lane & 3) ^ big_swz(r);
        bsrc[i] = big_wrow<EPI, BNT>(p, nt, r) + c * 8;
    }
    const int nk = (int)(p.K / TK);
    auto issue = [&](int kt) {
        unsigned char* slot = smem + (kt & (NSL - 1)) * SB;
        const int64_t k0 = (int64_t)kt * TK;
#pragma unroll
        for (int i = 0; i < 2; i++) glds16(asrc[i] + k0, slot + (32 * wave + 16 * i) * (TK * 2));
#pragma unroll
        for (int i = 0; i < NBI; i++) glds16(bsrc[i] + k0, slot + TM * TK * 2 + (16 * NBI * wave + 16 * i) * (TK * 2));
    };

    f32x4 acc[8][NJ];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < NJ; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    issue(0);
    if (nk > 1) issue(1);
    if (nk > 2) issue(2);
    for (int kt = 0; kt < nk; kt++) {
        // this wave's DMAs of tile kt have landed once at most the later tiles' are pending
        if (kt + 2 < nk) {
            if constexpr (LPK == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        } else if (kt + 1 < nk) {
            if constexpr (LPK == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();            // ... and every other wave's; slot kt-1 is free
        asm volatile("" ::: "memory");
        if (kt + 3 < nk) issue(kt + 3);          // into the slot of tile kt - 1
        const uint16_t* As = reinterpret_cast<const uint16_t*>(smem + (kt & (NSL - 1)) * SB);
        const uint16_t* Bs = As + TM * TK;
        bf16x8 af[8], bfr[NJ];
        // every fragment read is issued before the first MFMA (B first, then A in MFMA
        // order): one exposed LDS latency per k-tile instead of the compiler's four
        // read-two / wait-all / eight-MFMA batches (P = 2048: gate/up -2 %, O and down -6 %)
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int row = wn * (BNT / 4) + j * 16 + fr;
            bfr[j] = *reinterpret_cast<const bf16x8*>(Bs + row * TK + ((g ^ big_swz(row)) * 8));
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int row = wm * 128 + i * 16 + fr;
            af[i] = *reinterpret_cast<const bf16x8*>(As + row * TK + ((g ^ big_swz(row)) * 8));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int j = 0; j < NJ; j++)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }

    gemm_epilogue<EPI, 8, NJ>(acc, epi_out(p), m0, wm * 128, nt * BNT + wn * (BNT / 4), nt * (BNT / 2) + (BNT / 8) * wn, fr, g, p.b0,
                              p.b1, p.b2);
}

// ---------------------------------------------------------------------------
// Prefill GEMM, phase-interleaved: the tile pipeline, its layout and schedule, and the split-K
// hand-off are in gemm8_tile.hpp.  A kernel chooses its tile and k range, runs the pipeline,
// optionally merges split-K parts, and runs the epilogue.

// DMA sources of a bf16 tile: A rows from m0, weight rows of column tile nt
template <int EPI>
__device__ __forceinline__ void g8_set_tile(G8Bf16& op, const GemmParams& p, const G8Lane& l, int64_t m0, int64_t nt) {
    op.map(l, [&](int u, int i, int r, int cs) {
        if (u == 0 || u == 3) {
            int64_t ar = m0 + r;
            ar = ar < p.M ? ar : p.M - 1;   // rows past M: re-read row M-1, never stored
            op.src[u][i] = p.A + ar * p.lda + cs * 8;
        } else {
            op.src[u][i] = big_wrow<EPI, 256>(p, nt, r) + cs * 8;
        }
    });
}

// epilogue of a 256x256 tile held as 8x4 fragments per wave (as gemm_big_kernel at BNT = 256)
template <int EPI>
__device__ __forceinline__ void g8_epilogue(const f32x4 (&acc)[8][4], const EpiOut& o, const G8Lane& l, int64_t m0, int64_t nt,
                                            const uint16_t* b0, const uint16_t* b1, const uint16_t* b2) {
    gemm_epilogue<EPI, 8, 4>(acc, o, m0, l.wm * 128, nt * 256 + l.wn * 64, nt * 128 + 32 * l.wn, l.fr, l.g, b0, b1, b2);
}

template <int EPI>
__global__ __launch_bounds__(512) void gemm8_kernel(GemmParams p, int n_mt, G8Split sk) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const G8Lane l = g8_lane();
    const int wid = xcd_major_wid();
    const int tile = wid / sk.splitk, part = wid % sk.splitk;
    const int64_t mt = tile % n_mt, nt = tile / n_mt;
    const int64_t m0 = mt * g8::BM;

    G8Bf16 op;
    g8_set_tile<EPI>(op, p, l, m0, nt);
    const int nk_all = (int)(p.K / g8::BK);
    op.kb = (int)((int64_t)part * nk_all / sk.splitk);        // this part's k-tiles [kb, kb + nk)
    const int nk = (int)((int64_t)(part + 1) * nk_all / sk.splitk) - op.kb;
    f32x4 acc[8][4];
    g8_pipeline<false>(op, l, smem, nk, acc);   // nk >= 4 (plan_gemm)
    if (sk.splitk > 1 && !g8_splitk_merge(sk, tile, part, smem, l, acc)) return;   // uniform
    g8_epilogue<EPI>(acc, epi_out(p), l, m0, nt, p.b0, p.b1, p.b2);
}

// Stream-K form of gemm8 (one workgroup per CU, a fixed grid).  Tile quantisation costs the
// one-tile-per-workgroup kernel whole rounds: gate/up at 2,048 rows has 1,184 tiles = 4.625
// rounds of 256 (the fifth round 62 % busy), QKV 144 tiles (one round, 56 % busy), down 112
// (split-K 2: 224 of 256 CUs).  Here the work is (tile, k-tile) units: the first
// dp_rounds * grid tiles go whole, one per workgroup per round; the k-tile units of the
// remaining tiles are cut into `grid` contiguous ranges of `chunk` units (tile-major, so a
// range is a tail of one tile, whole tiles, the head of another).  A tile covered by one
// range is finished in place; a tile shared by several ranges (its SEGMENTS) is finished by
// the last-arriving segment (ticket), which sums every segment's fp32 slab in SEGMENT order
// (k order; independent of arrival order) and runs the epilogue.  A workgroup's only
// partial segments are its range's first and last: slab [workgroup][first / last].
struct G8Stream {
    int dp_rounds;     // whole-tile rounds: tile r * grid + w for r < dp_rounds
    int tiles;         // all tiles; stream-K covers [dp_rounds * grid, tiles)
    int chunk;         // k-tile units per stream-K range
    float* slab;       // [grid][2][256 * 256] fp32
    unsigned* cnt;     // [tiles], zero at rest
};

template <int EPI>
__global__ __launch_bounds__(512) void gemm8sk_kernel(GemmParams p, int n_mt, G8Stream sk) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const G8Lane l = g8_lane();
    const int nwg = gridDim.x, wid = xcd_major_wid();
    const int nk_all = (int)(p.K / g8::BK);

    int64_t m0 = 0, nt = 0;
    G8Bf16 op;
    f32x4 acc[8][4];
    // k-tiles [kb, kb + nk) of `tile` into acc
    auto run = [&](int tile, int kb, int nk) {
        nt = tile / n_mt;
        m0 = (int64_t)(tile % n_mt) * g8::BM;
        g8_set_tile<EPI>(op, p, l, m0, nt);
        op.kb = kb;
        g8_pipeline<true>(op, l, smem, nk, acc);
    };
    auto epilogue = [&]() { g8_epilogue<EPI>(acc, epi_out(p), l, m0, nt, p.b0, p.b1, p.b2); };

    // ---- whole tiles
    for (int r = 0; r < sk.dp_rounds; r++) {
        run(r * nwg + wid, 0, nk_all);
        epilogue();
        __syncthreads();   // the next tile's DMA reuses the buffers
    }
    // ---- stream-K ranges
    const int64_t base = (int64_t)sk.dp_rounds * nwg * nk_all;
    const int64_t total = (int64_t)sk.tiles * nk_all;
    const int64_t ustart = base + (int64_t)wid * sk.chunk;
    const int64_t uend = ustart + sk.chunk < total ? ustart + sk.chunk : total;
    for (int64_t u = ustart; u < uend;) {   // uniform
        const int tile = (int)(u / nk_all);
        const int k0 = (int)(u % nk_all);
        const int k1 = (int)(uend - u < (int64_t)(nk_all - k0) ? k0 + (uend - u) : nk_all);
        run(tile, k0, k1 - k0);
        bool emit = true;
        if (k0 != 0 || k1 != nk_all) {   // uniform: a shared tile
            const int slot = u == ustart ? 0 : 1;
            g8_slab_store(sk.slab + ((int64_t)wid * 2 + slot) * kG8SlabFloats, l, acc);
            // the tile's segments: ranges wf..wl
            const int64_t tu0 = (int64_t)tile * nk_all - base;
            const int wf = (int)(tu0 / sk.chunk), wl = (int)((tu0 + nk_all - 1) / sk.chunk);
            emit = g8_ticket_last(sk.cnt + tile, (unsigned)(wl - wf), smem, l);
            if (emit) {
                for (int w2 = wf; w2 <= wl; w2++) {   // segment (k) order
                    const int64_t s2 = base + (int64_t)w2 * sk.chunk;
                    const int slot2 = s2 / nk_all == tile ? 0 : 1;
                    g8_slab_sum(sk.slab + ((int64_t)w2 * 2 + slot2) * kG8SlabFloats, w2 == wf, l, acc);
                }
                g8_ticket_reset(sk.cnt + tile, l);
            }
        }
        if (emit) epilogue();
        u += k1 - k0;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Block-scaled fp8 prefill GEMM (round 5; BASELINE config 4's "CDNA4 fp8 MFMA", numerics flag
// QIE_LINEAR_ACT_FP8):  C[m, n] = sum_k (2^ea[m] qa[m, k]) (sw[n] qw[n, k])  with e4m3
// activation codes qa and per-row power-of-two exponents ea (qie_quantize_rows_fp8), e4m3
// weight codes qw with power-of-two row scales sw (the engine's fp8 arena, plain or 16-row
// tiled).  Both scales are row constants, so they enter v_mfma_scale_f32_16x16x128_f8f6f4 as
// its per-lane e8m0 operands (every lane of an A row / B column passes the same byte) and the
// accumulators come out scaled: the epilogues are gemm8's.  The product of two e4m3 values is
// exact; the instruction's K = 128 per step doubles the bf16 rate per clock (MI355X_MICROARCH
// "Matrix cores": twice the cycles of the bf16 16x16 form at 4x the K).
//   Structure = gemm8_kernel's (256x256 tile, 8 waves 2 x 4, four phases per k-tile, LDS-DMA
// units in read order, waves 4-7 one barrier behind): a k-tile is BK = 128 codes, i.e. the
// same 128-B LDS rows as gemm8's 64 bf16, so the buffers, unit schedule, swizzle and waits are
// unchanged; a fragment is 32 codes (chunks 2g, 2g + 1 of the row: k = 32 g + [0, 32), the
// 16x16x128 lane map) and a phase issues 8 MFMAs of twice the cycles instead of 16.
//   This kernel keeps its OWN copy of the unit map and the phase loop (g8_pipeline's text with
// the scaled-MFMA fragments): moved onto the shared pipeline behind an operand policy, its
// prologue compiled differently and the unsplit launches measured 0.6-1 % slower (QKV at 2,048
// rows 64.1 -> 64.8 us), so only the split-K hand-off and the epilogue are shared.  Change
// the schedule in gemm8_tile.hpp and here together.
// Tiled weights (QIE_LINEAR_FP8_T16) are gathered straight from their 1-KiB blocks by the
// per-lane DMA addresses (chunk c of row r: block (r / 16, c / 4), bytes 16 ((r % 16) +
// 16 (c % 4))), so the decode layout is the prefill's too — no bf16 copy is read.
struct MxParams {
    const uint8_t* A;     // [M][lda] e4m3 codes
    int64_t lda;          // bytes
    const uint8_t* ea;    // [M] e8m0 row exponents
    const uint8_t* w[3];  // fp8 segments: codes, then fp32 row scales
    const uint16_t* b[3];
    int64_t rows[3];      // segment rows
    int64_t n0, n01;
    int64_t M, K, N;
    uint16_t* C;
    int64_t ldc;
};

// segment, row-in-segment of tile column c (0..255) of column tile nt (big_wrow's mapping)
template <int EPI>
__device__ __forceinline__ int mx_wrow(const MxParams& p, int64_t nt, int c, int64_t& r) {
    if constexpr (EPI == QIE_EPI_SWIGLU) {
        const int ws = c / 64, q = c % 64;
        const int64_t j = nt * 128 + ws * 32 + (q % 32);
        r = j < p.N ? j : p.N - 1;
        return q >= 32 ? 1 : 0;
    } else {
        int64_t rr = nt * 256 + c;
        rr = rr < p.N ? rr : p.N - 1;
        if (rr < p.n0) { r = rr; return 0; }
        if (rr < p.n01) { r = rr - p.n0; return 1; }
        r = rr - p.n01;
        return 2;
    }
}

template <int EPI, bool T16>
__global__ __launch_bounds__(512) void gemm8mx_kernel(MxParams p, int n_mt, G8Split sk, int dbg) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int fr = lane & 15, g = lane >> 4;
    const int nwg = gridDim.x, orig = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = orig & 7;
    const int wid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
    const int tile = wid / sk.splitk, part = wid % sk.splitk;
    const int64_t mt = tile % n_mt, nt = tile / n_mt;
    const int64_t m0 = mt * g8::BM;
    const int64_t K = p.K;

    // e8m0 operands, packed 4 per register (byte i of sa_pk[qa]: A row 128 wm + 64 qa + 16 i +
    // fr; byte 2 qb + j of sb_pk: B tile column 64 wn + 32 qb + 16 j + fr -> the exponent of the
    // weight row's power-of-two scale): 3 VGPRs, the budget gemm8's 254 leaves
    uint32_t sa_pk[2] = {0u, 0u}, sb_pk = 0u;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        int64_t ar = m0 + 128 * wm + 16 * q + fr;
        ar = ar < p.M ? ar : p.M - 1;
        sa_pk[q >> 2] |= (uint32_t)p.ea[ar] << (8 * (q & 3));
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int64_t r;
        const int sg = mx_wrow<EPI>(p, nt, 64 * wn + 16 * j + fr, r);
        const uint8_t* base = sg == 0 ? p.w[0] : (sg == 1 ? p.w[1] : p.w[2]);
        const int64_t rows = sg == 0 ? p.rows[0] : (sg == 1 ? p.rows[1] : p.rows[2]);
        const uint32_t bits = __float_as_uint(reinterpret_cast<const float*>(base + rows * K)[r]);
        sb_pk |= ((bits >> 23) & 0xffu) << (8 * j);
    }
    // the exponents are waited for here, once: an opaque register pin makes them values of
    // this point, so no wait for them is left inside the DMA-pipelined loop
    asm volatile("" : "+v"(sa_pk[0]), "+v"(sa_pk[1]), "+v"(sb_pk));

    // DMA sources (gemm8's units and rows): A as 32-bit row offsets from p.A (4 VGPRs), W as
    // pointers (segments may lie anywhere)
    uint32_t aoff[2][2];
    const uint8_t* wsrc[2][2];
    int dst_row[4][2];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int b = 2 * wave + i;
            int row0;
            if (u == 0 || u == 3) row0 = (b < 8 ? 8 * b : 128 + 8 * (b - 8)) + (u == 3 ? 64 : 0);
            else row0 = 64 * (b >> 2) + 8 * (b & 3) + (u == 2 ? 32 : 0);
            dst_row[u][i] = row0;
            const int rw = row0 + (lane >> 3);
            const int cs = (lane & 7) ^ g8_swz(rw);
            if (u == 0 || u == 3) {
                int64_t ar = m0 + rw;
                ar = ar < p.M ? ar : p.M - 1;   // rows past M: re-read row M-1, never stored
                aoff[u == 3][i] = (uint32_t)(ar * p.lda + cs * 16);
            } else {
                int64_t r;
                const int sg = mx_wrow<EPI>(p, nt, rw, r);
                const uint8_t* base = sg == 0 ? p.w[0] : (sg == 1 ? p.w[1] : p.w[2]);
                if constexpr (T16)
                    wsrc[u - 1][i] = base + (r >> 4) * 16 * K + (cs >> 2) * 1024 + 16 * ((r & 15) + 16 * (cs & 3));
                else
                    wsrc[u - 1][i] = base + r * K + cs * 16;
            }
        }
    constexpr int64_t WSTEP = T16 ? 2048 : mx::BK;   // weight bytes per k-tile
    const int nk_all = (int)(K / mx::BK);
    const int kb = (int)((int64_t)part * nk_all / sk.splitk);
    const int nk = (int)((int64_t)(part + 1) * nk_all / sk.splitk) - kb;
    auto stage = [&](int u, int kt) {
        unsigned char* buf = smem + (kt & 1) * g8::BUF + ((u == 0 || u == 3) ? 0 : g8::BM * 128);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (u == 0 || u == 3)
                glds16(p.A + (int64_t)(kb + kt) * mx::BK + aoff[u == 3][i], buf + dst_row[u][i] * 128);
            else
                glds16(wsrc[u - 1][i] + (int64_t)(kb + kt) * WSTEP, buf + dst_row[u][i] * 128);
        }
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    i32x8_mx fa[4], fb0[2], fb1[2];

    auto frag = [&](const unsigned char* rowp, int row) -> i32x8_mx {
        const u32x4_g8 lo = *reinterpret_cast<const u32x4_g8*>(rowp + (((2 * g) ^ g8_swz(row)) * 16));
        const u32x4_g8 hi = *reinterpret_cast<const u32x4_g8*>(rowp + (((2 * g + 1) ^ g8_swz(row)) * 16));
        return i32x8_mx{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    };
    auto read_a = [&](const unsigned char* buf, int qa) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int row = 128 * wm + 64 * qa + 16 * i + fr;
            fa[i] = frag(buf + row * 128, row);
        }
    };
    auto read_b = [&](const unsigned char* buf, int qb, i32x8_mx (&fb)[2]) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int row = 64 * wn + 32 * qb + 16 * j + fr;
            fb[j] = frag(buf + g8::BM * 128 + row * 128, row);
        }
    };
    auto mfma_q = [&](int qa, int qb, const i32x8_mx (&fb)[2]) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 2; j++)
            {
                acc[4 * qa + i][2 * qb + j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                    fa[i], fb[j], acc[4 * qa + i][2 * qb + j], 0, 0, 0, (int)((sa_pk[qa] >> (8 * i)) & 0xffu), 0,
                    (int)((sb_pk >> (8 * (2 * qb + j))) & 0xffu));
                if (QIE_DBG(dbg == 1)) asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
            }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto bar = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    auto wait8 = [&](bool tail) {
        if (tail) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    };

    // prologue (gemm8's): UA0(0) UB0(0) UB1(0) UA1(0) UA0(1) UB0(1)
    stage(0, 0); stage(1, 0); stage(2, 0); stage(3, 0);
    if (nk > 1) { stage(0, 1); stage(1, 1); }
    if (nk > 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bar();
    if (wm == 1) bar();
    for (int t = 0; t < nk; t++) {
        const unsigned char* buf = smem + (t & 1) * g8::BUF;
        const bool tail = t >= nk - 2;
        // keep the packed exponents loop-variant: the byte extractions stay next to their
        // MFMAs instead of being hoisted into 12 registers live across the loop
        asm volatile("" : "+v"(sa_pk[0]), "+v"(sa_pk[1]), "+v"(sb_pk));
        read_b(buf, 0, fb0);
        __builtin_amdgcn_sched_barrier(0);
        read_a(buf, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (t + 1 < nk) stage(2, t + 1);
        wait8(tail);
        bar();
        mfma_q(0, 0, fb0);
        bar();
        read_b(buf, 1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        if (t + 1 < nk) stage(3, t + 1);
        wait8(tail);
        bar();
        mfma_q(0, 1, fb1);
        bar();
        read_a(buf, 1);
        __builtin_amdgcn_sched_barrier(0);
        if (t + 2 < nk) stage(0, t + 2);
        bar();
        mfma_q(1, 1, fb1);
        bar();
        if (t + 2 < nk) stage(1, t + 2);
        wait8(tail);
        bar();
        mfma_q(1, 0, fb0);
        bar();
    }
    if (wm == 0) bar();

    const G8Lane l{tid, lane, wave, wm, wn, fr, g};
    if (sk.splitk > 1 && !g8_splitk_merge(sk, tile, part, smem, l, acc)) return;   // uniform
    gemm_epilogue<EPI, 8, 4>(acc, epi_out(p), m0, wm * 128, nt * 256 + wn * 64, nt * 128 + 32 * wn, fr, g, p.b[0], p.b[1], p.b[2]);
}

// ---------------------------------------------------------------------------
// Split-K slabs + tickets, one set per stream (streams of one device may run GEMMs at the same
// time: tensor-parallel ranks on one GPU in the tests), grown on demand outside graph capture.
struct G8Ws {
    float* slab = nullptr;
    unsigned* cnt = nullptr;
    size_t slab_bytes = 0, cnt_n = 0;
};
static std::mutex g8_mu;
static std::map<hipStream_t, G8Ws> g8_ws;

// nonzero: the workspace would have to grow during a graph capture
static int g8_workspace(hipStream_t st, int slabs, int tiles, G8Split* out) {
    std::lock_guard<std::mutex> lk(g8_mu);
    G8Ws& w = g8_ws[st];
    const size_t need = (size_t)slabs * kG8SlabFloats * 4;
    if (need > w.slab_bytes || (size_t)tiles > w.cnt_n) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return 1;   // no split
        QIE_HIP(hipStreamSynchronize(st));
        const size_t sb = std::max(need, w.slab_bytes), cn = std::max((size_t)tiles, w.cnt_n);   // never shrink
        if (w.slab) hipFree(w.slab);
        if (w.cnt) hipFree(w.cnt);
        w = G8Ws{};
        QIE_HIP(hipMalloc((void**)&w.slab, sb));
        QIE_HIP(hipMalloc((void**)&w.cnt, cn * 4));
        QIE_HIP(hipMemsetAsync(w.cnt, 0, cn * 4, st));   // ordered before this stream's GEMMs
        w.slab_bytes = sb;
        w.cnt_n = cn;
    }
    out->slab = w.slab;
    out->cnt = w.cnt;
    return 0;
}

GemmKnobs dev_gemm_knobs() {   // (qie_common.hpp: also k_gemv.hip's linear_plan_text)
    GemmKnobs k;
    k.gemm_big = dev_env("QIE_GEMM_BIG", k.gemm_big);
    k.gemm8 = dev_env("QIE_GEMM8", k.gemm8);
    k.sk_grid = dev_env("QIE_GEMM8_SK_GRID", k.sk_grid);
    k.sk_mink = dev_env("QIE_GEMM8_SK_MINK", k.sk_mink);
    k.mx_splitk_max = dev_env("QIE_MX_SPLITK_MAX", k.mx_splitk_max);
    return k;
}

template <class... P, class... A>
static int launch_plan(void (*kernel)(P...), const GemmPlan& pl, hipStream_t st, A... args) {
    QIE_TRY(raise_dynamic_lds((const void*)kernel, pl.lds_bytes));
    hipLaunchKernelGGL(kernel, dim3(pl.grid_x, pl.grid_y), dim3(pl.threads), pl.lds_bytes, st, args...);
    QIE_LAUNCH_CHECK();
    return 0;
}

// QIE_LINEAR_ACT_FP8: what gemm8mx_kernel needs of the arguments
static int check_mx(const qie_linear_args* a) {
    QIE_REQUIRE((a->flags & QIE_LINEAR_FP8) && a->x_exps, "qie_linear: ACT_FP8 needs fp8 weights and x_exps");
    QIE_REQUIRE(a->K % mx::BK == 0 && a->ldx >= a->K && a->ldx % 16 == 0,
                "qie_linear: ACT_FP8 needs K %% 128 == 0 and ldx (bytes) %% 16 == 0");
    QIE_REQUIRE(a->norm_w == nullptr && a->argmax_keys == nullptr, "qie_linear: ACT_FP8 takes no fused norm / arg-max");
    // the kernel keeps A row offsets (row * lda + column) in 32 bits: refuse what would wrap
    // (e.g. 8 x 32k rows of the down projection's K = 18,944) instead of reading wrong rows
    QIE_REQUIRE(((int64_t)cdiv(a->M, 256) * 256) * a->ldx < ((int64_t)1 << 32),
                "qie_linear: ACT_FP8 with M (%lld) x ldx (%lld) >= 2^32 bytes of codes (split the rows)",
                (long long)a->M, (long long)a->ldx);
    if (a->flags & QIE_LINEAR_FP8_T16)
        QIE_REQUIRE(a->epilogue == QIE_EPI_SWIGLU ? a->N % 16 == 0
                                                  : a->seg_rows[0] % 16 == 0 && a->seg_rows[1] % 16 == 0 &&
                                                        a->seg_rows[2] % 16 == 0,
                    "qie_linear: tiled fp8 segments must be whole 16-row tiles");
    return 0;
}

// validate, fill the kernels' argument blocks, plan, get the workspace, launch the plan
int gemm(const qie_linear_args* a, hipStream_t st) {
    const bool act8 = (a->flags & QIE_LINEAR_ACT_FP8) != 0;
    if (act8) {
        QIE_TRY(check_mx(a));
    } else {
        QIE_REQUIRE(a->norm_w == nullptr, "qie_linear: fused RMSNorm is GEMV-only (M <= 8)");
        QIE_REQUIRE(a->argmax_keys == nullptr, "qie_linear: fused arg-max is GEMV-only (M <= 8)");
        QIE_REQUIRE(a->K % 8 == 0, "qie_linear: GEMM needs K %% 8 == 0");
    }
    const bool sw = a->epilogue == QIE_EPI_SWIGLU;
    GemmParams p;
    MxParams m;
    p.A = (const uint16_t*)a->x;
    m.A = (const uint8_t*)a->x;
    m.ea = a->x_exps;
    p.w0 = (const uint16_t*)a->w[0];
    p.w1 = (const uint16_t*)a->w[1];
    p.w2 = (const uint16_t*)a->w[2];
    p.b0 = (const uint16_t*)a->bias[0];
    p.b1 = (const uint16_t*)a->bias[1];
    p.b2 = (const uint16_t*)a->bias[2];
    for (int i = 0; i < 3; i++) {
        m.w[i] = (const uint8_t*)a->w[i];
        m.b[i] = (const uint16_t*)a->bias[i];
        m.rows[i] = sw ? (i < 2 ? a->N : 0) : a->seg_rows[i];
    }
    p.lda = m.lda = a->ldx;
    p.n0 = m.n0 = a->seg_rows[0];
    p.n01 = m.n01 = a->seg_rows[0] + a->seg_rows[1];
    p.M = m.M = a->M;
    p.K = m.K = a->K;
    p.N = m.N = a->N;
    p.wrows = 0;
    p.C = m.C = (uint16_t*)a->y;
    p.ldc = m.ldc = a->ldy;

    const GemmKnobs k = dev_gemm_knobs();
    const int cus = device_cu_count();
    GemmPlan pl = plan_gemm(*a, k, cus);
    G8Split ws{1, nullptr, nullptr};
    // no workspace (it would have to grow during a graph capture): what plan_gemm chooses without
    if (pl.slabs > 0 && g8_workspace(st, pl.slabs, pl.tickets, &ws) != 0) pl = plan_gemm(*a, k, cus, false);
    ws.splitk = pl.splitk;
    const G8Stream sk{pl.dp_rounds, pl.tiles, pl.chunk, ws.slab, ws.cnt};
    static const int mx_dbg = dev_env("QIE_MX_DBG", 0);
    return dispatch_epi(a->epilogue, [&](auto E) {
        constexpr int EPI = decltype(E)::value;
        switch (pl.family) {
            case GemmFamily::Generic: return launch_plan(gemm_kernel<EPI, 0>, pl, st, p);
            case GemmFamily::GenericFp8: return launch_plan(gemm_kernel<EPI, 1>, pl, st, p);
            case GemmFamily::Big256: return launch_plan(gemm_big_kernel<EPI, 256>, pl, st, p, pl.n_mt);
            case GemmFamily::Big128: return launch_plan(gemm_big_kernel<EPI, 128>, pl, st, p, pl.n_mt);
            case GemmFamily::Gemm8: return launch_plan(gemm8_kernel<EPI>, pl, st, p, pl.n_mt, ws);
            case GemmFamily::Gemm8StreamK: return launch_plan(gemm8sk_kernel<EPI>, pl, st, p, pl.n_mt, sk);
            case GemmFamily::Mx: return launch_plan(gemm8mx_kernel<EPI, false>, pl, st, m, pl.n_mt, ws, mx_dbg);
            case GemmFamily::MxT16: return launch_plan(gemm8mx_kernel<EPI, true>, pl, st, m, pl.n_mt, ws, mx_dbg);
        }
        return fail(-22, "qie_linear: internal: unplanned GEMM family");
    });
}

}  // namespace qie
