// k_gemm_fp4.hip — the prefill GEMM on MXFP4 weights (M > 16 rows; QIE_LINEAR_FP4_GEMM).
//
// Replaces matrix_mul (layers/src/matrix_mul.cu:165-288) for prompt-sized passes of a model whose
// projection weights are MXFP4 (qie_ops.h), so that no bf16 copy of them has to exist:
//   y = epilogue(x . W^T), x bf16 [M, K], W e2m1 codes + e8m0 block scales, plain or 16-row tiled.
// gemm4_kernel<EPI, T16>: 256x256 block tile, 8 waves as 2 (M) x 4 (N), 128x64 per wave = 8x4
// accumulators of v_mfma_f32_16x16x32_bf16, exactly gemm8_tile.hpp's, so G8Lane, the XCD remap, the
// tile epilogue and the split-K hand-off are that file's.  The two operands take different routes:
//   A (activations): LDS-DMA (glds16) into two 64-KB buffers of 256 rows x 256 B, one 128-column
//     unit each.  A wave-instruction moves 4 rows (1 KiB): lane -> row + (lane >> 4), LDS chunk
//     position lane & 15; wave w moves rows [32 w, 32 w + 32) in 8 instructions.
//   B (weights): never in LDS.  Per unit and 16-row weight tile j of the wave's 64 columns every
//     lane loads 16 B of codes = ONE MX block (lane (fr, g): weight row fr of the tile, columns
//     128 u + 32 g + [0, 32)) and its scale byte, through buffer resources whose range ends with the
//     segment's codes / scales: rows past N read zero.  T16: the wave's load is the contiguous 1-KiB
//     block of (tile, unit) and the 64-B scale line; plain: row fr, bytes 64 u + 16 g + [0, 16).
//     Dword s of the vector and the scale go through four v_cvt_scalef32_pk_bf16_fp4 (fp4_convert.hpp)
//     into the B operand of MFMA step s.  The two M halves load the same codes (from L2).
// Fragment mapping (dec4_kernel's, so A and B agree on the K permutation): MFMA step s = 0..3 of a
// unit multiplies columns 128 u + 32 g + 8 s + [0, 8) for lane group g; the A fragment is the 16-B
// chunk c = 4 g + s of the row's 256 B.  Chunk c of row r sits at LDS position (4 s + g) ^ swz(r),
// swz(r) = (r >> 1) & 7 (g8_swz): the low three position bits of a fragment read are
// (4 (s & 1) + g) ^ swz(fr), gemm8's expression with its k-step s2 = s & 1, and a 256-B row starts at
// bank 0 as a 128-B row does, so the ds_read_b128 of 16 rows x 4 groups meets the banks exactly as
// gemm8's conflict-free read does (checked by writing out both expressions for all 64 lanes and
// every s: identical slot multisets per 16-lane group; no counter run was made).
// Schedule, one unit per iteration, one s_barrier per unit, one loop body:
//   top     s_waitcnt vmcnt(0); s_barrier; B(t) moves to the working registers.  The only
//           operations in flight at the wait are A(t)'s 8 DMAs and B(t)'s 8 loads (4 code vectors +
//           4 scale bytes), issued one whole unit (128 MFMAs per wave) earlier, so the count is 0
//           and nothing younger is held up.  The barrier says that every wave's rows of A(t) are
//           in LDS and that every wave is done reading the other buffer (unit t - 1).
//   issue   A(t+1)'s 8 DMAs into that other buffer, B(t+1)'s 8 loads (last unit: nothing)
//   steps   s = 0..3: 16 conversions, then per 64-row half 4 fragment reads, lgkmcnt(0), 16 MFMAs
//           under s_setprio
// Prologue: A(0), B(0).  nk = 1 runs the loop once and issues nothing in it.
// (A two-set form with counted waits, vmcnt(16) at the top and vmcnt(8) at the bottom of a body
// unrolled by two, spilled 26-38 VGPRs in every instantiation: the accumulators were renamed
// between the copies.  gemm8's four phases and two wave groups stage both operands as LDS
// quadrants; here a unit's B lives in registers, the only LDS traffic is A, and the two waves of a
// SIMD overlap each other's reads and conversions with MFMAs.  DESIGN 22.5.)
// Numerics: products of the bf16 activations and the exactly dequantised bf16 weights, fp32
// accumulation per output in k order: unit by unit, step s = 0..3, the MFMA's own order within its 32
// products; split-K parts (G8Split slabs and tickets) in part order.  No float atomics; two runs are
// bit-identical; row m does not depend on M.
#include "qie_common.hpp"
#include "launch_util.hpp"
#include "gemm_plan.hpp"
#include "gemm8_tile.hpp"
#include "gemm_epilogue.hpp"
#include "fp4_convert.hpp"
#include "../../include/qie/qie_ops.h"

namespace qie {

struct Gemm4Params {
    const uint16_t* A;      // [M][lda] bf16
    int64_t lda;
    const uint8_t* w[3];    // fp4 segments: codes, then e8m0 scales (plain or tiled)
    const uint16_t* b[3];
    int64_t rows[3];        // segment rows (SWIGLU: N, N, 0)
    int64_t n0, n01;
    int64_t M, K, N;
    uint16_t* C;
    int64_t ldc;
};

namespace g4 {
constexpr int ROWB = 256;              // bytes of one A row of a unit (128 bf16)
constexpr int BUF = 256 * ROWB;        // 64 KB
}  // namespace g4

template <int EPI, bool T16>
__global__ __launch_bounds__(512) void gemm4_kernel(Gemm4Params p, int n_mt, G8Split sk) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const G8Lane l = g8_lane();
    const int wid = xcd_major_wid();
    const int tile = wid / sk.splitk, part = wid % sk.splitk;
    const int64_t mt = tile % n_mt, nt = tile / n_mt;
    const int64_t m0 = mt * 256;
    const uint32_t K = (uint32_t)p.K, units = K >> 7;
    const int kb = (int)((int64_t)part * units / sk.splitk);   // this part's units [kb, kb + nk)
    const int nk = (int)((int64_t)(part + 1) * units / sk.splitk) - kb;

    // ---- A: DMA instruction i moves rows 32 wave + 4 i + (lane >> 4); this lane's LDS position
    // lane & 15 of row r holds source chunk c = 4 g' + s' with 4 s' + g' = position ^ swz(r)
    uint32_t aoff[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int r = 32 * l.wave + 4 * i + (l.lane >> 4);
        const int q = (l.lane & 15) ^ g8_swz(r);
        const int c = 4 * (q & 3) + (q >> 2);
        int64_t ar = m0 + r;
        ar = ar < p.M ? ar : p.M - 1;   // rows past M: re-read row M-1, never stored
        aoff[i] = (uint32_t)(ar * p.lda * 2 + c * 16);   // bytes (gemm(): M_pad x ldx fits 32 bits)
    }
    const unsigned char* Ab = reinterpret_cast<const unsigned char*>(p.A);
    auto stage_a = [&](int t) {
        unsigned char* buf = smem + (t & 1) * g4::BUF + 32 * l.wave * g4::ROWB;
        // uniform base + 32-bit lane offset (the saddr form).  The offset goes through an opaque
        // move on purpose: otherwise its zero-extension is hoisted and the eight offsets live as
        // 64-bit per-lane values (16 VGPRs, spilled)
        const unsigned char* src = Ab + (int64_t)(kb + t) * g4::ROWB;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t o;
            asm volatile("v_mov_b32 %0, %1" : "=v"(o) : "v"(aoff[i]));
            glds16(src + o, buf + 4 * i * g4::ROWB);
        }
    };

    // ---- B: the wave's four 16-row weight tiles (wave-uniform segment and tile of each)
    // each tile's resources start AT the tile (and end with the segment's codes / scales), so one
    // lane offset serves the four tiles; a tile past its segment gets an empty range
    __amdgpu_buffer_rsrc_t crs[4], srs[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int sg;
        int64_t r0;   // the tile's first row within its segment
        if constexpr (EPI == QIE_EPI_SWIGLU) {
            sg = j >> 1;
            r0 = nt * 128 + 32 * l.wn + 16 * (j & 1);
        } else {
            const int64_t c0 = nt * 256 + 64 * l.wn + 16 * j;
            sg = c0 < p.n0 ? 0 : (c0 < p.n01 ? 1 : 2);
            r0 = c0 - (sg == 0 ? 0 : (sg == 1 ? p.n0 : p.n01));
        }
        const uint8_t* base = sg == 0 ? p.w[0] : (sg == 1 ? p.w[1] : p.w[2]);
        const int64_t rows = sg == 0 ? p.rows[0] : (sg == 1 ? p.rows[1] : p.rows[2]);
        const int64_t cbytes = rows * (K >> 1), sbytes = rows * (K >> 5);
        const int64_t rc = r0 < rows ? r0 : rows;   // (both layouts: r0 rows of codes / scales precede the tile)
        const int64_t cofs = rc * (K >> 1), sofs = rc * (K >> 5);
        crs[j] = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base + cofs), (short)0, (int)(cbytes - cofs), 0x00020000);
        srs[j] = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base + cbytes + sofs), (short)0, (int)(sbytes - sofs),
                                                   0x00020000);
    }
    const uint32_t cl = T16 ? (uint32_t)l.lane * 16u : (uint32_t)l.fr * (K >> 1) + 16u * l.g;
    const uint32_t sl = T16 ? (uint32_t)l.lane : (uint32_t)l.fr * (K >> 5) + l.g;
    struct BUnit {
        d4_u32x4 wv[4];
        uint32_t sc[4];
    };
    auto load_b = [&](BUnit& b, int t) {
        const uint32_t u = (uint32_t)(kb + t);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            b.wv[j] = __builtin_amdgcn_raw_buffer_load_b128(crs[j], cl + u * (T16 ? 1024u : 64u), 0, 0);
            b.sc[j] = __builtin_amdgcn_raw_buffer_load_b8(srs[j], sl + u * (T16 ? 64u : 4u), 0, 0);
        }
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment read base of this lane: row 128 wm + fr, position g ^ swz(fr) (step s: ^ 4 s)
    const int fbase = (128 * l.wm + l.fr) * g4::ROWB;
    const int fpos = l.g ^ g8_swz(l.fr);
    auto bar = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    auto compute = [&](const BUnit& b, int t) {
        const unsigned char* buf = smem + (t & 1) * g4::BUF + fbase;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            bf16x8 fb[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                fb[j] = __builtin_bit_cast(bf16x8, fp4x8_to_bf16x8(b.wv[j][s], e8m0_scale(b.sc[j])));
#pragma unroll
            for (int h = 0; h < 2; h++) {   // the two 64-row halves of the wave's rows
                bf16x8 fa[4];
#pragma unroll
                for (int i = 0; i < 4; i++)
                    fa[i] = *reinterpret_cast<const bf16x8*>(buf + 16 * (4 * h + i) * g4::ROWB + ((fpos ^ (4 * s)) * 16));
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        acc[4 * h + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[4 * h + i][j], 0, 0, 0);
                __builtin_amdgcn_s_setprio(0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // unit t: its A DMAs and B loads were issued one whole unit earlier, so the one wait is
    // vmcnt(0) (nothing younger is in flight); the barrier behind it says that every wave's part
    // of A(t) is in LDS and that every wave is done reading the other buffer (unit t - 1), which
    // A(t+1) then overwrites while unit t computes.  B(t) moves to `cur` (20 moves per 128 MFMAs)
    // so that the loop has ONE body: with two alternating register sets in a body unrolled by two
    // the accumulators were renamed between the copies and the kernel spilled.
    BUnit cur, nxt;
    stage_a(0);
    __builtin_amdgcn_sched_barrier(0);
    load_b(nxt, 0);
    for (int t = 0; t < nk; t++) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bar();
        cur = nxt;
        if (t + 1 < nk) {   // uniform
            stage_a(t + 1);
            __builtin_amdgcn_sched_barrier(0);
            load_b(nxt, t + 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        compute(cur, t);
    }

    // the lane coordinates again, from an opaque thread index: what the hand-off and the epilogue
    // derive from them (row / column offsets, slab offsets) is then computed here, not hoisted above
    // the loop, where it was held in ~36 VGPRs while the DMA offsets spilled
    int tid2 = threadIdx.x;
    asm volatile("" : "+v"(tid2));
    G8Lane e;
    e.tid = tid2, e.lane = tid2 & 63;
    e.wave = __builtin_amdgcn_readfirstlane(tid2 >> 6);
    e.wm = e.wave >> 2, e.wn = e.wave & 3;
    e.fr = e.lane & 15, e.g = e.lane >> 4;
    if (sk.splitk > 1 && !g8_splitk_merge(sk, tile, part, smem, e, acc)) return;   // uniform
    gemm_epilogue<EPI, 8, 4>(acc, epi_out(p), m0, e.wm * 128, nt * 256 + e.wn * 64, nt * 128 + 32 * e.wn, e.fr, e.g, p.b[0],
                             p.b[1], p.b[2]);
}

// what gemm4_kernel needs of the arguments (qie_linear validated the common part)
static int check_fp4_gemm(const qie_linear_args* a) {
    QIE_REQUIRE(a->K % 128 == 0, "qie_linear: fp4 weights need K %% 128 == 0 (K=%lld)", (long long)a->K);
    QIE_REQUIRE(a->norm_w == nullptr && a->argmax_keys == nullptr,
                "qie_linear: the fp4 GEMM (M > 16) takes no fused norm / arg-max");
    const bool sw = a->epilogue == QIE_EPI_SWIGLU;
    const int64_t s0 = a->seg_rows[0], s1 = a->seg_rows[1], s2 = a->seg_rows[2];
    if (a->flags & QIE_LINEAR_FP4_T16)
        QIE_REQUIRE(sw ? a->N % 16 == 0 : s0 % 16 == 0 && s1 % 16 == 0 && s2 % 16 == 0,
                    "qie_linear: tiled fp4 segments must be whole 16-row tiles");
    // a 16-row weight tile of a wave must lie in one segment: a segment another one follows is whole tiles
    QIE_REQUIRE(sw || !((s0 % 16 != 0 && (s1 > 0 || s2 > 0)) || ((s0 + s1) % 16 != 0 && s2 > 0)),
                "qie_linear: fp4 segments that another segment follows must be whole 16-row tiles");
    // the kernel keeps A offsets (bytes) in 32 bits and weight offsets in a 31-bit buffer range
    QIE_REQUIRE(((int64_t)cdiv(a->M, 256) * 256) * a->ldx * 2 < ((int64_t)1 << 32),
                "qie_linear: fp4 GEMM with M (%lld) x ldx (%lld) >= 2^32 bytes of activations (split the rows)",
                (long long)a->M, (long long)a->ldx);
    for (int s = 0; s < 3; s++)
        QIE_REQUIRE(((sw ? (s < 2 ? a->N : 0) : a->seg_rows[s]) + 256) * (a->K / 2 + a->K / 32) < ((int64_t)1 << 31),
                    "qie_linear: fp4 GEMM: weight segment %d exceeds the 2^31-byte buffer range", s);
    return 0;
}

// gemm() (k_gemm.hip) plans, gets the split-K workspace and hands the launch over
int gemm4_check(const qie_linear_args* a) { return check_fp4_gemm(a); }

int gemm4_launch(const qie_linear_args* a, const GemmPlan& pl, const G8Split& ws, hipStream_t st) {
    const bool sw = a->epilogue == QIE_EPI_SWIGLU;
    Gemm4Params p;
    p.A = (const uint16_t*)a->x;
    p.lda = a->ldx;
    for (int i = 0; i < 3; i++) {
        p.w[i] = (const uint8_t*)a->w[i];
        p.b[i] = (const uint16_t*)a->bias[i];
        p.rows[i] = sw ? (i < 2 ? a->N : 0) : (a->w[i] ? a->seg_rows[i] : 0);
    }
    p.n0 = a->seg_rows[0];
    p.n01 = a->seg_rows[0] + a->seg_rows[1];
    p.M = a->M;
    p.K = a->K;
    p.N = a->N;
    p.C = (uint16_t*)a->y;
    p.ldc = a->ldy;
    const bool t16 = pl.family == GemmFamily::Fp4T16;
    return dispatch_epi(a->epilogue, [&](auto E) {
        constexpr int EPI = decltype(E)::value;
        const void* fn = t16 ? (const void*)gemm4_kernel<EPI, true> : (const void*)gemm4_kernel<EPI, false>;
        QIE_TRY(raise_dynamic_lds(fn, pl.lds_bytes));
        if (t16)
            hipLaunchKernelGGL((gemm4_kernel<EPI, true>), dim3(pl.grid_x), dim3(pl.threads), pl.lds_bytes, st, p, pl.n_mt, ws);
        else
            hipLaunchKernelGGL((gemm4_kernel<EPI, false>), dim3(pl.grid_x), dim3(pl.threads), pl.lds_bytes, st, p, pl.n_mt, ws);
        QIE_LAUNCH_CHECK();
        return 0;
    });
}

}  // namespace qie
