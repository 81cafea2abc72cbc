// gemm8_tile.hpp — the phase-interleaved 256x256 GEMM tile pipeline (gemm8_kernel,
// gemm8sk_kernel; k_score.hip's score_tile_kernel) and the split-K hand-off (those two and
// gemm8mx_kernel); k_gemm.hip and k_score.hip include it.  gemm8mx_kernel runs the same schedule
// from its own copy (see there).
//
// Prefill GEMM, phase-interleaved (round 4; cdna_hip_programming.md §5 "The 256² 8-phase
// template", written for this NT layout).  256x256 block tile, BK = 64, 8 waves as 2 (M) x 4
// (N), 128x64 per wave = 8x4 accumulators; LDS = two 64-KB k-tile buffers (A rows then W
// rows, 128-B rows, 16-B chunk c of row r at c ^ ((r >> 1) & 7): conflict-free
// ds_read_b128 for the 16x16x32 fragments).  A k-tile is consumed in FOUR phases, one C
// quadrant (64 x 32 per wave, 16 MFMAs) each:
//   P1 (qa0, qb0) reads A[qa0] + B[qb0]    P2 (qa0, qb1) reads B[qb1]
//   P3 (qa1, qb1) reads A[qa1]             P4 (qa1, qb0) (B[qb0] kept in registers)
// and the k-tile is staged as four 16-KB units in the order it is read: UA0 (the qa0 A rows
// of both M halves), UB0, UB1, UA1 (2 LDS-DMA instructions per wave each).  Phase P3 of tile
// t stages UA0(t+2), P4 UB0(t+2), P1 of t+1 UB1(t+2), P2 of t+1 UA1(t+2): every unit lands in
// its buffer >= 2 phases after the last read of what it overwrites, and is read 5-6 phases
// after it was issued.  Each phase = [fragment reads, one unit's DMAs, the counted wait]
// s_barrier [lgkmcnt(0), 16 MFMAs] s_barrier; the wait is vmcnt(8) at the end of P4, P1,
// P2 (the unit read next phase has landed; 4 units stay in flight), never 0 before the
// last two tiles.  Waves 4-7 run one barrier behind waves 0-3 (an extra s_barrier before the
// loop, waves 0-3 one after it), so on every SIMD one wave's MFMAs overlap the other
// wave's reads and DMA issue.  Accumulation order per output = k order (as gemm_big).
//
// The operand policy (G8Bf16 below) supplies what a different operand format would change: the
// fragment types and reads, the MFMAs of one quadrant, and the source address of a DMA.
#pragma once

#include "qie_common.hpp"

namespace qie {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4_g8 __attribute__((ext_vector_type(4)));
typedef int i32x8_mx __attribute__((ext_vector_type(8)));

namespace g8 {
constexpr int BM = 256, BN = 256, BK = 64;
constexpr int BUF = (BM + BN) * BK * 2;   // 64 KB: A rows [0, 256) then W rows, 128 B each
}  // namespace g8
namespace mx {
constexpr int BK = 128;   // codes per k-tile row (128 B)
}

__device__ __forceinline__ int g8_swz(int r) { return (r >> 1) & 7; }

__device__ __forceinline__ void glds16(const void* src, void* lds) {
    __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(src),
                                     (__attribute__((address_space(3))) void*)(lds), 16, 0, 0);
}

// thread coordinates of the 8-wave (2 x 4) kernels
struct G8Lane {
    int tid, lane, wave, wm, wn, fr, g;
};
__device__ __forceinline__ G8Lane g8_lane() {
    G8Lane l;
    l.tid = threadIdx.x, l.lane = l.tid & 63;
    l.wave = __builtin_amdgcn_readfirstlane(l.tid >> 6);
    l.wm = l.wave >> 2, l.wn = l.wave & 3;
    l.fr = l.lane & 15, l.g = l.lane >> 4;
    return l;
}

// bijective XCD remap (cdna_hip_programming.md §5 'XCD swizzle must be bijective'): XCD-major
// workgroup index, so consecutive indices (consecutive tiles, which share a weight tile, and the
// parts of one tile) sit on one XCD's L2
__device__ __forceinline__ int xcd_major_wid() {
    const int nwg = gridDim.x, orig = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = orig & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
}

// DMA units: unit u (0 UA0, 1 UB0, 2 UB1, 3 UA1), instruction i of this wave moves the
// 8-row block b = 2 wave + i of the unit; lane -> row + (lane >> 3), LDS chunk lane & 7
// (holding source chunk (lane & 7) ^ swz(row)).  dst_row: tile row of the block (A: 0..255,
// W: 0..255), wave-uniform.  map() calls src_of(u, i, r, cs) with this lane's tile row r and
// source chunk cs of every (unit, instruction).
struct G8Units {
    int dst_row[4][2];
    template <class F>
    __device__ __forceinline__ void map(const G8Lane& l, F&& src_of) {
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int b = 2 * l.wave + i;
                int row0;
                if (u == 0 || u == 3) row0 = (b < 8 ? 8 * b : 128 + 8 * (b - 8)) + (u == 3 ? 64 : 0);
                else row0 = 64 * (b >> 2) + 8 * (b & 3) + (u == 2 ? 32 : 0);
                dst_row[u][i] = row0;
                const int r = row0 + (l.lane >> 3);
                const int cs = (l.lane & 7) ^ g8_swz(r);
                src_of(u, i, r, cs);
            }
    }
};

// ------------------------------------------------------------------ operand policy
// bf16 (v_mfma_f32_16x16x32_bf16): fragments bf16x8[.][2] (two 32-deep k-steps per k-tile), 16
// MFMAs per phase, one 64-bit source pointer per DMA.
struct G8Bf16 : G8Units {
    using FragA = bf16x8[4][2];
    using FragB = bf16x8[2][2];
    const uint16_t* src[4][2];
    int kb = 0;   // first k-tile of the range the pipeline runs

    __device__ __forceinline__ const void* unit_src(int u, int i, int kt) const {
        const int64_t k0 = (int64_t)(kb + kt) * g8::BK;
        return src[u][i] + k0;
    }
    __device__ __forceinline__ void read_a(const G8Lane& l, const unsigned char* buf, int qa, FragA& fa) const {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
                const int row = 128 * l.wm + 64 * qa + 16 * i + l.fr;
                fa[i][s2] = *reinterpret_cast<const bf16x8*>(buf + row * 128 + (((4 * s2 + l.g) ^ g8_swz(row)) * 16));
            }
    }
    __device__ __forceinline__ void read_b(const G8Lane& l, const unsigned char* buf, int qb, FragB& fb) const {
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
                const int row = 64 * l.wn + 32 * qb + 16 * j + l.fr;
                fb[j][s2] = *reinterpret_cast<const bf16x8*>(buf + g8::BM * 128 + row * 128 +
                                                             (((4 * s2 + l.g) ^ g8_swz(row)) * 16));
            }
    }
    __device__ __forceinline__ void mfma(int qa, int qb, const FragA& fa, const FragB& fb, f32x4 (&acc)[8][4]) const {
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 2; j++)
                    acc[4 * qa + i][2 * qb + j] =
                        __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][s2], fb[j][s2], acc[4 * qa + i][2 * qb + j], 0, 0, 0);
    }
};

// ------------------------------------------------------------------ the pipeline
// k-tiles [op.kb, op.kb + nk) of the tile op.map() was given, into acc (zeroed here).
// NK1: nk may be 1 (the second k-tile's prologue units are then not staged).  gemm8_kernel's
// launches always have nk >= 4 and keep the unguarded prologue.
template <bool NK1, class Op>
__device__ __forceinline__ void g8_pipeline(Op& op, const G8Lane& l, unsigned char* smem, int nk, f32x4 (&acc)[8][4]) {
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    typename Op::FragA fa;
    typename Op::FragB fb0, fb1;

    auto stage = [&](int u, int kt) {   // unit u of local k-tile kt into buffer kt & 1
        unsigned char* buf = smem + (kt & 1) * g8::BUF + ((u == 0 || u == 3) ? 0 : g8::BM * 128);
#pragma unroll
        for (int i = 0; i < 2; i++) glds16(op.unit_src(u, i, kt), buf + op.dst_row[u][i] * 128);
    };
    auto mfma_q = [&](int qa, int qb, const typename Op::FragB& fb) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        op.mfma(qa, qb, fa, fb, acc);
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

    // prologue: UA0(0) UB0(0) UB1(0) UA1(0) UA0(1) UB0(1); P1(0) reads UA0(0), UB0(0)
    stage(0, 0); stage(1, 0); stage(2, 0); stage(3, 0);
    if (!NK1 || nk > 1) {   // uniform
        stage(0, 1); stage(1, 1);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    bar();
    if (l.wm == 1) bar();   // waves 4-7 one barrier behind
    for (int t = 0; t < nk; t++) {
        const unsigned char* buf = smem + (t & 1) * g8::BUF;
        const bool tail = t >= nk - 2;
        // ---- P1 (qa0, qb0): reads A[qa0], B[qb0]; stages UB1(t+1); retires UB1(t)
        op.read_b(l, buf, 0, fb0);
        __builtin_amdgcn_sched_barrier(0);
        op.read_a(l, buf, 0, fa);
        __builtin_amdgcn_sched_barrier(0);
        if (t + 1 < nk) stage(2, t + 1);
        wait8(tail);
        bar();
        mfma_q(0, 0, fb0);
        bar();
        // ---- P2 (qa0, qb1): reads B[qb1]; stages UA1(t+1); retires UA1(t)
        op.read_b(l, buf, 1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        if (t + 1 < nk) stage(3, t + 1);
        wait8(tail);
        bar();
        mfma_q(0, 1, fb1);
        bar();
        // ---- P3 (qa1, qb1): reads A[qa1]; stages UA0(t+2)
        op.read_a(l, buf, 1, fa);
        __builtin_amdgcn_sched_barrier(0);
        if (t + 2 < nk) stage(0, t + 2);
        bar();
        mfma_q(1, 1, fb1);
        bar();
        // ---- P4 (qa1, qb0): B[qb0] from registers; stages UB0(t+2); retires UA0/UB0(t+1)
        if (t + 2 < nk) stage(1, t + 2);
        wait8(tail);
        bar();
        mfma_q(1, 0, fb0);
        bar();
    }
    if (l.wm == 0) bar();   // balance the barrier count of the two wave groups
}

// ------------------------------------------------------------------ split-K hand-off
// Split-K (tiles < CUs: Qwen2-7B O / down at 2,048 rows have 112 256x256 tiles, QKV 144): the
// k-tiles of a tile are cut into `splitk` consecutive parts, one workgroup each (the remap
// keeps a tile's parts on one XCD).  Every part stores its fp32 accumulators write-through
// (sc1) into its slab [tile][part] (256 KB, each lane's 16-B accumulator quads in fragment
// order), drains, and adds to the tile's ticket; the part whose add comes last sums the slabs
// in PART order (sc1 loads: cdna_hip_programming.md §5 'Projection GEMM' item 2), so the result
// does not depend on arrival order, runs the epilogue and resets the ticket.
struct G8Split {
    int splitk;
    float* slab;       // [tiles][splitk][256 * 256] fp32
    unsigned* cnt;     // [tiles], zero at rest
};
constexpr int kG8SlabFloats = g8::BM * g8::BN;

// this wave's quads: slab float offset ((wave * 32 + i * 4 + j) * 64 + lane) * 4
__device__ __forceinline__ int g8_slab_off(const G8Lane& l, int i, int j) {
    return ((l.wave * 32 + i * 4 + j) * 64 + l.lane) * 16;
}
// store acc into the slab (write-through); every storing wave drains, then the block meets
__device__ __forceinline__ void g8_slab_store(float* slab, const G8Lane& l, const f32x4 (&acc)[8][4]) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(slab, (short)0, kG8SlabFloats * 4, 0x00020000);
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_g8, acc[i][j]), rs, g8_slab_off(l, i, j), 0, 16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains
    __syncthreads();
}
// one add to the tile's ticket per workgroup; true (block-uniform) in the workgroup whose add
// found `last`, i.e. came after every other one's.  The flag sits at the start of the staging
// array, which is free (one LDS object).
__device__ __forceinline__ bool g8_ticket_last(unsigned* cnt, unsigned last, unsigned char* smem, const G8Lane& l) {
    int* flag = reinterpret_cast<int*>(smem);
    if (l.tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = old == last ? 1 : 0;
    }
    __syncthreads();
    return *flag != 0;
}
__device__ __forceinline__ void g8_ticket_reset(unsigned* cnt, const G8Lane& l) {
    if (l.tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// acc = slab (first) or acc + slab
__device__ __forceinline__ void g8_slab_sum(const float* slab, bool first, const G8Lane& l, f32x4 (&acc)[8][4]) {
#pragma clang fp contract(off)
    const auto rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(slab), (short)0, kG8SlabFloats * 4, 0x00020000);
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rq, g8_slab_off(l, i, j), 0, 16));
            acc[i][j] = first ? v : acc[i][j] + v;
        }
}
// The whole hand-off of part `part` of `tile`; false (block-uniform) in every part but the one
// that arrived last, which leaves with the tile's sum in acc.
__device__ __forceinline__ bool g8_splitk_merge(const G8Split& sk, int tile, int part, unsigned char* smem, const G8Lane& l,
                                                f32x4 (&acc)[8][4]) {
    const int64_t tb = (int64_t)tile * sk.splitk;
    g8_slab_store(sk.slab + (tb + part) * kG8SlabFloats, l, acc);
    if (!g8_ticket_last(sk.cnt + tile, (unsigned)sk.splitk - 1, smem, l)) return false;   // uniform
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < sk.splitk; q++)   // part order: independent of who arrived last
        g8_slab_sum(sk.slab + (tb + q) * kG8SlabFloats, q == 0, l, acc);
    g8_ticket_reset(sk.cnt + tile, l);
    return true;
}

}  // namespace qie
