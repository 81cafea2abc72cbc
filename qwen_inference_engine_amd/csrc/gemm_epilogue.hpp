// gemm_epilogue.hpp — the epilogue every prefill GEMM kernel ends in (k_gemm.hip, k_gemm_fp4.hip):
// bias / residual / SwiGLU / fp32 from the fp32 accumulator fragments.
#pragma once

#include "qie_common.hpp"
#include "linear_epilogue.hpp"
#include "../../include/qie/qie_ops.h"

namespace qie {

typedef float f32x4_epi __attribute__((ext_vector_type(4)));

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
__device__ __forceinline__ void gemm_epilogue(const f32x4_epi (&acc)[NI][NJ], const EpiOut& o, int64_t m0, int wrow, int64_t col0,
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

}  // namespace qie
