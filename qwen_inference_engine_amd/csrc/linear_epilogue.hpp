// linear_epilogue.hpp — the epilogue arithmetic the linear kernels share (device only).
#pragma once

#include "qie_common.hpp"
#include "../../include/qie/qie_ops.h"

namespace qie {

// SwiGLU of one output from its fp32 gate and up sums (launch_act + launch_elem, SiLU.cu:10-23):
// both projections round to bf16, a = bf16(g * (1 / (1 + expf(-g)))), y = bf16(u * a).
__device__ __forceinline__ uint16_t swiglu_bf16(float gate, float up) {
#pragma clang fp contract(off)
    const float g = rbf(gate);
    const float u = rbf(up);
    const float a = rbf(g * (1.0f / (1.0f + expf(-g))));
    return f2bf(u * a);
}

// One lane's share of a reduced 16 x 16 output tile in the MFMA C layout: column n, rows
// 4 g + r (skinny_mfma_kernel, dec8_kernel).  c: the sums with the fp8 row scale applied
// (c[1]: the up tile of SWIGLU); ep: RESIDUAL the old values of the four rows, STORE ep[0] the
// bias (0 without one).  STORE with keys: kbest[r] takes the arg-max key of row 4 g + r.
template <int EPI, int NB>
__device__ __forceinline__ void emit_tile16(const float (&c)[NB][4], const float* ep, uint16_t* y, int64_t ldy, int M,
                                            int64_t N, int64_t n, int g, const unsigned long long* keys,
                                            int64_t key_col0, unsigned long long (&kbest)[4]) {
#pragma clang fp contract(off)
    if (n >= N) return;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = 4 * g + r;
        if (i >= M) continue;
        uint16_t* yr = y + (int64_t)i * ldy;
        if constexpr (EPI == QIE_EPI_SWIGLU) {
            yr[n] = swiglu_bf16(c[0][r], c[1][r]);
        } else if constexpr (EPI == QIE_EPI_RESIDUAL) {
            yr[n] = f2bf(ep[r] + rbf(c[0][r]));
        } else if constexpr (EPI == QIE_EPI_F32) {
            reinterpret_cast<float*>(y)[(int64_t)i * ldy + n] = c[0][r];
        } else {
            const uint16_t o = f2bf(c[0][r] + ep[0]);
            yr[n] = o;
            if (keys) {
                const unsigned long long kk = sel_key(bf2f(o), (uint32_t)(n + key_col0));
                kbest[r] = kk > kbest[r] ? kk : kbest[r];
            }
        }
    }
}

}  // namespace qie
