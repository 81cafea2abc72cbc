// fp4_convert.hpp — the MXFP4 kernels' code -> bf16 conversion (k_decode_fp4.hip, k_gemm_fp4.hip).
#pragma once

#include "qie_common.hpp"

namespace qie {

typedef unsigned int d4_u32x4 __attribute__((ext_vector_type(4)));

// eight codes of one MX block -> eight bf16, the kernel's conversion: four
// v_cvt_scalef32_pk_bf16_fp4, byte b of the word = columns 2b (low nibble) and 2b + 1
// (tests/test_gpu_fp4.py checks every code under several exponents: qie_debug_fp4_decode_bf16)
__device__ __forceinline__ d4_u32x4 fp4x8_to_bf16x8(uint32_t w, float sc) {
    const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0);
    const auto p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1);
    const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2);
    const auto p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3);
    return d4_u32x4{__builtin_bit_cast(uint32_t, p0), __builtin_bit_cast(uint32_t, p1), __builtin_bit_cast(uint32_t, p2),
                    __builtin_bit_cast(uint32_t, p3)};
}
// the e8m0 byte as the conversion's scale operand: the f32 with that exponent field
__device__ __forceinline__ float e8m0_scale(uint32_t e) { return __uint_as_float(e << 23); }

}  // namespace qie
