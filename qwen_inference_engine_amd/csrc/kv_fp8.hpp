// kv_fp8.hpp — the fp8 KV cache's row format in device form (qie_ops.h "fp8 KV cache"): the
// quantiser of a row held 8 elements per lane, the code -> bf16 conversion with the row's scale
// as the conversion's operand, and the addressing of the exponent bytes.  Shared by the writer,
// the expander and the copy (k_kv_fp8.hip) and by the decode attention's KV8 form
// (attn_decode.hpp), so that all of them read and write one format.
#pragma once
#include "qie_common.hpp"
#include "../../include/qie/qie_ops.h"

namespace qie {

// The exponent bytes of an fp8 cache: [L][nkv][run] per sequence / page, i.e. the cache's own
// addressing at one byte per token — `em` is the cache's KvMap with the exponent stride.
struct Kv8Exps {
    uint8_t* ke;
    uint8_t* ve;
    KvMap em;
};
// exponent byte of token `tok` of sequence `seq` in (layer, kv head) lg
template <bool PG>
__device__ __forceinline__ int64_t kv8_exp_off(const KvMap& em, int64_t lg, int64_t seq, int tok) {
    return kv_run_off(em, lg, 1) + kv_tok<PG>(em, seq, tok, 1);
}

// the e8m0 byte as the conversion's scale operand: the f32 with that exponent field
__device__ __forceinline__ float kv8_scale(uint32_t e) { return __uint_as_float(e << 23); }

// eight e4m3 codes x the row scale -> eight bf16: four v_cvt_scalef32_pk_bf16_fp8, the scale
// applied by the conversion itself (a power of two: exact, no multiply issued)
__device__ __forceinline__ uint4 fp8x8_to_bf16x8(uint2 c, float sc) {
    const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)c.x, sc, false);
    const auto p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)c.x, sc, true);
    const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)c.y, sc, false);
    const auto p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)c.y, sc, true);
    return make_uint4(__builtin_bit_cast(uint32_t, p0), __builtin_bit_cast(uint32_t, p1),
                      __builtin_bit_cast(uint32_t, p2), __builtin_bit_cast(uint32_t, p3));
}

// One row quantised by the LPT = hd / 8 lanes that hold it (8 bf16 each, an aligned lane group
// within a 16-lane DPP row): qie_quantize_rows_fp8's quantiser — amax over the row,
// e4m3_row_scale, x / s rounded to nearest even by v_cvt_pk_fp8_f32 — so codes and exponent
// equal that op's bit for bit.  Every lane of the group must be active (DPP reduction).
struct Kv8Row {
    uint2 codes;      // this lane's 8 codes
    uint32_t e;       // the row's e8m0 byte
    uint4 deq;        // this lane's 8 dequantised values (what every later reader sees)
};
template <int LPT>
__device__ __forceinline__ Kv8Row kv8_quantize_row(const uint4& bf8) {
    float x[8];
    unpack8(bf8, x);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) amax = fmaxf(amax, fabsf(x[j]));
    amax = group_max<LPT>(amax);
    const float s = e4m3_row_scale(amax);
    const float inv = 1.0f / s;   // exact: a power of two
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] * inv, x[1] * inv, 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] * inv, x[3] * inv, lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4] * inv, x[5] * inv, 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6] * inv, x[7] * inv, hi, true);
    Kv8Row r;
    r.codes = make_uint2((uint32_t)lo, (uint32_t)hi);
    r.e = (__float_as_uint(s) >> 23) & 0xffu;
    r.deq = fp8x8_to_bf16x8(r.codes, s);
    return r;
}

// Validated exponent addressing of a public fp8 descriptor (k_kv_fp8.hip); `who` names the caller.
int kv8_exps_make(const qie_kv_cache_fp8* c, const KvMap& km, Kv8Exps* out, const char* who);

}  // namespace qie
