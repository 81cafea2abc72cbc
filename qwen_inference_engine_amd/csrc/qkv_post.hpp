// qkv_post.hpp — the q/k post-projection's arguments and per-pair arithmetic (qk-norm + RoPE),
// shared by the bf16 writer (k_misc.hip qkv_post_kernel) and the fp8-KV writer (k_kv_fp8.hip), so
// that both compute the same q and the same K / V rows before any quantisation.
//
// Block per row, one wave per head.  Each lane owns one RoPE pair:
//   REF: (2*lane, 2*lane+1) interleaved (RoPE.cu:12-18)
//   HF : (lane, lane + hd/2) rotate_half
// qk-norm (Qwen3 only) is the per-head RMSNorm of qk_norm.cu:43-79.
#pragma once
#include "qie_common.hpp"
#include "../../include/qie/qie_ops.h"

namespace qie {

struct QkvPostArgs {
    const uint16_t* qkv;
    const int32_t* pos;
    int rows_per_seq;
    const uint16_t* q_norm;
    const uint16_t* k_norm;
    const float* cs;
    const float* sn;
    int nq, nkv, hd;
    uint16_t* kc;
    uint16_t* vc;
    KvMap km;
    int layer;
    float eps;
    int numerics;
    uint16_t* q_out;
};

// Round 6: the wave's heads are taken in batches of kQkvBatch whose source pairs are all
// loaded before the first store (the row-at-a-time form waited one memory round trip per head,
// nine in a row per wave at Qwen2-7B widths); the arithmetic per element is unchanged.
constexpr int kQkvBatch = 10;

// The ragged form (qie_qkv_post_ragged): the row's sequence comes from a segment table held by
// value in the arguments instead of m / rows_per_seq; nothing else differs.
struct QkvPostRaggedArgs : QkvPostArgs {
    qie_row_segs segs;
};
__device__ __forceinline__ int64_t qkv_row_seq(const QkvPostArgs& a, int64_t m) { return m / a.rows_per_seq; }
__device__ __forceinline__ int64_t qkv_row_seq(const QkvPostRaggedArgs& a, int64_t m) {
    int seq = a.segs.seq[0];   // constant indices only: the table stays in scalar registers
#pragma unroll
    for (int z = 1; z < QIE_RAGGED_MAX_SEGS; z++)
        if (z < a.segs.n && m >= a.segs.row0[z]) seq = a.segs.seq[z];
    return seq;
}

// The lane's pair (elements i0 low, i1 high of `raw`) of one head: qk-norm with weight nw (null:
// none) and RoPE with (c, s) when `rope`; y0 / y1 are the fp32 values whose bf16 rounding is stored.
template <bool HF>
__device__ __forceinline__ void qkv_post_pair(uint32_t raw, bool active, bool rope, const uint16_t* nw, int i0, int i1,
                                              float c, float s, int hd, float eps, float& y0, float& y1) {
#pragma clang fp contract(off)
    float x0 = active ? bf2f((uint16_t)(raw & 0xffffu)) : 0.f;
    float x1 = active ? bf2f((uint16_t)(raw >> 16)) : 0.f;
    if (rope && nw) {
        float ss = wave_sum(x0 * x0 + x1 * x1);
        float rms = sqrtf((ss / (float)hd) + eps);
        if (HF) {
            float inv = 1.0f / rms;
            x0 = rbf(bf2f(nw[i0]) * rbf(x0 * inv));
            x1 = rbf(bf2f(nw[i1]) * rbf(x1 * inv));
        } else {
            x0 = rbf((x0 / rms) * bf2f(nw[i0]));
            x1 = rbf((x1 / rms) * bf2f(nw[i1]));
        }
    }
    y0 = x0;
    y1 = x1;
    if (rope) {
        if (HF) {
            y0 = rbf(rbf(x0 * c) + rbf(-x1 * s));
            y1 = rbf(rbf(x1 * c) + rbf(x0 * s));
        } else {
            y0 = x0 * c - x1 * s;
            y1 = x1 * c + x0 * s;
        }
    }
}

}  // namespace qie
