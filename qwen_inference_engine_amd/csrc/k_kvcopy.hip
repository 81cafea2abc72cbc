// k_kvcopy.hip — qie_kv_copy: the K and V rows of a range of positions of one sequence copied to
// the same positions of another, every layer and kv head in one launch.
//
// The reference has no such step: its sequences own every page of their linked list
// (iengine.cu:73-109).  Here a fork copies the one partial page (paged) or the whole prefix
// (contiguous), and a writer about to touch a shared page copies the rows below its write.
//
// A pure stream.  Within one (layer, kv head) run the rows of one page (paged) or of the whole
// range (contiguous) are r * head_dim * 2 contiguous bytes on both sides, so the kernel indexes
// 16-byte units u of the range, unit u = (row u / cph, chunk u % cph) with cph = head_dim / 8:
// consecutive lanes move consecutive 16 bytes, a wave 1 KiB per instruction, and only the page
// lookup (one cached table word per unit) differs between the forms.  grid = (units / (4 x
// block), layers x kv heads, {K, V}); each thread issues its four loads before its four stores.
#include "qie_common.hpp"
#include "launch_util.hpp"
#include "../../include/qie/qie_ops.h"

namespace qie {

constexpr int kKvCopyUnroll = 4;

struct KvCopyArgs {
    const uint16_t *sk, *sv;
    uint16_t *dk, *dv;
    KvMap sm, dm;
    int sseq, dseq;
    int pos0, units, cph, hd;
};

// unit u of the range: its 16 bytes of the source run, and where they go in the destination run
template <bool PG>
__device__ __forceinline__ void kv_copy_load(const KvCopyArgs& a, const uint16_t* __restrict__ s, int u, uint4& r,
                                             int64_t& off) {
    const int row = u / a.cph, ch = u - row * a.cph;
    r = *reinterpret_cast<const uint4*>(s + kv_tok<PG>(a.sm, a.sseq, a.pos0 + row, a.hd) + ch * 8);
    off = kv_tok<PG>(a.dm, a.dseq, a.pos0 + row, a.hd) + ch * 8;
}

// (named registers, not arrays: the compiler moved a guarded uint4 r[4] into LDS)
template <bool PG>
__global__ __launch_bounds__(256) void kv_copy_kernel(const KvCopyArgs a) {
    static_assert(kKvCopyUnroll == 4, "four named registers below");
    const int64_t lg = blockIdx.y;
    const uint16_t* __restrict__ s = (blockIdx.z ? a.sv : a.sk) + kv_run_off(a.sm, lg, a.hd);
    uint16_t* __restrict__ d = (blockIdx.z ? a.dv : a.dk) + kv_run_off(a.dm, lg, a.hd);
    const int n = (int)blockDim.x;
    const int u0 = blockIdx.x * (n * kKvCopyUnroll) + threadIdx.x;
    uint4 r0, r1, r2, r3;
    int64_t o0, o1, o2, o3;
    if (u0 + 3 * n < a.units) {   // a full block: four loads in flight, then four stores
        kv_copy_load<PG>(a, s, u0, r0, o0);
        kv_copy_load<PG>(a, s, u0 + n, r1, o1);
        kv_copy_load<PG>(a, s, u0 + 2 * n, r2, o2);
        kv_copy_load<PG>(a, s, u0 + 3 * n, r3, o3);
        *reinterpret_cast<uint4*>(d + o0) = r0;
        *reinterpret_cast<uint4*>(d + o1) = r1;
        *reinterpret_cast<uint4*>(d + o2) = r2;
        *reinterpret_cast<uint4*>(d + o3) = r3;
        return;
    }
    for (int u = u0; u < a.units; u += n) {   // the range's last block
        kv_copy_load<PG>(a, s, u, r0, o0);
        *reinterpret_cast<uint4*>(d + o0) = r0;
    }
}

}  // namespace qie

using namespace qie;

extern "C" int qie_kv_copy(const qie_kv_cache* src, int32_t src_seq, const qie_kv_cache* dst, int32_t dst_seq,
                           int32_t pos0, int32_t n_rows, void* stream) {
    QIE_REQUIRE(src && dst && src_seq >= 0 && dst_seq >= 0 && pos0 >= 0 && n_rows >= 0, "qie_kv_copy: bad arguments");
    QIE_REQUIRE(!src->block_table == !dst->block_table, "qie_kv_copy: one cache is paged, the other contiguous");
    QIE_REQUIRE(src->n_layers == dst->n_layers && src->n_kv_heads == dst->n_kv_heads && src->head_dim == dst->head_dim &&
                    (!src->block_table || src->page_tokens == dst->page_tokens),
                "qie_kv_copy: the caches differ in n_layers, n_kv_heads, head_dim or page_tokens");
    KvMap sm, dm;
    QIE_TRY(kv_map_make(src, &sm, "qie_kv_copy"));
    QIE_TRY(kv_map_make(dst, &dm, "qie_kv_copy"));
    QIE_REQUIRE((int64_t)pos0 + n_rows <= src->max_ctx && (int64_t)pos0 + n_rows <= dst->max_ctx,
                "qie_kv_copy: positions %d..%lld exceed max_ctx %d / %d", pos0, (long long)pos0 + n_rows - 1,
                src->max_ctx, dst->max_ctx);
    const int hd = src->head_dim;
    QIE_REQUIRE(hd % 8 == 0 && src->seq_stride % 8 == 0 && dst->seq_stride % 8 == 0 && ((uintptr_t)src->k % 16) == 0 &&
                    ((uintptr_t)src->v % 16) == 0 && ((uintptr_t)dst->k % 16) == 0 && ((uintptr_t)dst->v % 16) == 0,
                "qie_kv_copy: caches must be 16-byte aligned with head_dim % 8 == 0 and seq_stride % 8 == 0");
    const bool same = src->block_table
                          ? src->k == dst->k && src->block_table + (int64_t)src_seq * src->max_pages ==
                                                    dst->block_table + (int64_t)dst_seq * dst->max_pages
                          : (const uint16_t*)src->k + (int64_t)src_seq * src->seq_stride ==
                                (const uint16_t*)dst->k + (int64_t)dst_seq * dst->seq_stride;
    QIE_REQUIRE(!same, "qie_kv_copy: source and destination are the same sequence of the same cache");
    if (n_rows == 0) return 0;
    const int64_t lg = (int64_t)src->n_layers * src->n_kv_heads;
    const int64_t units = (int64_t)n_rows * (hd / 8);
    QIE_REQUIRE(lg <= 65535 && units <= INT32_MAX / 2, "qie_kv_copy: %lld (layer, kv head) runs of %lld units",
                (long long)lg, (long long)units);
    KvCopyArgs a{(const uint16_t*)src->k, (const uint16_t*)src->v, (uint16_t*)dst->k, (uint16_t*)dst->v, sm, dm,
                 src_seq, dst_seq, pos0, (int)units, hd / 8, hd};
    // grid from the byte count: one wave per run for a few rows, 16 KiB per 256-thread block beyond
    const int block = units <= 64 ? 64 : 256;
    const dim3 grid((unsigned)((units + block * kKvCopyUnroll - 1) / (block * kKvCopyUnroll)), (unsigned)lg, 2);
    hipLaunchKernelGGL((sm.table ? kv_copy_kernel<true> : kv_copy_kernel<false>), grid, dim3(block), 0,
                       (hipStream_t)stream, a);
    QIE_LAUNCH_CHECK();
    return 0;
}
