// launch_util.hpp — host-side launch helpers shared by every kernel file.
#pragma once

#include <cstddef>
#include <type_traits>

#include "../../include/qie/qie_ops.h"

namespace qie {

// Dynamic LDS above the default 64 KiB needs hipFuncAttributeMaxDynamicSharedMemorySize raised
// on the kernel, per device.  Does nothing for bytes <= 64 KiB; otherwise remembers, per
// (device, function), the largest limit set so far and raises it only when this launch needs
// more.  Returns 0 or a failure code (qie::fail).  Thread-safe (k_misc.hip).
int raise_dynamic_lds(const void* fn, size_t bytes);

// Blocks of `threads` threads and `shm` bytes of dynamic LDS resident per CU on the current
// device (hipOccupancyMaxActiveBlocksPerMultiprocessor), cached per (device, function,
// threads, shm); `fallback` where the query fails.  Thread-safe.
int resident_blocks_per_cu(const void* fn, int threads, size_t shm, int fallback);

// Runtime epilogue -> compile-time constant: calls f(std::integral_constant<int, E>) for the E
// among EPIS that equals `epi`, the LAST of EPIS otherwise (the sites' former `default:`).
// Only the listed epilogues are instantiated.
template <int E0, int... EPIS, class F>
inline int dispatch_epi(int epi, F&& f) {
    if constexpr (sizeof...(EPIS) == 0) {
        return f(std::integral_constant<int, E0>{});
    } else {
        if (epi == E0) return f(std::integral_constant<int, E0>{});
        return dispatch_epi<EPIS...>(epi, static_cast<F&&>(f));
    }
}
// all four, STORE the default
template <class F>
inline int dispatch_epi(int epi, F&& f) {
    return dispatch_epi<QIE_EPI_SWIGLU, QIE_EPI_RESIDUAL, QIE_EPI_F32, QIE_EPI_STORE>(epi, static_cast<F&&>(f));
}

}  // namespace qie
