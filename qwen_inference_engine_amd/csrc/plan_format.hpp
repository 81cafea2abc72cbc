// plan_format.hpp — the one wording of a linear layer's launch plan (linear_plan.hpp,
// gemm_plan.hpp).  Host only.  tools/plan_dump.cpp prints it for shapes read from stdin on 256
// CUs; the library's qie_debug_linear_plan prints it for a live argument block on the device's CU
// count with the library's knobs, so a test can assert which instantiation a launch takes.
#pragma once

#include <cstdarg>
#include <cstdio>
#include <string>

#include "gemm_plan.hpp"
#include "linear_plan.hpp"

namespace qie {

inline const char* epi_name(int epi) {
    static const char* names[] = {"STORE", "RESIDUAL", "SWIGLU", "F32"};
    return epi >= 0 && epi < 4 ? names[epi] : "?";
}

inline void plan_appendf(std::string& s, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    s += buf;
}

inline std::string format_gemm_plan(const GemmPlan& g, int epi) {
    std::string s;
    const char* e = epi_name(epi);
    switch (g.family) {
        case GemmFamily::Generic: plan_appendf(s, "gemm_kernel<%s,0>", e); break;
        case GemmFamily::GenericFp8: plan_appendf(s, "gemm_kernel<%s,1>", e); break;
        case GemmFamily::Big256: plan_appendf(s, "gemm_big_kernel<%s,256>", e); break;
        case GemmFamily::Big128: plan_appendf(s, "gemm_big_kernel<%s,128>", e); break;
        case GemmFamily::Gemm8: plan_appendf(s, "gemm8_kernel<%s> splitk=%d", e, g.splitk); break;
        case GemmFamily::Gemm8StreamK:
            plan_appendf(s, "gemm8sk_kernel<%s> dp_rounds=%d chunk=%d", e, g.dp_rounds, g.chunk);
            break;
        case GemmFamily::Mx: plan_appendf(s, "gemm8mx_kernel<%s,0> splitk=%d", e, g.splitk); break;
        case GemmFamily::MxT16: plan_appendf(s, "gemm8mx_kernel<%s,1> splitk=%d", e, g.splitk); break;
    }
    plan_appendf(s, " n_mt=%d tiles=%d slabs=%d tickets=%d grid=%u", g.n_mt, g.tiles, g.slabs, g.tickets, g.grid_x);
    if (g.grid_y != 1) plan_appendf(s, "x%u", g.grid_y);
    plan_appendf(s, " threads=%d lds=%zu", g.threads, g.lds_bytes);
    return s;
}

// One line (no newline) for the launch qie_linear makes of `a`: its routing (fp8 activations and
// M > 16 straight to the GEMM), then plan_linear.  resident_blocks: what the occupancy query
// returns for the launch; <= 0 where it is not known, and a grid that depends on it prints as
// "grid=?".
inline std::string format_linear_plan(const qie_linear_args& a, const Knobs& k, const GemmKnobs& gk, int cus,
                                      int resident_blocks, bool allow_split = true) {
    const bool fp4 = (a.flags & (QIE_LINEAR_FP4 | QIE_LINEAR_FP4_T16)) != 0;   // plan_linear's, at every M
    if (!fp4 && ((a.flags & QIE_LINEAR_ACT_FP8) || a.M > 16)) return format_gemm_plan(plan_gemm(a, gk, cus, allow_split), a.epilogue);
    const LinearPlan pl = plan_linear(a, LinearExtras{}, cus, k);
    std::string s;
    if (pl.error != PlanError::None) {
        plan_appendf(s, "error %d", (int)pl.error);
        return s;
    }
    switch (pl.family) {
        case LinearFamily::Dec8:
            plan_appendf(s, "dec8 KU=%d KS=%d parts=%d", pl.dec8_ku, pl.dec8_ks, pl.dec8_parts);
            return s;
        case LinearFamily::Dec4:
            plan_appendf(s, "dec4 KU=%d KS=%d parts=%d t16=%d", pl.dec4_ku, pl.dec4_ks, pl.dec4_parts,
                         (a.flags & QIE_LINEAR_FP4_T16) ? 1 : 0);
            return s;
        case LinearFamily::Gemm: return format_gemm_plan(plan_gemm(a, gk, cus, allow_split), a.epilogue);
        case LinearFamily::Skinny:
            plan_appendf(s, "skinny_mfma_kernel<%s,%d,%d,4,%d> t16=%d", epi_name(pl.epi), pl.wt, pl.xlds, pl.uo,
                         (int)pl.t16);
            break;
        case LinearFamily::Gemv:
            plan_appendf(s, "gemv_kernel<%d,%d,%s,%d,%d,%d>", pl.mt, pl.rpw, epi_name(pl.epi),
                         pl.uo ? pl.uo : 8, pl.xch, pl.wt);
            if (pl.block_waves) plan_appendf(s, " LB=%d", pl.rpw == 1 ? 1024 : kGemvBalancedThreads);
            plan_appendf(s, " xlds=%d tasks=%lld bpc=%d", pl.xlds, (long long)pl.n_tasks, pl.bpc);
            break;
    }
    if (resident_blocks <= 0 && pl.needs_occupancy()) {
        plan_appendf(s, " grid=? threads=%d lds=%zu", pl.threads(), pl.lds_bytes);
        return s;
    }
    const LaunchGeom g = launch_geometry(pl, cus, resident_blocks);
    plan_appendf(s, " grid=%u threads=%d lds=%zu", g.grid, g.threads, g.lds_bytes);
    return s;
}

}  // namespace qie
