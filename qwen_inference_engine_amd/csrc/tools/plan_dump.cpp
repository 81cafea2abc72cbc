// plan_dump — prints the launch plan of M <= 16 linear layers (linear_plan.hpp) without a GPU.
// Plain host program (`make plan_dump`); tests/test_linear_plan_cpu.py compares its output with
// a table derived by hand.
//
// stdin, one shape per line:
//   name M K N epilogue norm flags seg0,seg1,seg2 resident_blocks [knob=value ...]
// epilogue: STORE RESIDUAL SWIGLU F32; norm: 0 / 1; flags: the QIE_LINEAR_* bits;
// resident_blocks: what the occupancy query returns for the launch (used where the plan needs
// it); knobs: balanced, blocks_per_cu (Knobs fields).  The device has 256 CUs.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../linear_plan.hpp"

using namespace qie;

static const char* kEpi[] = {"STORE", "RESIDUAL", "SWIGLU", "F32"};

int main() {
    const int cus = 256;
    std::string line;
    static const uint16_t dummy[8] = {0};
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        std::string name, epi, segs, kv;
        long long M, K, N;
        int norm, flags, nb;
        if (!(in >> name >> M >> K >> N >> epi >> norm >> flags >> segs >> nb)) {
            fprintf(stderr, "plan_dump: bad line: %s\n", line.c_str());
            return 2;
        }
        qie_linear_args a;
        memset(&a, 0, sizeof(a));
        a.M = M, a.K = K, a.N = N, a.ldx = K, a.ldy = N, a.flags = flags;
        a.x = a.y = (void*)dummy;
        for (int e = 0; e < 4; e++)
            if (epi == kEpi[e]) a.epilogue = e;
        long long s0 = 0, s1 = 0, s2 = 0;
        sscanf(segs.c_str(), "%lld,%lld,%lld", &s0, &s1, &s2);
        a.seg_rows[0] = s0, a.seg_rows[1] = s1, a.seg_rows[2] = s2;
        for (int s = 0; s < 3; s++) a.w[s] = a.seg_rows[s] ? dummy : nullptr;
        a.norm_w = norm ? dummy : nullptr;
        Knobs k;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string key = kv.substr(0, eq);
            const int v = atoi(kv.c_str() + eq + 1);
            if (key == "balanced") k.balanced = v;
            else if (key == "blocks_per_cu") k.blocks_per_cu = v;
            else {
                fprintf(stderr, "plan_dump: unknown knob %s\n", key.c_str());
                return 2;
            }
        }
        const LinearPlan pl = plan_linear(a, LinearExtras{}, cus, k);
        printf("%s:", name.c_str());
        if (pl.error != PlanError::None) {
            printf(" error %d\n", (int)pl.error);
            continue;
        }
        switch (pl.family) {
            case LinearFamily::Dec8:
                printf(" dec8 KU=%d KS=%d parts=%d\n", pl.dec8_ku, pl.dec8_ks, pl.dec8_parts);
                continue;
            case LinearFamily::Gemm: printf(" gemm\n"); continue;
            case LinearFamily::Skinny:
                printf(" skinny_mfma_kernel<%s,%d,%d,4,%d> t16=%d", kEpi[pl.epi], pl.wt, pl.xlds, pl.uo, (int)pl.t16);
                break;
            case LinearFamily::Gemv:
                printf(" gemv_kernel<%d,%d,%s,%d,%d,%d>", pl.mt, pl.rpw, kEpi[pl.epi],
                       pl.uo ? pl.uo : (pl.rpw >= 4 ? 4 : 8), pl.xch, pl.wt);
                if (pl.block_waves) printf(" LB=%d", pl.rpw == 1 ? 1024 : kGemvBalancedThreads);
                printf(" xlds=%d tasks=%lld bpc=%d", pl.xlds, (long long)pl.n_tasks, pl.bpc);
                break;
        }
        const LaunchGeom g = launch_geometry(pl, cus, nb);
        printf(" grid=%u threads=%d lds=%zu\n", g.grid, g.threads, g.lds_bytes);
    }
    return 0;
}
