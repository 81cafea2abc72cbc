// plan_dump — prints the launch plan of linear layers without a GPU: M <= 16 rows by
// plan_linear (linear_plan.hpp); more rows, rows that plan hands to the GEMM, and fp8 activations
// (QIE_LINEAR_ACT_FP8) at any M by plan_gemm (gemm_plan.hpp), in plan_format.hpp's wording.
// Plain host program (`make plan_dump`); tests/test_linear_plan_cpu.py and
// tests/test_gemm_plan_cpu.py compare its output with tables derived by hand,
// tests/test_linear_variants_cpu.py with the instantiations tests/linear_cases.py declares.
//
// stdin, one shape per line:
//   name M K N epilogue norm flags seg0,seg1,seg2 resident_blocks [knob=value ...]
// epilogue: STORE RESIDUAL SWIGLU F32; norm: 0 / 1; flags: the QIE_LINEAR_* bits;
// resident_blocks: what the occupancy query returns for the launch (used where the plan needs
// it); knobs: balanced, blocks_per_cu (Knobs fields), gemm_big, gemm8, sk_grid, sk_mink,
// mx_splitk_max (GemmKnobs fields), allow_split (plan_gemm's argument).  The device has 256 CUs.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../plan_format.hpp"

using namespace qie;

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
            if (epi == epi_name(e)) a.epilogue = e;
        long long s0 = 0, s1 = 0, s2 = 0;
        sscanf(segs.c_str(), "%lld,%lld,%lld", &s0, &s1, &s2);
        a.seg_rows[0] = s0, a.seg_rows[1] = s1, a.seg_rows[2] = s2;
        for (int s = 0; s < 3; s++) a.w[s] = a.seg_rows[s] ? dummy : nullptr;
        a.norm_w = norm ? dummy : nullptr;
        Knobs k;
        GemmKnobs gk;
        bool allow_split = true;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const std::string key = kv.substr(0, eq);
            const int v = atoi(kv.c_str() + eq + 1);
            if (key == "balanced") k.balanced = v;
            else if (key == "blocks_per_cu") k.blocks_per_cu = v;
            else if (key == "gemm_big") gk.gemm_big = v;
            else if (key == "gemm8") gk.gemm8 = v;
            else if (key == "sk_grid") gk.sk_grid = v;
            else if (key == "sk_mink") gk.sk_mink = v;
            else if (key == "mx_splitk_max") gk.mx_splitk_max = v;
            else if (key == "allow_split") allow_split = v != 0;
            else {
                fprintf(stderr, "plan_dump: unknown knob %s\n", key.c_str());
                return 2;
            }
        }
        printf("%s: %s\n", name.c_str(), format_linear_plan(a, k, gk, cus, nb, allow_split).c_str());
    }
    return 0;
}
