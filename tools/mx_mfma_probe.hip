// Probe of v_mfma_scale_f32_16x16x128_f8f6f4 semantics on gfx950 (dev tool, one wave):
// lane l holds A row (l & 15), k = 32 (l >> 4) + [0, 32) and B column (l & 15), same k; the
// e8m0 scale byte of the lanes of a row / column scales it.  Checked against a host float64
// product for: unit scales, per-row / per-column scales, data in one k-block only, and
// max-magnitude code pairs.  Measured (r05, profiles/r05_mx_mfma_probe.txt): the result is
// within ~1e-4 of sum|p| of the exact sum, NOT fp32-exact: the instruction's internal sum
// of its 128 products loses bits (case 0-4: 8e-5..1.5e-4) — the accumulation bar of the
// fp8-activation tests (tests/test_gpu_fp8_mx.py MX_ACC_REL) and oracle order 8's model.
// Case 5 (A scales varying per 32-k block within a row) did not follow the per-block lane map
// (r05: 1.17 x sum|p|); r06 prints the error under both candidate maps and names the one the
// hardware follows.  The engine passes one scale per row (every lane of a row the same byte),
// which both maps read identically.
// Integer and needle cases (integer_cases() below; profiles/mx_mfma_probe_integers.txt): small
// integer products added to an integer accumulator are exact while the result stays below 2^23
// ("largest exact L"), and a sum with one nonzero product is that product -- the premises of the
// exact families of tests/mx_cases.py.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void probe(const unsigned char* A, const unsigned char* B, const unsigned char* sa, const unsigned char* sb,
                      float* C, const float* Cin) {
    const int l = threadIdx.x, r = l & 15, g = l >> 4;
    i32x8 a, b;
    for (int i = 0; i < 8; i++) {
        int va = 0, vb = 0;
        for (int j = 0; j < 4; j++) {
            va |= (int)A[r * 128 + 32 * g + 4 * i + j] << (8 * j);
            vb |= (int)B[r * 128 + 32 * g + 4 * i + j] << (8 * j);   // B stored [col][k]
        }
        a[i] = va;
        b[i] = vb;
    }
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    if (Cin)
        for (int i = 0; i < 4; i++) c[i] = Cin[(4 * g + i) * 16 + r];
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, (int)sa[l], 0, (int)sb[l]);
    for (int i = 0; i < 4; i++) C[(4 * g + i) * 16 + r] = c[i];   // row 4g + i, col r
}

static float e4m3(unsigned char b) {
    const int ex = (b >> 3) & 15, man = b & 7;
    float v = ex == 0 ? man / 512.f : std::ldexp(1.f + man / 8.f, ex - 7);
    return (b & 0x80) ? -v : v;
}

// the e4m3 code of a small integer (|v| <= 16: every one is an e4m3 value)
static unsigned char e4m3_of_int(int v) {
    for (int c = 0; c < 256; c++)
        if ((c & 0x7f) != 0x7f && e4m3((unsigned char)c) == (float)v && !(v == 0 && c != 0)) return (unsigned char)c;
    std::abort();
}

// Integer cases (the premise of the exact tests of gemm8mx_kernel, tests/mx_cases.py F1): codes
// that are integers in [-4, 4], so every product is an integer in [-16, 16], added to an
// accumulator input that is an integer of up to 2^L with the result still below 2^L -- with
// unit scales, and with per-row / per-column scales where the accumulator is that integer times
// 2^(ea + eb).  fill 0: codes random in [-4, 4]; 1: all +-4 (the largest sums, cancelling);
// 2: all in [1, 4] (the SwiGLU gate side: the sum only grows).  Also "needles": one nonzero
// product per sum from random codes of all 254 values, scaled (F2).  Prints the elements that
// differ from the exact result per L; returns the largest L up to which none does.
static int integer_cases(unsigned char* dA, unsigned char* dB, unsigned char* dsa, unsigned char* dsb, float* dC) {
    unsigned char hA[16 * 128], hB[16 * 128], hsa[64], hsb[64];
    float hC[256], hCin[256];
    float* dCin;
    hipMalloc(&dCin, sizeof(hCin));
    int exact_L = 0;
    bool all_below = true;
    for (int L = 6; L <= 24; L++) {
        long wrong[2] = {0, 0}, total = 0;
        double worst = 0;
        for (int scaled = 0; scaled < 2; scaled++)
            for (int fill = 0; fill < 3; fill++)
                for (int rep = 0; rep < 4; rep++) {
                    srand(1000 * L + 100 * scaled + 10 * fill + rep);
                    for (int i = 0; i < 16 * 128; i++) {
                        int a, b;
                        if (fill == 0) a = rand() % 9 - 4, b = rand() % 9 - 4;
                        else if (fill == 1) a = (rand() & 1) ? 4 : -4, b = (rand() & 1) ? 4 : -4;
                        else a = 1 + rand() % 4, b = 1 + rand() % 4;
                        hA[i] = e4m3_of_int(a);
                        hB[i] = e4m3_of_int(b);
                    }
                    for (int l = 0; l < 64; l++) {
                        hsa[l] = (unsigned char)(scaled ? 127 + (7 * (l & 15)) % 41 - 20 : 127);
                        hsb[l] = (unsigned char)(scaled ? 127 + (5 * (l & 15)) % 25 - 12 : 127);
                    }
                    double want[256];
                    for (int i = 0; i < 16; i++)
                        for (int j = 0; j < 16; j++) {
                            long s = 0;
                            for (int k = 0; k < 128; k++) s += (long)e4m3(hA[i * 128 + k]) * (long)e4m3(hB[j * 128 + k]);
                            // the accumulator input: an integer with |c + s| < 2^L, half of them
                            // as near +-2^L as that allows
                            const long lim = (1L << L) - 1;
                            long c = (rand() & 1) ? (rand() % (2 * lim + 1)) - lim : ((rand() & 1) ? lim : -lim) - s;
                            if (c + s > lim) c = lim - s;
                            if (c + s < -lim) c = -lim - s;
                            if (c > (1L << 24)) c = 1L << 24;
                            if (c < -(1L << 24)) c = -(1L << 24);
                            const int e = hsa[i] - 127 + hsb[j] - 127;
                            hCin[i * 16 + j] = (float)std::ldexp((double)c, e);
                            want[i * 16 + j] = std::ldexp((double)(c + s), e);
                        }
                    hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice);
                    hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice);
                    hipMemcpy(dsa, hsa, 64, hipMemcpyHostToDevice);
                    hipMemcpy(dsb, hsb, 64, hipMemcpyHostToDevice);
                    hipMemcpy(dCin, hCin, sizeof(hCin), hipMemcpyHostToDevice);
                    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dC, (const float*)dCin);
                    hipMemcpy(hC, dC, sizeof(hC), hipMemcpyDeviceToHost);
                    for (int i = 0; i < 256; i++) {
                        total++;
                        if ((double)hC[i] != want[i]) {
                            wrong[scaled]++;
                            worst = std::fmax(worst, std::fabs((double)hC[i] - want[i]) / std::fabs(want[i] + 1e-300));
                        }
                    }
                }
        std::printf("integers L=%2d: products in [-16, 16], |acc| < 2^%d: wrong %ld (unit scales) + %ld (row / column "
                    "scales) of %ld, worst relative error %.3e\n", L, L, wrong[0], wrong[1], total, worst);
        if (wrong[0] + wrong[1] == 0 && all_below) exact_L = L;
        else all_below = false;
    }
    // needles: A row i has random codes, B column j one nonzero code at k = (37 j + 11 rep) % 128
    long wrong = 0, total = 0;
    for (int rep = 0; rep < 16; rep++) {
        srand(7000 + rep);
        std::memset(hB, 0, sizeof(hB));
        for (int i = 0; i < 16 * 128; i++) {
            unsigned char x = (unsigned char)(rand() & 0xff);
            if ((x & 0x7f) == 0x7f) x &= 0xfe;
            hA[i] = x;
        }
        int kk[16];
        for (int j = 0; j < 16; j++) {
            unsigned char y = (unsigned char)(rand() & 0xff);
            if ((y & 0x7f) == 0x7f) y &= 0xfe;
            if ((y & 0x7f) == 0) y |= 1;
            kk[j] = (37 * j + 11 * rep) % 128;
            hB[j * 128 + kk[j]] = y;
        }
        for (int l = 0; l < 64; l++) {
            hsa[l] = (unsigned char)(127 + (7 * (l & 15) + rep) % 41 - 20);
            hsb[l] = (unsigned char)(127 + (5 * (l & 15) + rep) % 25 - 12);
        }
        hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice);
        hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice);
        hipMemcpy(dsa, hsa, 64, hipMemcpyHostToDevice);
        hipMemcpy(dsb, hsb, 64, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dC, (const float*)nullptr);
        hipMemcpy(hC, dC, sizeof(hC), hipMemcpyDeviceToHost);
        for (int i = 0; i < 16; i++)
            for (int j = 0; j < 16; j++) {
                const double w = std::ldexp((double)e4m3(hA[i * 128 + kk[j]]) * (double)e4m3(hB[j * 128 + kk[j]]),
                                            hsa[i] - 127 + hsb[j] - 127);
                total++;
                if ((double)hC[i * 16 + j] != w) wrong++;   // (-0 == +0 here: the sign of a zero is not counted)
            }
    }
    std::printf("needles: one nonzero product per sum, all 254 codes, row / column scales: wrong %ld of %ld\n", wrong, total);
    hipFree(dCin);
    return exact_L;
}

int main() {
    unsigned char hA[16 * 128], hB[16 * 128], hsa[64], hsb[64];
    float hC[256];
    unsigned char *dA, *dB, *dsa, *dsb;
    float* dC;
    hipMalloc(&dA, sizeof(hA)); hipMalloc(&dB, sizeof(hB)); hipMalloc(&dsa, 64); hipMalloc(&dsb, 64);
    hipMalloc(&dC, sizeof(hC));
    int fails = 0;
    for (int t = 0; t < 9; t++) {
        srand(100 + t);
        for (int i = 0; i < 16 * 128; i++) {
            unsigned char x = (unsigned char)(rand() & 0xff), y = (unsigned char)(rand() & 0xff);
            if ((x & 0x7f) == 0x7f) x &= 0xfe;   // no NaN codes
            if ((y & 0x7f) == 0x7f) y &= 0xfe;
            const int kb = (i % 128) / 32;
            if (t == 2 && kb != 1) x = 0;        // data in k-block 1 only
            if (t == 3 && kb != 3) y = 0;
            // 6: small codes plus one max-magnitude pair per (row, col) at k = 5 (0x7E = 448);
            // 7: the pair at 0x76 (= 240), 8: at 0x70 (= 128)
            if (t >= 6) {
                x &= 0xb7;   // exponent <= 6: |v| < 1
                y &= 0xb7;
                if (i % 128 == 5) { x = t == 6 ? 0x7E : (t == 7 ? 0x76 : 0x70); y = x; }
            }
            hA[i] = x;
            hB[i] = y;
        }
        for (int l = 0; l < 64; l++) {
            hsa[l] = (unsigned char)(t >= 1 ? 127 + ((l & 15) % 5) - 2 : 127);    // per-row scale
            hsb[l] = (unsigned char)(t >= 4 ? 127 + ((l & 15) % 3) - 1 : 127);    // per-column scale
            if (t == 5) hsa[l] = (unsigned char)(127 + (l >> 4) - 1);             // per-k-block scale (rows equal)
        }
        hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice);
        hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice);
        hipMemcpy(dsa, hsa, 64, hipMemcpyHostToDevice);
        hipMemcpy(dsb, hsb, 64, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dC, (const float*)nullptr);
        hipMemcpy(hC, dC, sizeof(hC), hipMemcpyDeviceToHost);
        // scale lane maps: 0 = lane (row + 16 * k-block) scales that row's 32-k block (the
        // per-block reading); 1 = lane `row` (lanes 0..15) scales the row's whole 128-k span
        // (one scale per row, the engine's use: every lane of a row passes the same byte)
        double maxerr[2] = {0, 0};
        for (int map = 0; map < 2; map++)
            for (int i = 0; i < 16; i++)
                for (int j = 0; j < 16; j++) {
                    double s = 0, sabs = 0;
                    for (int k = 0; k < 128; k++) {
                        const int blk = map == 0 ? k / 32 : 0;
                        const double sA = std::ldexp(1.0, hsa[i + 16 * blk] - 127),
                                     sB = std::ldexp(1.0, hsb[j + 16 * blk] - 127);
                        const double p = (double)e4m3(hA[i * 128 + k]) * sA * (double)e4m3(hB[j * 128 + k]) * sB;
                        s += p;
                        sabs += std::fabs(p);
                    }
                    maxerr[map] = std::fmax(maxerr[map], std::fabs(hC[i * 16 + j] - s) / (sabs + 1e-30));
                }
        std::printf("case %d: max |err| / sum|p| = %.3e (per-32-k-block lane map) / %.3e (lane = row, one scale per "
                    "128 k)%s\n", t, maxerr[0], maxerr[1],
                    t == 5 ? "  <- per-k-block A scales: which map the hardware follows" : "");
        if (t != 5 && maxerr[0] > 2e-4) fails++;   // the instruction's own accumulation: ~1e-4 of sum|p|
        if (t == 5) std::printf("case 5 lane map: %s\n", maxerr[0] <= 2e-4 ? "per-32-k-block (lane = row + 16 blk)"
                                                 : (maxerr[1] <= 2e-4 ? "lane = row, one scale per 128 k (lanes 16..63 ignored)"
                                                                      : "neither modelled map"));
        if (t == 5) {
            // fit, per A row i, the scale exponent the hardware applied to each 32-k block b
            // (all (e0..e3) in [-3, 3]^4, least max relative error over the 16 columns): the
            // exponents name the lane group whose scale byte was used (hsa = 126 + lane / 16)
            for (int i = 0; i < 16; i++) {
                double S[4][16];
                for (int b = 0; b < 4; b++)
                    for (int j = 0; j < 16; j++) {
                        double sum = 0;
                        for (int k = 32 * b; k < 32 * b + 32; k++)
                            sum += (double)e4m3(hA[i * 128 + k]) * (double)e4m3(hB[j * 128 + k]) *
                                   std::ldexp(1.0, hsb[j + 16 * b] - 127);
                        S[b][j] = sum;
                    }
                int best[4] = {0, 0, 0, 0};
                double berr = 1e300;
                for (int c = 0; c < 7 * 7 * 7 * 7; c++) {
                    const int e[4] = {c % 7 - 3, (c / 7) % 7 - 3, (c / 49) % 7 - 3, (c / 343) % 7 - 3};
                    double err = 0;
                    for (int j = 0; j < 16; j++) {
                        double v = 0, a = 0;
                        for (int b = 0; b < 4; b++) {
                            v += std::ldexp(S[b][j], e[b]);
                            a += std::fabs(std::ldexp(S[b][j], e[b]));
                        }
                        err = std::fmax(err, std::fabs(hC[i * 16 + j] - v) / (a + 1e-30));
                    }
                    if (err < berr) { berr = err; for (int b = 0; b < 4; b++) best[b] = e[b]; }
                }
                std::printf("case 5 row %2d: fitted block exponents %d %d %d %d (err %.1e); lane groups %d %d %d %d\n", i,
                            best[0], best[1], best[2], best[3], berr, best[0] + 1, best[1] + 1, best[2] + 1, best[3] + 1);
            }
        }
    }
    const int exact_L = integer_cases(dA, dB, dsa, dsb, dC);
    std::printf("largest exact L: %d\n", exact_L);
    std::printf("%s\n", fails ? "FAIL" : "OK");
    return fails ? 1 : 0;
}
