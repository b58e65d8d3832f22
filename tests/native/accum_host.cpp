// Host build of csrc/grad_accum_math.h for tests/test_accum_cpu.py: the text the device kernel compiles, callable on host
// arrays, so that the three modes are checked against numpy without a GPU.  With ACCUM_MAIN it is a stand-alone program
// that runs windows over buffers of exactly their size (built with the host sanitizers by the same test).
#include "grad_accum_math.h"

// one mode over host arrays, element by element as the kernel's scalar path: 0 FIRST, 1 ADD, 2 FIN
extern "C" void accum_array_host(float* grad, float* acc, int64_t n, int mode, float s) {
    for (int64_t i = 0; i < n; ++i) {
        if (mode == 0) acc[i] = fpd_accum_first(grad[i]);
        else if (mode == 1) acc[i] = fpd_accum_add(acc[i], grad[i]);
        else grad[i] = fpd_accum_fin(acc[i], s);
    }
}

#if defined(ACCUM_MAIN)
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
int main() {
    int cases = 0;
    const int64_t sizes[5] = {0, 1, 3, 4099, 65537};
    uint64_t state = 0x9e3779b97f4a7c15ull;
    double sum = 0.0;
    for (int z = 0; z < 5; ++z) {
        const size_t n = (size_t)sizes[z];
        for (int m = 1; m <= 4; ++m) {
            // m identical micro-batches of multiples of 2^-10: the window's mean is the micro-batch itself for m = 1, 2, 4
            std::vector<float> g(n), acc(n, NAN), g0;
            for (size_t i = 0; i < n; ++i) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                g[i] = (float)((int)(state >> 50) - 8192) / 1024.0f;
            }
            g0 = g;
            accum_array_host(g.data(), acc.data(), sizes[z], 0, 0.f);                     // FIRST over a NaN accumulator
            if (n && memcmp(acc.data(), g0.data(), 4 * n) != 0) { printf("FIRST is not a copy (n=%lld)\n", (long long)sizes[z]); return 1; }
            for (int j = 1; j < m; ++j) accum_array_host(g.data(), acc.data(), sizes[z], 1, 0.f);
            if (g != g0) { printf("ADD wrote grad\n"); return 1; }
            const std::vector<float> acc0 = acc;
            accum_array_host(g.data(), acc.data(), sizes[z], 2, (float)(1.0 / m));
            if (n && memcmp(acc.data(), acc0.data(), 4 * n) != 0) { printf("FIN wrote acc\n"); return 1; }
            for (size_t i = 0; i < n; ++i) {
                if (m != 3 && g[i] != g0[i]) { printf("window of %d equal micro-batches: %g != %g\n", m, (double)g[i], (double)g0[i]); return 1; }
                if (m == 3 && !(fabsf(g[i] - g0[i]) <= 1e-6f * fabsf(g0[i]))) { printf("window of 3: %g vs %g\n", (double)g[i], (double)g0[i]); return 1; }
                sum += g[i];
            }
            ++cases;
        }
    }
    // special values: inf - inf and a NaN element give NaN in that element only; -0 + 0 = 0; the copy keeps -0
    float g[5] = {INFINITY, NAN, -0.f, 1.f, -0.f}, acc[5] = {-INFINITY, 1.f, 0.f, 2.f, 9.f};
    accum_array_host(g, acc, 4, 1, 0.f);
    if (!isnan(acc[0]) || !isnan(acc[1]) || acc[2] != 0.f || signbit(acc[2]) || acc[3] != 3.f || acc[4] != 9.f) { printf("ADD specials\n"); return 1; }
    accum_array_host(g, acc, 5, 0, 0.f);
    if (!isinf(acc[0]) || !isnan(acc[1]) || !signbit(acc[2]) || acc[3] != 1.f || !signbit(acc[4])) { printf("FIRST specials\n"); return 1; }
    accum_array_host(g, acc, 5, 2, 0.5f);
    if (!isinf(g[0]) || !isnan(g[1]) || !signbit(g[2]) || g[3] != 0.5f) { printf("FIN specials\n"); return 1; }
    cases += 3;
    printf("grad_accum_math: %d cases ok (checksum %.6f)\n", cases, sum);
    return 0;
}
#endif
