// Host build of csrc/grad_clip_math.h for tests/test_clip_cpu.py: the text the device kernels compile, callable on host
// values, so that norm, coefficient and scale are checked against numpy without a GPU.  With CLIP_MAIN it is a stand-alone
// program that clips seeded and special-valued buffers of exactly their size (built with the host sanitizers by the same
// test).
#include "grad_clip_math.h"

extern "C" float clip_norm_host(double sumsq) { return fpd_clip_norm(sumsq); }
extern "C" float clip_coef_host(float norm, float max_norm) { return fpd_clip_coef(norm, max_norm); }
extern "C" float clip_scale_host(float g, float coef) { return fpd_clip_scale(g, coef); }
// the whole op on a host array, in the device's order of operations behind the sum (the sum itself in array order)
extern "C" void clip_array_host(float* g, int64_t n, float max_norm, float* out) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += (double)g[i] * (double)g[i];
    out[0] = fpd_clip_norm(s);
    out[1] = fpd_clip_coef(out[0], max_norm);
    if (out[1] == 1.0f) return;
    for (int64_t i = 0; i < n; ++i) g[i] = fpd_clip_scale(g[i], out[1]);
}

#if defined(CLIP_MAIN)
#include <stdio.h>
#include <vector>
int main() {
    int cases = 0;
    const int64_t sizes[5] = {0, 1, 3, 4099, 65537};
    uint64_t state = 0x9e3779b97f4a7c15ull;
    double acc = 0.0;
    for (int z = 0; z < 5; ++z) {
        std::vector<float> g((size_t)sizes[z]), g0;
        for (size_t i = 0; i < g.size(); ++i) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            g[i] = (float)((double)(state >> 11) / 9007199254740992.0 - 0.5);
        }
        g0 = g;
        float out[2] = {-1.f, -1.f};
        clip_array_host(g.data(), sizes[z], INFINITY, out);              // measure only: coef 1, nothing moves
        if (out[1] != 1.f || !(out[0] >= 0.f) || g != g0) { printf("max_norm inf moved the gradient (n=%lld)\n", (long long)sizes[z]); return 1; }
        const float norm = out[0];
        clip_array_host(g.data(), sizes[z], norm * 4.f + 1.f, out);      // far above the norm: still untouched
        if (out[1] != 1.f || g != g0) { printf("a large max_norm moved the gradient\n"); return 1; }
        if (sizes[z] > 0) {
            clip_array_host(g.data(), sizes[z], norm * 0.5f, out);       // half the norm: coef 1/2 or just below, norm halves
            if (!(out[1] <= 0.5f && out[1] > 0.49f) || out[0] != norm) { printf("coef %g at half the norm\n", (double)out[1]); return 1; }
            float again[2];
            clip_array_host(g.data(), sizes[z], INFINITY, again);
            if (!(again[0] <= norm * 0.5f * 1.0001f && again[0] >= norm * 0.49f)) { printf("clipped norm %g of %g\n", (double)again[0], (double)norm); return 1; }
            for (size_t i = 0; i < g.size(); ++i) acc += g[i];
        }
        cases += 4;
    }
    // special values: a large element overflows no square; inf gives norm inf, coef 0 under a finite max_norm and NaN under inf;
    // a NaN element gives a NaN norm and coefficient, which the scale writes everywhere
    float big[3] = {1e30f, -1e30f, 1e30f}, out[2];
    clip_array_host(big, 3, 1.f, out);
    if (!isfinite(out[0]) || !(out[1] > 0.f && out[1] < 1e-29f)) { printf("1e30 elements: norm %g coef %g\n", (double)out[0], (double)out[1]); return 1; }
    float a[3] = {1.f, INFINITY, -2.f};
    clip_array_host(a, 3, 1.f, out);
    if (!isinf(out[0]) || out[1] != 0.f || a[0] != 0.f || !isnan(a[1]) || a[2] != 0.f) { printf("inf element\n"); return 1; }
    float b[2] = {1.f, INFINITY};
    clip_array_host(b, 2, INFINITY, out);
    if (!isinf(out[0]) || !isnan(out[1]) || !isnan(b[0])) { printf("inf element under max_norm inf\n"); return 1; }
    float c[2] = {1.f, NAN};
    clip_array_host(c, 2, 1.f, out);
    if (!isnan(out[0]) || !isnan(out[1]) || !isnan(c[0]) || !isnan(c[1])) { printf("NaN element\n"); return 1; }
    float none[1] = {7.f};
    clip_array_host(none, 0, 1.f, out);
    if (out[0] != 0.f || out[1] != 1.f || none[0] != 7.f) { printf("n = 0\n"); return 1; }
    cases += 5;
    printf("grad_clip_math: %d cases ok (checksum %.6f)\n", cases, acc);
    return 0;
}
#endif
