// Host build of csrc/adamw_math.h for tests/test_adamw_cpu.py: the text the device kernel compiles, callable on host arrays,
// so that decay, AMSGrad and masked elements are checked against numpy without a GPU.  With ADAMW_MAIN it is a stand-alone
// program that steps seeded and special-valued buffers of exactly their size (built with the host sanitizers by the same
// test).
#include "adamw_math.h"

// one step over a host array, element by element as the kernel's tail does: the mask bit of element i is bit i & 31 of word i >> 5
extern "C" void adamw_array_host(float* p, const float* g, float* m, float* v, float* vmax, const uint32_t* mask, int64_t n, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, float grad_scale, int64_t step_done) {
    float bc1, bc2;
    fpd_adamw_bias_corrections(beta1, beta2, step_done, &bc1, &bc2);
    const fpd_adamw_coef_t c = fpd_adamw_coefs(lr, beta1, beta2, eps, weight_decay, grad_scale, bc1, bc2);
    const int decay = weight_decay != 0.f;
    for (int64_t i = 0; i < n; ++i) {
        const int ex = decay && mask != 0 && ((mask[i >> 5] >> (uint32_t)(i & 31)) & 1u);
        p[i] = fpd_adamw_update(p[i], g[i], &m[i], &v[i], vmax ? &vmax[i] : 0, decay && !ex, c);
    }
}
extern "C" void adamw_bias_host(float beta1, float beta2, int64_t step_done, float* out) { fpd_adamw_bias_corrections(beta1, beta2, step_done, out, out + 1); }

#if defined(ADAMW_MAIN)
#include <stdio.h>
#include <vector>
int main() {
    int cases = 0;
    const int64_t sizes[5] = {0, 1, 33, 4099, 65537};
    uint64_t state = 0x9e3779b97f4a7c15ull;
    double acc = 0.0;
    for (int z = 0; z < 5; ++z)
        for (int mode = 0; mode < 8; ++mode) {      // bit 0: decay, bit 1: AMSGrad, bit 2: mask
            const size_t n = (size_t)sizes[z];
            std::vector<float> p(n), g(n), m(n, 0.f), v(n, 0.f), x(n, 0.f);
            std::vector<uint32_t> mask((n + 31) / 32, 0u);
            for (size_t i = 0; i < n; ++i) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                p[i] = (float)((double)(state >> 11) / 9007199254740992.0 - 0.5);
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                g[i] = 0.01f * (float)((double)(state >> 11) / 9007199254740992.0 - 0.5);
                if (i % 3 == 1) mask[i >> 5] |= 1u << (i & 31);
            }
            const std::vector<float> p0 = p;
            for (int t = 0; t < 3; ++t)
                adamw_array_host(p.data(), g.data(), m.data(), v.data(), (mode & 2) ? x.data() : 0, (mode & 4) ? mask.data() : 0, sizes[z],
                                 1e-3f, 0.9f, 0.999f, 1e-8f, (mode & 1) ? 0.25f : 0.f, 1.f, t);
            for (size_t i = 0; i < n; ++i) {
                // three steps of at most lr each (|m / denom| <= 1 up to the bias corrections), and a decay that only shrinks
                if (!(fabsf(p[i] - p0[i]) <= 3.5e-3f + 1e-3f * fabsf(p0[i])) || !(v[i] >= 0.f)) { printf("element %zu of %zu left its range (mode %d)\n", i, n, mode); return 1; }
                if ((mode & 2) && !(x[i] >= v[i])) { printf("vmax below v at %zu (mode %d)\n", i, mode); return 1; }
                acc += p[i];
            }
            ++cases;
        }
    // special values: a zero gradient from the first step keeps m, v and a parameter of +-0; a NaN second moment wins the maximum
    float p[4] = {0.f, -0.f, 2.f, 1.f}, g[4] = {0.f, 0.f, 0.f, NAN}, m[4] = {0, 0, 0, 0}, v[4] = {0, 0, 0, 0}, x[4] = {0, 0, 0, 5.f};
    adamw_array_host(p, g, m, v, x, 0, 4, 0.5f, 0.9f, 0.999f, 1e-8f, 0.5f, 1.f, 0);
    if (p[0] != 0.f || signbit(p[0]) || p[1] != 0.f || !signbit(p[1]) || p[2] != 1.5f) { printf("zero gradient\n"); return 1; }
    if (m[0] != 0.f || v[1] != 0.f || x[2] != 0.f || !isnan(x[3]) || !isnan(p[3])) { printf("moments / NaN maximum\n"); return 1; }
    cases += 2;
    printf("adamw_math: %d cases ok (checksum %.6f)\n", cases, acc);
    return 0;
}
#endif
