// Host build of csrc/ema_math.h for tests/test_ema_cpu.py: the text the device kernel compiles, callable on host values, so
// that the weight schedule and the update rule are checked against numpy without a GPU.  With EMA_MAIN it is a stand-alone
// program that walks the schedule over the crossing of the warm-up ramp and updates seeded and special values in buffers of
// exactly their size (built with the host sanitizers by the same test).
#include "ema_math.h"

extern "C" float ema_weight_host(int64_t updates_done, double decay, int warmup) { return fpd_ema_weight(updates_done, decay, warmup); }
extern "C" float ema_update_host(float e, float x, float w) { return fpd_ema_update(e, x, w); }
extern "C" void ema_update_array_host(float* e, const float* x, int64_t n, float w) {
    for (int64_t i = 0; i < n; ++i) e[i] = fpd_ema_update(e[i], x[i], w);
}

#if defined(EMA_MAIN)
#include <math.h>
#include <stdio.h>
#include <vector>
int main() {
    // the schedule: never above 1 - 0 = 1, never below 1 - decay, non-increasing in the number of updates
    const double decays[4] = {0.0, 0.5, 0.999, 0.9998};
    int n = 0;
    for (int z = 0; z < 4; ++z)
        for (int warm = 0; warm < 2; ++warm) {
            float prev = 2.f;
            for (int64_t u = 0; u < 60000; u += (u < 64 ? 1 : 997)) {
                const float w = ema_weight_host(u, decays[z], warm);
                if (!(w <= 1.f && w >= (float)(1.0 - decays[z]) && w <= prev)) { printf("weight %g at u=%lld decay=%g warm=%d\n", (double)w, (long long)u, decays[z], warm); return 1; }
                if (!warm && w != (float)(1.0 - decays[z])) { printf("weight without warm-up\n"); return 1; }
                prev = w;
                ++n;
            }
        }
    if (ema_weight_host(0, 0.9998, 1) != (float)(1.0 - 2.0 / 11.0)) { printf("first warm-up weight\n"); return 1; }
    // (1 + u) / (10 + u) reaches 0.9998 at u = 44 990: below it the ramp rules, above it the decay
    if (ema_weight_host(44979, 0.9998, 1) == ema_weight_host(44999, 0.9998, 1) || ema_weight_host(44999, 0.9998, 1) != (float)(1.0 - 0.9998)) {
        printf("crossing of the ramp\n");
        return 1;
    }
    // the update: buffers of exactly n elements; decay 0 (w = 1) lands on a source within a factor 2 of the average
    const int64_t sizes[4] = {1, 3, 4099, 65537};
    uint64_t state = 0x9e3779b97f4a7c15ull;
    double acc = 0.0;
    for (int z = 0; z < 4; ++z) {
        std::vector<float> e((size_t)sizes[z]), x((size_t)sizes[z]);
        for (size_t i = 0; i < e.size(); ++i) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            e[i] = (float)((double)(state >> 11) / 9007199254740992.0 - 0.5);
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            x[i] = e[i] * (1.f + 0.01f * (float)((double)(state >> 11) / 9007199254740992.0 - 0.5));      // within a factor 2 of e
        }
        for (int k = 0; k < 3; ++k) ema_update_array_host(e.data(), x.data(), sizes[z], ema_weight_host(k, 0.9998, 1));
        for (size_t i = 0; i < e.size(); ++i) acc += e[i];
        ema_update_array_host(e.data(), x.data(), sizes[z], ema_weight_host(0, 0.0, 0));
        for (size_t i = 0; i < e.size(); ++i)
            if (e[i] != x[i]) { printf("decay 0 does not land on the source at %zu\n", i); return 1; }      // x - e is exact (Sterbenz)
        n += 4;
    }
    const float special[8] = {0.f, -0.f, 1e-45f, -1e-45f, INFINITY, -INFINITY, NAN, 3.4028235e38f};
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) {
            const float r = ema_update_host(special[i], special[j], 0.25f);
            if ((isnan(special[i]) || isnan(special[j])) && !isnan(r)) { printf("NaN does not stay NaN\n"); return 1; }
            ++n;
        }
    printf("ema_math: %d cases ok (checksum %.6f)\n", n, acc);
    return 0;
}
#endif
