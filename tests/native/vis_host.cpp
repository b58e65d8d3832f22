// Host build of csrc/vis_math.h for tests/test_vis_cpu.py: the text the device kernels compile, callable on host arrays, so
// that the per-pixel arithmetic of the debug images is checked against the numpy restatement without a GPU.  With VIS_MAIN it
// is a stand-alone program that walks every blend pair and seeded pixels (built with the host sanitizers by the same test).
#include "vis_math.h"

extern "C" void vis_blend_all_host(uint8_t* out) {          // out[c * 256 + r] for every (table byte c, base byte r)
    for (int c = 0; c < 256; ++c)
        for (int r = 0; r < 256; ++r) out[c * 256 + r] = fpd_vis_blend((uint8_t)c, (uint8_t)r);
}
extern "C" void vis_norm_bytes_host(const float* x, int64_t n, float mn, float mx, int normalize, uint8_t* out) {
    const float neg_min = normalize ? -mn : -0.f;
    const float d = normalize ? fpd_vis_denom(mn, mx) : 1.f;
    for (int64_t i = 0; i < n; ++i) out[i] = fpd_vis_norm_byte(x[i], neg_min, d);
}
extern "C" void vis_heat_bytes_host(const float* x, int64_t n, uint8_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = fpd_vis_heat_byte(x[i]);
}
extern "C" int vis_resize4_host(int a, int b, int c, int d) { return fpd_vis_resize4((uint8_t)a, (uint8_t)b, (uint8_t)c, (uint8_t)d); }
extern "C" int vis_mark_pos_host(int cell, int extent, int padding, double joint) { return fpd_vis_mark_pos(cell, extent, padding, joint); }
extern "C" int vis_trunc_host(double v) { return fpd_vis_trunc(v); }
extern "C" int vis_in_ring_host(int dx, int dy) { return fpd_vis_in_ring(dx, dy); }
extern "C" int vis_in_cross_host(int dx, int dy) { return fpd_vis_in_cross(dx, dy); }

#if defined(VIS_MAIN)
#include <stdio.h>
#include <vector>
int main() {
    std::vector<uint8_t> blend(65536);
    vis_blend_all_host(blend.data());
    long long acc = 0;
    for (int i = 0; i < 65536; ++i) acc += blend[i];
    if (blend[0] != 0 || blend[65535] != 255) { printf("blend ends: %d %d\n", blend[0], blend[65535]); return 1; }
    uint64_t state = 0x9e3779b97f4a7c15ull;
    const int n = 4099;
    std::vector<float> x(n);
    std::vector<uint8_t> out(n);
    for (int round = 0; round < 6; ++round) {
        float mn = 3.4e38f, mx = -3.4e38f;
        for (int i = 0; i < n; ++i) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const double u = (double)(state >> 11) / 9007199254740992.0;
            x[i] = round == 5 ? 0.25f : (float)((u - 0.5) * (round == 4 ? 1e30 : 6.0));
            mn = x[i] < mn ? x[i] : mn;
            mx = x[i] > mx ? x[i] : mx;
        }
        x[0] = NAN;
        vis_norm_bytes_host(x.data(), n, mn, mx, round != 3, out.data());
        for (int i = 0; i < n; ++i) acc += out[i];
        vis_heat_bytes_host(x.data(), n, out.data());
        for (int i = 0; i < n; ++i) acc += out[i];
    }
    const double coords[] = {-1e300, -2147483649.0, -3.5, -0.5, 0.0, 0.999, 7.25, 2147483648.0, 1e300, NAN, INFINITY, -INFINITY};
    for (double c : coords) {
        const int p = vis_mark_pos_host(3, 256, 2, c), t = vis_trunc_host(c);
        for (int dy = -3; dy <= 3; ++dy)
            for (int dx = -3; dx <= 3; ++dx) acc += vis_in_ring_host(p + dx - t, dy) + vis_in_cross_host(dx, t + dy - p);
    }
    acc += vis_resize4_host(255, 255, 255, 255) + vis_resize4_host(0, 0, 0, 1);
    printf("vis_math: cases ok (checksum %lld)\n", acc);
    return 0;
}
#endif
