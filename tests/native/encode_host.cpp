// Host build of csrc/encode_math.h for tests/test_encode_cpu.py: the text the device kernel compiles, callable on host
// values, so that the decisions of the unbiased target encoding are checked against numpy without a GPU.  With ENCODE_MAIN
// it is a stand-alone program that renders seeded and designed joints the way the kernel does (row and column factors, then
// their products) into buffers of exactly the map's size (built with the host sanitizers by the same test).
#include "encode_math.h"

extern "C" void encode_place_host(double jx, double jy, double sx, double sy, int sigma, int W, int H, float vis, int has_jw, float jw,
                                  fpd_encode_place_t* o) {
    fpd_encode_place(jx, jy, sx, sy, sigma, W, H, vis, has_jw, jw, o);
}
extern "C" double encode_factor_host(int x, double mu, int sigma) { return fpd_encode_factor(x, mu, sigma); }
extern "C" float encode_value_host(double ex, double ey) { return fpd_encode_value(ex, ey); }
extern "C" int encode_trunc_host(double v) { return fpd_encode_trunc(v); }

#if defined(ENCODE_MAIN)
#include <stdio.h>
#include <vector>
int main() {
    const int sizes[5][3] = {{12, 16, 1}, {28, 20, 2}, {48, 64, 2}, {128, 128, 3}, {5, 7, 1}};      // (W, H, sigma)
    uint64_t state = 0x9e3779b97f4a7c15ull;
    double acc = 0.0;
    int n = 0, drawn = 0;
    for (int z = 0; z < 5; ++z) {
        const int W = sizes[z][0], H = sizes[z][1], sigma = sizes[z][2];
        const double tmp = 3.0 * sigma;
        std::vector<double> ex((size_t)W), ey((size_t)H);
        std::vector<float> map((size_t)W * H);                                // exactly W*H: a pixel outside the map is caught
        for (int k = 0; k < 64; ++k) {
            double u[3];
            for (int i = 0; i < 3; ++i) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                u[i] = (double)(state >> 11) / 9007199254740992.0;
            }
            double mx = -2 * tmp + u[0] * (W + 4 * tmp), my = -2 * tmp + u[1] * (H + 4 * tmp);
            // the designed centres on both sides of the guards, and values no int holds (the other coordinate mid-map)
            if (k < 8) { mx = W / 2.0; my = H / 2.0; }
            if (k == 0) mx = W + tmp;
            if (k == 1) mx = W + tmp - 9.5367431640625e-07;
            if (k == 2) mx = -tmp - 2.0;
            if (k == 3) mx = -tmp - 1.5;
            if (k == 4) my = 1e300;
            if (k == 5) my = -1e300;
            if (k == 6) mx = NAN;
            if (k == 7) my = INFINITY;
            const float vis = u[2] < 0.2 ? 0.f : (u[2] < 0.4 ? 0.5f : 1.f);
            fpd_encode_place_t p;
            encode_place_host(mx * 4.0, my * 3.0, 4.0, 3.0, sigma, W, H, vis, k & 1, 1.25f, &p);
            ++n;
            if (k == 0 || k == 2 || (k >= 4 && k <= 7)) { if (!p.outside || p.drawn || p.weight != 0.f) { printf("case %d of size %d is not outside\n", k, z); return 1; } }
            if ((k == 1 || k == 3) && p.outside) { printf("case %d of size %d is outside\n", k, z); return 1; }
            if (p.drawn != (!p.outside && vis > 0.5f)) { printf("drawn flag of case %d of size %d\n", k, z); return 1; }
            if (!p.drawn) continue;
            for (int x = 0; x < W; ++x) ex[(size_t)x] = encode_factor_host(x, p.mu_x, sigma);
            for (int y = 0; y < H; ++y) ey[(size_t)y] = encode_factor_host(y, p.mu_y, sigma);
            for (int q = 0; q < W * H; ++q) {
                const int y = q / W, x = q - y * W;
                const float v = encode_value_host(ex[(size_t)x], ey[(size_t)y]);
                if (!(v >= 0.f && v <= 1.f)) { printf("value %g at size %d case %d\n", (double)v, z, k); return 1; }
                map[(size_t)q] = v;
                acc += v;
            }
            ++drawn;
        }
    }
    if (encode_trunc_host(-0.5) != 0 || encode_trunc_host(-1.0) != -1 || encode_trunc_host(2.9) != 2 || encode_trunc_host(1e300) != 1073741824) {
        printf("truncation\n");
        return 1;
    }
    printf("encode_math: %d cases ok, %d maps drawn (checksum %.6f)\n", n, drawn, acc);
    return 0;
}
#endif
