// Host build of csrc/dark_math.h for tests/test_dark_cpu.py: the text the device kernel compiles, callable on host values,
// so that the Newton step of the DARK decode is checked against numpy without a GPU.  With DARK_MAIN it is a stand-alone
// program that walks seeded log maps, the guards and det == 0 (built with the host sanitizers by the same test).
#include "dark_math.h"

extern "C" int dark_step_host(const double* v, double* off) { return fpd_dark_step(v, &off[0], &off[1]); }
extern "C" float dark_apply_host(float c, double off) { return fpd_dark_apply(c, off); }
extern "C" int dark_interior_host(int px, int py, int W, int H) { return fpd_dark_interior(px, py, W, H); }
extern "C" void dark_tap_host(int i, int* d) { fpd_dark_tap(i, &d[0], &d[1]); }

#if defined(DARK_MAIN)
#include <stdio.h>
#include <vector>
int main() {
    const int sizes[4][2] = {{12, 16}, {28, 20}, {48, 64}, {8, 10}};      // (W, H)
    uint64_t state = 0x9e3779b97f4a7c15ull;
    double acc = 0.0;
    int n = 0, taken = 0;
    for (int z = 0; z < 4; ++z) {
        const int W = sizes[z][0], H = sizes[z][1];
        std::vector<double> L((size_t)W * H);                             // exactly W*H: a tap outside the map is caught
        for (int k = 0; k < 200; ++k) {
            double u[3];
            for (int i = 0; i < 3; ++i) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                u[i] = (double)(state >> 11) / 9007199254740992.0;
            }
            const double mx = u[0] * (W - 1), my = u[1] * (H - 1);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) L[(size_t)y * W + x] = log(0.3 + u[2]) - ((x - mx) * (x - mx) + (y - my) * (y - my)) / 8.0;
            const int px = (int)(mx + 0.5), py = (int)(my + 0.5);
            ++n;
            if (!fpd_dark_interior(px, py, W, H)) continue;
            double v[FPD_DARK_POINTS], off[2];
            for (int i = 0; i < FPD_DARK_POINTS; ++i) {
                int d[2];
                dark_tap_host(i, d);
                v[i] = L[(size_t)(py + d[1]) * W + (px + d[0])];
            }
            if (!dark_step_host(v, off)) { printf("no step at size %d case %d\n", z, k); return 1; }
            const float cx = dark_apply_host((float)px, off[0]), cy = dark_apply_host((float)py, off[1]);
            // a quadratic log map: the step lands on the centre
            if (!(fabs((double)cx - mx) < 1e-4 && fabs((double)cy - my) < 1e-4)) { printf("off centre at size %d case %d\n", z, k); return 1; }
            acc += cx + cy;
            ++taken;
        }
    }
    double flat[FPD_DARK_POINTS], off[2] = {1.0, 1.0};
    for (int i = 0; i < FPD_DARK_POINTS; ++i) flat[i] = -2.5;
    if (dark_step_host(flat, off) != 0 || off[0] != 0.0 || off[1] != 0.0) { printf("det == 0 took a step\n"); return 1; }
    printf("dark_math: %d cases ok, %d steps (checksum %.6f)\n", n, taken, acc);
    return 0;
}
#endif
