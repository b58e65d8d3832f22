// Host build of csrc/val_post_math.h for tests/test_val_post_cpu.py: the text the device kernel compiles, callable on host
// values, so that the inverse affine map is checked against numpy without a GPU.  With VAL_POST_MAIN it is a stand-alone
// program that walks seeded centres and scales (built with the host sanitizers by the same test).
#include "val_post_math.h"

extern "C" void val_inverse_affine_host(const double* c, const double* s, int box_f32, int W, int H, double* t) {
    fpd_val_inverse_affine(c[0], c[1], s[0], box_f32, W, H, t);
}
extern "C" double val_box_area_host(const double* s, int box_f32) { return fpd_val_box_area(s[0], s[1], box_f32); }

#if defined(VAL_POST_MAIN)
#include <stdio.h>
int main() {
    const int sizes[5][2] = {{64, 64}, {48, 64}, {72, 96}, {4, 16}, {8, 8}};
    uint64_t state = 0x9e3779b97f4a7c15ull;
    double acc = 0.0;
    int n = 0;
    for (int z = 0; z < 5; ++z)
        for (int f32 = 0; f32 < 2; ++f32)
            for (int k = 0; k < 300; ++k) {
                double v[4];
                for (int i = 0; i < 4; ++i) {
                    state = state * 6364136223846793005ull + 1442695040888963407ull;
                    v[i] = (double)(state >> 11) / 9007199254740992.0;
                }
                double c[2] = {v[0] * 640.0, v[1] * 480.0}, s[2] = {k ? 0.05 + v[2] * 4.0 : 0.0, 0.05 + v[3] * 4.0}, t[6];
                if (f32) { c[0] = (float)c[0]; c[1] = (float)c[1]; s[0] = (float)s[0]; s[1] = (float)s[1]; }
                val_inverse_affine_host(c, s, f32, sizes[z][0], sizes[z][1], t);
                for (int i = 0; i < 6; ++i)
                    if (!(t[i] == t[i])) { printf("NaN at size %d case %d\n", z, k); return 1; }
                acc += t[2] + t[5] + val_box_area_host(s, f32);
                ++n;
            }
    printf("val_post_math: %d cases ok (checksum %.6f)\n", n, acc);
    return 0;
}
#endif
