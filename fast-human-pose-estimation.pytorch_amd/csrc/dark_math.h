// The Newton step of distribution-aware coordinate decoding (DARK, Zhang et al., CVPR 2020) at one heat-map peak: from the
// 13 values of the log heat map L around (px, py) the central-difference gradient and Hessian, and the offset
// -Hess^-1 grad, in float64 and in the operation order of the numpy restatement (tests/_dark_ref.py):
//   dx  = 0.5  * (L[py][px+1] - L[py][px-1])                                  dy likewise
//   dxx = 0.25 * (L[py][px+2] - 2 * L[py][px] + L[py][px-2])                  dyy likewise
//   dxy = 0.25 * (L[py+1][px+1] - L[py-1][px+1] - L[py+1][px-1] + L[py-1][px-1])
//   det = dxx * dyy - dxy * dxy;  det == 0: no step
//   (ox, oy) = (-(dyy * dx - dxy * dy) / det, -(dxx * dy - dxy * dx) / det)
// fpd_dark_tap(i) names the 13 positions in the order `v` holds them.  Host and device compile the same text with
// contraction off, so a host build is checked against numpy bit for bit without a GPU (tests/test_dark_cpu.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if !defined(FPD_HD)
#if defined(__HIPCC__)
#define FPD_HD __host__ __device__
#else
#define FPD_HD
#endif
#endif

#define FPD_DARK_POINTS 13

// (dx, dy) of value i relative to the peak: centre, the four neighbours, the four at distance 2, the four diagonals
FPD_HD static inline void fpd_dark_tap(int i, int* dx, int* dy) {
    const int8_t ox[FPD_DARK_POINTS] = {0, 1, -1, 0, 0, 2, -2, 0, 0, 1, 1, -1, -1};
    const int8_t oy[FPD_DARK_POINTS] = {0, 0, 0, 1, -1, 0, 0, 2, -2, 1, -1, 1, -1};
    *dx = ox[i];
    *dy = oy[i];
}

// 1 < px < W - 2 and 1 < py < H - 2: all 13 positions lie inside the map
FPD_HD static inline int fpd_dark_interior(int px, int py, int W, int H) { return 1 < px && px < W - 2 && 1 < py && py < H - 2; }

// returns 1 and the offset when the step is taken, 0 (offset 0) when det == 0
FPD_HD static inline int fpd_dark_step(const double* v, double* ox, double* oy) {
#pragma clang fp contract(off)
    const double dx = 0.5 * (v[1] - v[2]);
    const double dy = 0.5 * (v[3] - v[4]);
    const double dxx = 0.25 * (v[5] - 2.0 * v[0] + v[6]);
    const double dyy = 0.25 * (v[7] - 2.0 * v[0] + v[8]);
    const double dxy = 0.25 * (v[9] - v[10] - v[11] + v[12]);
    const double det = dxx * dyy - dxy * dxy;
    *ox = 0.0;
    *oy = 0.0;
    if (!(det != 0.0)) return 0;
    *ox = -(dyy * dx - dxy * dy) / det;
    *oy = -(dxx * dy - dxy * dx) / det;
    return 1;
}

// numpy's `coords[n, p] += offset` (a float32 element, a float64 offset): one rounding of the float64 sum
FPD_HD static inline float fpd_dark_apply(float c, double off) {
#pragma clang fp contract(off)
    return (float)((double)c + off);
}
