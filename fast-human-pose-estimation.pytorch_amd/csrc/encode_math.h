// The per-joint decisions of DARK's unbiased target encoding (include/fpd_amd.h, fpd_targets_unbiased_t): the real-valued
// centre, the integer corners of its 3-sigma box, the outside test, the weight and whether the map is drawn at all, in
// float64 and in the operation order of the numpy restatement (tests/_encode_ref.py):
//   mu = joint / stride                               one division, no + 0.5, no rounding
//   ul = (int)(mu - tmp), br = (int)(mu + tmp + 1)     tmp = 3 * sigma; the cast truncates toward zero like Python's int()
//   outside = ulx >= W || uly >= H || brx < 0 || bry < 0
//   w = outside ? 0 : vis;  written weight = w * joints_weight[j] (float32);  drawn = !outside && w > 0.5f
// fpd_encode_factor is one axis of the separable Gaussian: exp(-(x - mu)^2 / (2 sigma^2)) in float64.
// Host and device compile the same text with contraction off, so a host build is checked against numpy bit for bit without
// a GPU (tests/test_encode_cpu.py).
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

typedef struct {
    double mu_x, mu_y;
    int32_t ulx, uly, brx, bry;
    int32_t outside, drawn;
    float w;                       // vis, or 0 outside: what the drawn decision reads
    float weight;                  // w * joints_weight[j]: what is written
} fpd_encode_place_t;

// (int)v for every double: beyond +-2^30 the cast saturates there (no heat map is that large, so no comparison below
// changes), and a NaN gives INT32_MIN, which the caller never compares (a centre that is not finite is outside)
FPD_HD static inline int32_t fpd_encode_trunc(double v) {
    if (!(v == v)) return INT32_MIN;
    if (v >= 1073741824.0) return 1073741824;
    if (v <= -1073741824.0) return -1073741824;
    return (int32_t)v;
}

// jw: joints_weight[j], read only when has_jw
FPD_HD static inline void fpd_encode_place(double jx, double jy, double stride_x, double stride_y, int sigma, int W, int H,
                                           float vis, int has_jw, float jw, fpd_encode_place_t* o) {
#pragma clang fp contract(off)
    const double tmp = (double)(3 * sigma);
    o->mu_x = jx / stride_x;
    o->mu_y = jy / stride_y;
    o->ulx = fpd_encode_trunc(o->mu_x - tmp);
    o->uly = fpd_encode_trunc(o->mu_y - tmp);
    o->brx = fpd_encode_trunc(o->mu_x + tmp + 1.0);
    o->bry = fpd_encode_trunc(o->mu_y + tmp + 1.0);
    const int finite = (o->mu_x - o->mu_x == 0.0) && (o->mu_y - o->mu_y == 0.0);
    o->outside = !finite || o->ulx >= W || o->uly >= H || o->brx < 0 || o->bry < 0;
    o->w = o->outside ? 0.f : vis;
    o->weight = has_jw ? o->w * jw : o->w;
    o->drawn = !o->outside && o->w > 0.5f;
}

FPD_HD static inline double fpd_encode_factor(int x, double mu, int sigma) {
#pragma clang fp contract(off)
    const double d = (double)x - mu;
    return exp(-(d * d) / (2.0 * (double)sigma * (double)sigma));
}

// one rounding of the float64 product of the two axes' factors
FPD_HD static inline float fpd_encode_value(double ex, double ey) {
#pragma clang fp contract(off)
    return (float)(ex * ey);
}
