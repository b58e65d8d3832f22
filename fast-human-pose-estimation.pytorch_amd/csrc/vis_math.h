// The per-pixel arithmetic of utils.vis (the reference's lib/utils/vis.py:20-116) in the dtypes and operation order of the
// host code it replaces -- torch float32 tensor ops, cv2.resize at exactly 4:1, numpy's float64 blend -- so that the canvases
// the device renders equal a host restatement byte for byte (tests/_vis_ref.py):
//   fpd_vis_denom       float32(double(max) - double(min) + 1e-5): the scalar div_() receives
//   fpd_vis_norm_byte   x.add_(-min).div_(d).mul(255).clamp(0, 255).byte(), every step an IEEE float32 operation
//   fpd_vis_heat_byte   heatmap.mul(255).clamp(0, 255).byte()
//   fpd_vis_resize4     cv2.resize INTER_LINEAR at 4:1 on bytes: both taps of either axis weigh 1/2, which the fixed-point
//                       scheme evaluates as (a + b + c + d + 2) >> 2 over the four centre pixels of the 4x4 block
//   fpd_vis_blend       uint8(colored * 0.7 + resized * 0.3) in float64: two products, one sum, truncation
//   fpd_vis_trunc       Python's int() of a float64 coordinate (towards zero), saturated so that the cast is defined
//   fpd_vis_in_ring     the joint mark of save_batch_image_with_joints: 1 <= dx^2 + dy^2 <= 9
//   fpd_vis_in_cross    the peak mark of save_batch_heatmaps: dx^2 + dy^2 == 1
// Host and device compile the same text with contraction off (an fma in the blend or in v * 255 changes bytes), so a host
// build is checked without a GPU (tests/test_vis_cpu.py).
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

FPD_HD static inline float fpd_vis_denom(float mn, float mx) {
#pragma clang fp contract(off)
    return (float)((double)mx - (double)mn + 1e-5);
}

// trunc(clamp(v * 255, 0, 255)); a NaN stays out of the comparisons' way and becomes 0
FPD_HD static inline uint8_t fpd_vis_unit_byte(float v) {
#pragma clang fp contract(off)
    float s = v * 255.0f;
    if (!(s > 0.0f)) s = 0.0f;
    if (s > 255.0f) s = 255.0f;
    return (uint8_t)(int)s;
}

// neg_min = float32(-min); d = fpd_vis_denom(min, max), or neg_min = -0, d = 1 without normalisation
FPD_HD static inline uint8_t fpd_vis_norm_byte(float x, float neg_min, float d) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    const float v = __fdiv_rn(x + neg_min, d);
#else
    const float v = (x + neg_min) / d;
#endif
    return fpd_vis_unit_byte(v);
}

FPD_HD static inline uint8_t fpd_vis_heat_byte(float m) { return fpd_vis_unit_byte(m); }

FPD_HD static inline uint8_t fpd_vis_resize4(uint8_t a, uint8_t b, uint8_t c, uint8_t d) {
    return (uint8_t)(((int)a + (int)b + (int)c + (int)d + 2) >> 2);
}

FPD_HD static inline uint8_t fpd_vis_blend(uint8_t colored, uint8_t resized) {
#pragma clang fp contract(off)
    const double p = (double)colored * 0.7;
    const double q = (double)resized * 0.3;
    return (uint8_t)(int)(p + q);
}

FPD_HD static inline int fpd_vis_trunc(double v) {
    const double lim = 1073741824.0;               // 2^30: far outside any canvas, and +-3 still fit an int
    if (!(v > -lim)) return -(1 << 30);            // (NaN too)
    if (v > lim) return 1 << 30;
    return (int)v;
}

// canvas position of a joint of grid cell (cell_x, cell_y): int(cell * (extent + padding) + padding + joint), float64 sum
FPD_HD static inline int fpd_vis_mark_pos(int cell, int extent, int padding, double joint) {
#pragma clang fp contract(off)
    return fpd_vis_trunc((double)(cell * (extent + padding) + padding) + joint);
}

FPD_HD static inline int fpd_vis_in_ring(int dx, int dy) {
    const long long r = (long long)dx * dx + (long long)dy * dy;
    return r >= 1 && r <= 9;
}

FPD_HD static inline int fpd_vis_in_cross(int dx, int dy) { return (long long)dx * dx + (long long)dy * dy == 1; }
