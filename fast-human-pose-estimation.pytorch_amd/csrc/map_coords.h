// Heat-map coordinates -> image coordinates, shared by every kernel that writes predictions (infer.hip, dark.hip).
#pragma once
#include "common.h"

// transform_preds (transforms.py:50-55,99-102) in float64, stored as float32: trans[n] . [x, y, 1].  The two rows are written
// out with the fused multiply-adds final_preds_kernel has always been compiled to (x: t0*X first, y: t4*Y first), with
// contraction off, so that every kernel that maps coordinates rounds alike whatever the compiler would choose per call site:
// for float32 boxes the float64 sums sit on float32 rounding ties often enough for the order to show.
__device__ __forceinline__ void map_coords(const double* t, float cx, float cy, float& ox, float& oy) {
#pragma clang fp contract(off)
    const double X = (double)cx, Y = (double)cy;
    ox = (float)(t[2] + fma(t[1], Y, t[0] * X));
    oy = (float)(t[5] + fma(t[3], X, t[4] * Y));
}
