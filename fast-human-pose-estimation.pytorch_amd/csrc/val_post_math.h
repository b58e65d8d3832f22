// The per-sample scalar work of core.function.validate (/root/reference/lib/core/function.py:262-276) for one sample:
//   fpd_val_inverse_affine   utils.transforms.get_affine_transform(c, s, 0, [W, H], inv=1) (transforms.py:57-92) in the
//                            dtypes numpy gives every intermediate: scale * 200 in float32 for float32 boxes, the point
//                            pairs rounded to float32 exactly where the host stores them into its float32 src/dst arrays,
//                            then the float64 solve of  [dst | 1] . X = src  the way numpy.linalg.solve performs it
//                            (dgesv of the OpenBLAS numpy ships): a left-looking LU with partial pivoting (first largest
//                            entry wins, the column below the pivot scaled by the pivot's reciprocal) and two
//                            triangular solves whose substitutions are fused multiply-adds where that library's are.
//                            That operation order is what makes the six doubles equal numpy's to the bit, for every
//                            map size including those whose second pivot is a row swap (H > 2 W).
//   fpd_val_box_area         np.prod(s * 200, 1) in the dtype of s
// Host and device compile the same text (contraction off: only the fma() calls fuse), so a host build is checked against
// numpy without a GPU (tests/test_val_post_cpu.py).
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

// t[6] = the 2x3 heat-map -> image matrix, row-major
FPD_HD static inline void fpd_val_inverse_affine(double c0, double c1, double s0, int box_f32, int W, int H, double* t) {
#pragma clang fp contract(off)
    const double src_w = box_f32 ? (double)((float)s0 * 200.0f) : s0 * 200.0;
    const double up = src_w * -0.5;                       // rot = 0: src_dir = [0 * 1 - up * 0, 0 * 0 + up * 1]
    const double d0 = 0.0 * 1.0 - up * 0.0, d1 = 0.0 * 0.0 + up * 1.0;
    const double dw = (double)W, dh = (double)H;
    float p[3][2], q[3][2];                               // p: image (src), q: heat map (dst)
    p[0][0] = (float)c0; p[0][1] = (float)c1;
    p[1][0] = (float)(c0 + d0); p[1][1] = (float)(c1 + d1);
    q[0][0] = (float)(dw * 0.5); q[0][1] = (float)(dh * 0.5);
    q[1][0] = (float)(dw * 0.5 + 0.0); q[1][1] = (float)(dh * 0.5 + (double)(float)(dw * -0.5));
    for (int k = 0; k < 2; ++k) {                         // get_3rd_point, float32
        float (*v)[2] = k ? q : p;
        const float e0 = v[0][0] - v[1][0], e1 = v[0][1] - v[1][1];
        v[2][0] = v[1][0] + -e1;
        v[2][1] = v[1][1] + e0;
    }
    double A[3][3], B[3][2];
    for (int i = 0; i < 3; ++i) {
        A[i][0] = (double)q[i][0]; A[i][1] = (double)q[i][1]; A[i][2] = 1.0;
        B[i][0] = (double)p[i][0]; B[i][1] = (double)p[i][1];
    }
    // dgetf2, left-looking: column j takes the updates of the columns before it, then the pivot search, the row swap
    // (B's rows go with A's: dlaswp) and the scaling by the pivot's reciprocal
    for (int j = 0; j < 2; ++j) {
        if (j == 1)
            for (int i = 1; i < 3; ++i) A[i][1] = A[i][1] - A[i][0] * A[0][1];
        int piv = j;
        double best = fabs(A[j][j]);
        for (int i = j + 1; i < 3; ++i)
            if (fabs(A[i][j]) > best) { best = fabs(A[i][j]); piv = i; }
        if (piv != j) {
            for (int k = 0; k < 3; ++k) { const double x = A[j][k]; A[j][k] = A[piv][k]; A[piv][k] = x; }
            for (int k = 0; k < 2; ++k) { const double x = B[j][k]; B[j][k] = B[piv][k]; B[piv][k] = x; }
        }
        const double r = 1.0 / A[j][j];
        for (int i = j + 1; i < 3; ++i) A[i][j] = A[i][j] * r;
    }
    A[1][2] = A[1][2] - A[1][0] * A[0][2];
    A[2][2] = A[2][2] - fma(A[2][1], A[1][2], A[2][0] * A[0][2]);
    // dgetrs = two dtrsm: rows 0-1 of the unit-lower solve substitute (fused), row 2 takes one dot product; the upper solve
    // runs row 2, one plain update of rows 0-1, then rows 1-0 (diagonal by reciprocal, fused substitution)
    for (int c = 0; c < 2; ++c) {
        double b0 = B[0][c], b1 = B[1][c], b2 = B[2][c];
        b1 = fma(-b0, A[1][0], b1);
        b2 = b2 - fma(A[2][1], b1, A[2][0] * b0);
        b2 = b2 * (1.0 / A[2][2]);
        b0 = b0 - A[0][2] * b2;
        b1 = b1 - A[1][2] * b2;
        b1 = b1 * (1.0 / A[1][1]);
        b0 = fma(-b1, A[0][1], b0);
        b0 = b0 * (1.0 / A[0][0]);
        t[3 * c] = b0; t[3 * c + 1] = b1; t[3 * c + 2] = b2;
    }
}

// np.prod(s * 200, 1): float32 arithmetic for float32 boxes, widened when stored into the float64 all_boxes
FPD_HD static inline double fpd_val_box_area(double s0, double s1, int box_f32) {
#pragma clang fp contract(off)
    if (box_f32) return (double)(((float)s0 * 200.0f) * ((float)s1 * 200.0f));
    return (s0 * 200.0) * (s1 * 200.0);
}
