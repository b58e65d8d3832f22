// The scalar part of JointsDataset.__getitem__ (/root/reference/lib/dataset/JointsDataset.py:137-167) and
// utils.transforms.get_affine_transform (transforms.py:57-110) for one sample, in the dtypes numpy gives every
// intermediate (numpy >= 2 promotion: a Python scalar adopts the array's dtype, a numpy float64 scalar does not):
//   half-body        float32 throughout (selected joints cast to float32; Python-float aspect_ratio, 1.0, 1.5 and the int
//                    pixel_std enter as float32); mean = sequential float32 sum in joint order / count
//   scale jitter     s * np.float64 -> float64 whatever s was
//   flipped centre   width - c[0] - 1 in the dtype of c: float32 after a half-body crop or for float32 boxes, else float64
//   scale * 200.0    float32 only for a float32 scale that was never jittered (validation mode)
//   point pairs      rounded to float32 exactly where the reference stores them into its float32 src/dst arrays
//   matrix           float64 solve of the three point pairs, then cv::invertAffineTransform's expression
// Host and device compile the same text (contraction off: every product and sum is rounded like numpy's), so the host
// build can be checked against the fixture without a GPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fpd_amd.h"

#if defined(__HIPCC__)
#define FPD_HD __host__ __device__
#else
#define FPD_HD
#endif

struct fpd_aug_sample_t {
    double c[2], s[2], r;
    int32_t flip;
    double trans[6], minv[6];
};

FPD_HD static inline double fpd_clipd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// half_body_transform (JointsDataset.py:65-108); false = None, None (c and s are kept)
FPD_HD static inline bool fpd_half_body(const fpd_augment_t& a, const double* jt, const float* vs, double n_half, float* c, float* s) {
#pragma clang fp contract(off)
    const int J = a.db.J;
    int nu = 0, nl = 0;
    for (int j = 0; j < J; ++j)
        if (vs[j] > 0.f) (a.db.upper[j] ? nu : nl) += 1;
    const bool upper = (n_half < 0.5 && nu > 2) ? true : !(nl > 2);
    const int n = upper ? nu : nl;
    if (n < 2) return false;
    float sx = 0.f, sy = 0.f, x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
    for (int j = 0; j < J; ++j) {
        if (!(vs[j] > 0.f) || (a.db.upper[j] != 0) != upper) continue;
        const float x = (float)jt[3 * j], y = (float)jt[3 * j + 1];
        sx += x; sy += y;
        x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
    }
    c[0] = (float)((double)sx / (double)n);            // np.mean: sum / intp count, evaluated in float64, stored float32
    c[1] = (float)((double)sy / (double)n);
    float w = x1 - x0, h = y1 - y0;
    const float ar = (float)a.db.aspect_ratio, ps = (float)a.db.pixel_std;
    if (w > ar * h) h = w * 1.0f / ar;
    else if (w < ar * h) w = h * ar;
    s[0] = (w * 1.0f / ps) * 1.5f;
    s[1] = (h * 1.0f / ps) * 1.5f;
    return true;
}

// sample b of the batch, image i of the database (already range-checked)
FPD_HD static inline void fpd_augment_sample(const fpd_augment_t& a, int b, int i, fpd_aug_sample_t& o) {
#pragma clang fp contract(off)
    const int J = a.db.J;
    const double* jt = a.db.joints + (size_t)i * J * 3;
    const float* vs = a.db.vis + (size_t)i * J;
    const double width = (double)a.db.images[i].w;
    double c0 = a.db.center[2 * i], c1 = a.db.center[2 * i + 1], s0 = a.db.scale[2 * i], s1 = a.db.scale[2 * i + 1];
    bool c_f32 = a.db.box_f32 != 0, s_f32 = a.db.box_f32 != 0;
    double r = 0.0;
    int flip = 0;
    if (a.is_train) {
        const double* dr = a.draws + (size_t)b * a.draw_stride;
        double nvis = 0.0;
        for (int j = 0; j < J; ++j) nvis += (double)vs[j];
        if (nvis > (double)a.num_joints_half_body && dr[0] < a.prob_half_body) {
            float hc[2], hs[2];
            if (fpd_half_body(a, jt, vs, dr[1], hc, hs)) {
                c0 = hc[0]; c1 = hc[1]; s0 = hs[0]; s1 = hs[1];
                c_f32 = true;
            }
        }
        const double f = fpd_clipd(dr[2] * a.sf + 1.0, 1.0 - a.sf, 1.0 + a.sf);
        s0 = s0 * f; s1 = s1 * f;
        s_f32 = false;
        r = dr[4] <= 0.6 ? fpd_clipd(dr[3] * a.rf, -a.rf * 2.0, a.rf * 2.0) : 0.0;
        if (a.flip && dr[5] <= 0.5) {
            flip = 1;
            c0 = c_f32 ? (double)(((float)width - (float)c0) - 1.0f) : (width - c0) - 1.0;
        }
    }
    o.c[0] = c0; o.c[1] = c1; o.s[0] = s0; o.s[1] = s1; o.r = r; o.flip = flip;
    // get_affine_transform(c, s, r, image_size)
    const double src_w = s_f32 ? (double)((float)s0 * 200.0f) : s0 * 200.0;
    const double rad = 3.141592653589793 * r / 180.0;
    const double sn = sin(rad), cs = cos(rad);
    const double up = src_w * -0.5;
    const double d0 = 0.0 * cs - up * sn, d1 = 0.0 * sn + up * cs;                // get_dir([0, src_w * -0.5], rot_rad)
    const double dw = (double)a.out_w, dh = (double)a.out_h;
    float p[3][2], q[3][2];
    p[0][0] = (float)c0; p[0][1] = (float)c1;
    p[1][0] = (float)(c0 + d0); p[1][1] = (float)(c1 + d1);
    q[0][0] = (float)(dw * 0.5); q[0][1] = (float)(dh * 0.5);
    q[1][0] = (float)(dw * 0.5 + 0.0); q[1][1] = (float)(dh * 0.5 + (double)(float)(dw * -0.5));
    for (int k = 0; k < 2; ++k) {                                                   // get_3rd_point, float32
        float (*v)[2] = k ? q : p;
        const float e0 = v[0][0] - v[1][0], e1 = v[0][1] - v[1][1];
        v[2][0] = v[1][0] + -e1;
        v[2][1] = v[1][1] + e0;
    }
    // cv2.getAffineTransform: the map taking p[i] to q[i], float64, solved about p[0] (differences of float32 values are
    // exact in float64)
    const double u1x = (double)p[1][0] - p[0][0], u1y = (double)p[1][1] - p[0][1];
    const double u2x = (double)p[2][0] - p[0][0], u2y = (double)p[2][1] - p[0][1];
    const double det = u1x * u2y - u2x * u1y;
    double* m = o.trans;
    for (int k = 0; k < 2; ++k) {
        const double v1 = (double)q[1][k] - q[0][k], v2 = (double)q[2][k] - q[0][k];
        const double ma = (v1 * u2y - v2 * u1y) / det, mb = (u1x * v2 - u2x * v1) / det;
        m[3 * k] = ma; m[3 * k + 1] = mb;
        m[3 * k + 2] = (double)q[0][k] - ma * (double)p[0][0] - mb * (double)p[0][1];
    }
    // cv::invertAffineTransform (lib/utils/transforms.py invert_affine)
    const double dd = m[0] * m[4] - m[1] * m[3];
    const double d = dd != 0.0 ? 1.0 / dd : 0.0;
    const double a11 = m[4] * d, a22 = m[0] * d, a12 = -m[1] * d, a21 = -m[3] * d;
    o.minv[0] = a11; o.minv[1] = a12; o.minv[2] = -a11 * m[2] - a12 * m[5];
    o.minv[3] = a21; o.minv[4] = a22; o.minv[5] = -a21 * m[2] - a22 * m[5];
}
