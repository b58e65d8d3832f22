// Device data pipeline of the training loop (/root/reference/lib/dataset/JointsDataset.py:113-198 __getitem__ and :233-289
// generate_target): what the reference does per sample in DataLoader workers (cv2 + numpy) as two batch kernels, so that a
// loader only has to hand over decoded 8-bit images, the augmentation parameters it drew and the joint annotations.
//   render_targets_kernel  generate_target: integer placement of the Gaussian patch (bit-exact index work; the patch values
//                          come from the caller, computed with the reference's float32 numpy expression)
//   warp_affine_kernel     cv2.warpAffine(INTER_LINEAR, zero border) in OpenCV's fixed-point arithmetic -> ToTensor ->
//                          Normalize, written straight into the NCHW fp32 batch the stem kernel reads
//   augment_params_kernel  the random augmentation of __getitem__ (:137-179: half-body, scale / rotation jitter, flip,
//                          get_affine_transform, joint transform) from a device-resident database and a table of draws;
//                          its output drives warp_affine_aug_kernel and render_targets_kernel, so a batch needs three
//                          launches and no host work per sample
//   render_targets_unbiased_kernel  DARK's unbiased encoding (include/fpd_amd.h fpd_targets_unbiased_t): the Gaussian at the
//                          real-valued centre over the whole map, float64 values rounded once; the third launch of a batch
//                          when MODEL.TARGET_TYPE is gaussian_unbiased
#include <algorithm>

#include "augment_math.h"
#include "common.h"
#include "encode_math.h"

namespace {

// numpy's int(): truncation toward zero of a float64
__device__ __forceinline__ int trunc_i(double v) { return (int)v; }

// jw: joints_weight [J] (JointsDataset.py:286-287) or null
__device__ __forceinline__ void render_targets_body(const fpd_targets_t& a, const float* jw) {
    const int bj = blockIdx.x;
    const double* jt = a.joints + (size_t)bj * 3;
    float* tg = a.target + (size_t)bj * a.H * a.W;
    const int tmp = (a.patch - 1) / 2;                                  // sigma * 3
    // JointsDataset.py:254-255 (float64 division and sum, then int())
    const int mu_x = trunc_i(__dadd_rn(__ddiv_rn(jt[0], a.stride_x), 0.5));
    const int mu_y = trunc_i(__dadd_rn(__ddiv_rn(jt[1], a.stride_y), 0.5));
    const int ulx = mu_x - tmp, uly = mu_y - tmp, brx = mu_x + tmp + 1, bry = mu_y + tmp + 1;
    float w = a.vis[bj];
    const bool outside = ulx >= a.W || uly >= a.H || brx < 0 || bry < 0;
    if (outside) w = 0.f;                                              // :259-263
    if (threadIdx.x == 0) a.weight[bj] = jw ? __fmul_rn(w, jw[bj % a.J]) : w;
    const bool paste = !outside && w > 0.5f;                           // :279-282
    const int x0 = max(0, ulx), x1 = min(brx, a.W), y0 = max(0, uly), y1 = min(bry, a.H);
    for (int p = threadIdx.x; p < a.H * a.W; p += blockDim.x) {
        const int y = p / a.W, x = p - y * a.W;
        float v = 0.f;
        if (paste && x >= x0 && x < x1 && y >= y0 && y < y1) v = a.g[(y - uly) * a.patch + (x - ulx)];
        tg[p] = v;
    }
}

__global__ __launch_bounds__(256) void render_targets_kernel(const fpd_targets_t a) { render_targets_body(a, nullptr); }
__global__ __launch_bounds__(256) void render_targets_w_kernel(const fpd_targets_w_t a) { render_targets_body(a.t, a.joints_weight); }

// One workgroup per (sample, joint).  The decisions come from encode_math.h; the value of pixel (x, y) is the float64 product
// of a column factor ex[x] and a row factor ey[y] (W + H exponentials per map instead of H * W), both in LDS: s_factor holds
// ex[0..W) then ey[0..H).  Rows whose length is a multiple of four are written 16 bytes at a time when the buffer allows it.
__global__ __launch_bounds__(256) void render_targets_unbiased_kernel(const fpd_targets_unbiased_t a) {
    extern __shared__ double s_factor[];
    const int bj = blockIdx.x, HW = a.H * a.W;
    const double* jt = a.joints + (size_t)bj * 3;
    float* tg = a.target + (size_t)bj * HW;
    const bool has_jw = a.joints_weight != nullptr;
    fpd_encode_place_t pl;
    fpd_encode_place(jt[0], jt[1], a.stride_x, a.stride_y, a.sigma, a.W, a.H, a.vis[bj], has_jw, has_jw ? a.joints_weight[bj % a.J] : 0.f, &pl);
    if (threadIdx.x == 0) a.weight[bj] = pl.weight;
    const bool wide = (a.W & 3) == 0 && ((uintptr_t)a.target & 15) == 0;      // then every map starts on 16 bytes as well
    if (!pl.drawn) {                                                        // the same for the whole block
        if (wide) {
            for (int q = threadIdx.x; q < HW / 4; q += blockDim.x) reinterpret_cast<float4*>(tg)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int p = threadIdx.x; p < HW; p += blockDim.x) tg[p] = 0.f;
        }
        return;
    }
    double* ex = s_factor;
    double* ey = s_factor + a.W;
    for (int i = threadIdx.x; i < a.W + a.H; i += blockDim.x)
        s_factor[i] = i < a.W ? fpd_encode_factor(i, pl.mu_x, a.sigma) : fpd_encode_factor(i - a.W, pl.mu_y, a.sigma);
    __syncthreads();
    if (wide) {
        for (int q = threadIdx.x; q < HW / 4; q += blockDim.x) {
            const int p = 4 * q, y = p / a.W, x = p - y * a.W;               // W % 4 == 0: the four pixels share the row
            const double r = ey[y];
            reinterpret_cast<float4*>(tg)[q] = make_float4(fpd_encode_value(ex[x], r), fpd_encode_value(ex[x + 1], r),
                                                           fpd_encode_value(ex[x + 2], r), fpd_encode_value(ex[x + 3], r));
        }
    } else {
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            const int y = p / a.W, x = p - y * a.W;
            tg[p] = fpd_encode_value(ex[x], ey[y]);
        }
    }
}

// cv::saturate_cast<int>(double) = cvRound = round half to even
__device__ __forceinline__ int cv_round(double v) { return __double2int_rn(v); }
__device__ __forceinline__ int sat_short(int v) { return min(max(v, -32768), 32767); }

// One thread per destination pixel, three channels.  OpenCV (imgwarp.cpp WarpAffineInvoker + remapBilinear, 8-bit):
//   AB_BITS 10, INTER_BITS 5, round_delta = 1024/32/2 = 16
//   X = (cvRound((m1*y + m2)*1024) + 16 + cvRound(m0*x*1024)) >> 5     (1/32-pixel source coordinate), Y likewise
//   sx = X >> 5, fx = X & 31; weights (32-fx)(32-fy)*32 ... as shorts (32768 saturates to 32767), sum of the four
//   products + 2^14 >> 15, saturated to 8 bit; taps outside the image contribute the border value 0.
// flip: tap column X reads source column w-1-X -- the warp of the mirrored image (data_numpy[:, ::-1, :], :162), not a
// matrix with the mirror composed in, whose fixed-point terms would round differently
struct warp_src {
    const uint8_t* img;
    int h, w;
    int64_t row_bytes;
    double minv[6];
    bool flip;
};

template <typename A>
__device__ __forceinline__ void warp_affine_body(const A& a, const warp_src& s) {
    const int b = blockIdx.y;
    const int HW = a.H * a.W;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
        const int y = p / a.W, x = p - y * a.W;
        const int X0 = cv_round(__dmul_rn(__dadd_rn(__dmul_rn(s.minv[1], (double)y), s.minv[2]), 1024.0)) + 16;
        const int Y0 = cv_round(__dmul_rn(__dadd_rn(__dmul_rn(s.minv[4], (double)y), s.minv[5]), 1024.0)) + 16;
        const int ad = cv_round(__dmul_rn(__dmul_rn(s.minv[0], (double)x), 1024.0));
        const int bd = cv_round(__dmul_rn(__dmul_rn(s.minv[3], (double)x), 1024.0));
        const int X = (X0 + ad) >> 5, Y = (Y0 + bd) >> 5;
        const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
        const int fx = X & 31, fy = Y & 31;
        int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
        if (w00 > 32767) w00 = 32767;                                   // saturate_cast<short>; fx = fy = 0: the result is
                                                                        // the source pixel either way
        const bool in_x0 = (unsigned)sx < (unsigned)s.w, in_x1 = (unsigned)(sx + 1) < (unsigned)s.w;
        const bool in_y0 = (unsigned)sy < (unsigned)s.h, in_y1 = (unsigned)(sy + 1) < (unsigned)s.h;
        const uint8_t* r0 = s.img + (int64_t)sy * s.row_bytes;
        const uint8_t* r1 = r0 + s.row_bytes;
        const int c0 = s.flip ? s.w - 1 - sx : sx, c1 = s.flip ? s.w - 2 - sx : sx + 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int p00 = (in_y0 && in_x0) ? r0[3 * c0 + c] : 0;
            const int p01 = (in_y0 && in_x1) ? r0[3 * c1 + c] : 0;
            const int p10 = (in_y1 && in_x0) ? r1[3 * c0 + c] : 0;
            const int p11 = (in_y1 && in_x1) ? r1[3 * c1 + c] : 0;
            int v = (p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + (1 << 14)) >> 15;
            v = min(max(v, 0), 255);
            // ToTensor: uint8 -> float32 / 255; Normalize: (t - mean) / std  (torch fp32 ops, in this order)
            const float t = __fdiv_rn((float)v, 255.f);
            a.out[((size_t)b * 3 + c) * HW + p] = __fdiv_rn(__fsub_rn(t, a.mean[c]), a.std[c]);
        }
    }
}

__global__ __launch_bounds__(256) void warp_affine_kernel(const fpd_warp_t a) {
    const fpd_warp_src_t t = a.src[blockIdx.y];
    warp_src s = {t.img, t.h, t.w, t.row_bytes, {t.minv[0], t.minv[1], t.minv[2], t.minv[3], t.minv[4], t.minv[5]}, false};
    warp_affine_body(a, s);
}

__global__ __launch_bounds__(256) void warp_affine_aug_kernel(const fpd_warp_aug_t a) {
    const fpd_aug_crop_t t = a.crop[blockIdx.y];
    warp_src s = {nullptr, 0, 0, 0, {t.minv[0], t.minv[1], t.minv[2], t.minv[3], t.minv[4], t.minv[5]}, t.flip != 0};
    if ((unsigned)t.src < (unsigned)a.N) {             // an index outside the table reads nothing: every tap is border
        const fpd_aug_img_t im = a.images[t.src];
        s.img = im.img; s.h = im.h; s.w = im.w; s.row_bytes = im.row_bytes;
    }
    warp_affine_body(a, s);
}

// One 64-thread block per sample: thread 0 does the scalar work (augment_math.h), then one thread per joint applies the
// flip's exchange and the affine map (fliplr_joints transforms.py:32-47, JointsDataset.py:177-179).
__global__ __launch_bounds__(64) void augment_params_kernel(const fpd_augment_t a) {
#pragma clang fp contract(off)
    __shared__ fpd_aug_sample_t o;
    const int b = blockIdx.x, J = a.db.J;
    int i = a.idx[(size_t)b * a.idx_stride];
    const bool known = (unsigned)i < (unsigned)a.db.N;
    if (!known) i = 0;
    if (threadIdx.x == 0) {
        fpd_augment_sample(a, b, i, o);
        fpd_aug_crop_t cr;
        cr.src = known ? i : -1;
        cr.flip = o.flip;
        for (int k = 0; k < 6; ++k) { cr.minv[k] = o.minv[k]; a.trans[(size_t)b * 6 + k] = o.trans[k]; }
        a.crop[b] = cr;
        a.center[2 * b] = o.c[0]; a.center[2 * b + 1] = o.c[1];
        a.scale[2 * b] = o.s[0]; a.scale[2 * b + 1] = o.s[1];
        a.rotation[b] = o.r;
        a.flipped[b] = o.flip;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < J; j += blockDim.x) {
        const int k = o.flip ? a.db.flip_src[j] : j;
        const float v = a.db.vis[(size_t)i * J + k];
        double x = a.db.joints[((size_t)i * J + k) * 3], y = a.db.joints[((size_t)i * J + k) * 3 + 1];
        if (o.flip) {
            x = ((double)a.db.images[i].w - x - 1.0) * (double)v;
            y = y * (double)v;
        }
        if (v > 0.f) {
            const double nx = o.trans[0] * x + o.trans[1] * y + o.trans[2];
            const double ny = o.trans[3] * x + o.trans[4] * y + o.trans[5];
            x = nx; y = ny;
        }
        double* out = a.joints + ((size_t)b * J + j) * 3;
        out[0] = x; out[1] = y; out[2] = 0.0;
        a.vis[(size_t)b * J + j] = v;
    }
}

}  // namespace

int fpd_render_targets_w_launch(const fpd_targets_w_t& a, hipStream_t st) {
    FPD_LAUNCH(render_targets_w_kernel, dim3(a.t.B * a.t.J), dim3(256), 0, st, a);
    return 0;
}

// api.hip has checked (H + W) * 8 bytes against the LDS a kernel gets without asking
int fpd_render_targets_unbiased_launch(const fpd_targets_unbiased_t& a, hipStream_t st) {
    FPD_LAUNCH(render_targets_unbiased_kernel, dim3(a.B * a.J), dim3(256), (size_t)(a.H + a.W) * sizeof(double), st, a);
    return 0;
}

int fpd_warp_affine_aug_launch(const fpd_warp_aug_t& a, hipStream_t st) {
    const int bx = std::min(cdiv(a.H * a.W, 256), 256);
    FPD_LAUNCH(warp_affine_aug_kernel, dim3(bx, a.B), dim3(256), 0, st, a);
    return 0;
}

int fpd_augment_params_launch(const fpd_augment_t& a, hipStream_t st) {
    FPD_LAUNCH(augment_params_kernel, dim3(a.B), dim3(64), 0, st, a);
    return 0;
}

int fpd_render_targets_launch(const fpd_targets_t& a, hipStream_t st) {
    FPD_LAUNCH(render_targets_kernel, dim3(a.B * a.J), dim3(256), 0, st, a);
    return 0;
}

int fpd_warp_affine_launch(const fpd_warp_t& a, hipStream_t st) {
    const int bx = std::min(cdiv(a.H * a.W, 256), 256);
    FPD_LAUNCH(warp_affine_kernel, dim3(bx, a.B), dim3(256), 0, st, a);
    return 0;
}
