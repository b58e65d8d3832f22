// Distribution-aware coordinate decoding (DARK, Zhang et al., CVPR 2020) of the validation path in one launch
// (fpd_dark_t): per (sample, joint) the arg-max of the raw map, a separable Gaussian blur with zeros outside the map, the
// rescaled log map at the 13 positions around the peak, one Newton step in float64 (dark_math.h, the text a host build
// checks against numpy) and the map to image coordinates (map_coords.h; the matrix from the caller, or from
// val_post_math.h on the device for the fused validation step).
//
// One block per (sample, joint), like final_preds_kernel and val_post_kernel.  With the NHWC `merged` map a block's loads
// are J elements apart; the J blocks of a sample run side by side and share every line (infer.hip says why that is fine).
// The map is read ONCE, into LDS; the row pass goes from that image to a second one and the column pass back, so two fp32
// images of H*W are all the LDS the blur needs: 128 KB at the 128x128 limit, of the 160 KB a gfx950 CU has.  In both
// passes a lane works on consecutive x, so the lanes of a wave read consecutive LDS words for every tap: no bank conflicts.
// The taps stay float64 and so do the sums (a v_fma_f64 per tap on a part whose fp64 vector rate equals its unpacked fp32
// rate); each image is rounded to fp32 once when it is stored.  A peak that fails the interior guard, or a map without a
// positive maximum, is not refined whatever the blur gives, so its block skips the blur (a block-uniform branch).
// (A block of 1024 threads, a lane per pixel, was measured at 32x16x64x64: 32.7 us against 32.0, no gain; 256 it stays.)
#include "argmax.h"
#include "common.h"
#include "conv_dispatch.h"
#include "dark_math.h"
#include "map_coords.h"
#include "val_post_math.h"

namespace {

__device__ __forceinline__ float block_max(float v, float* s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = s[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = fmaxf(r, s[w]);
    return r;
}

__global__ __launch_bounds__(256) void dark_kernel(const fpd_dark_t p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ ArgMax s_am[4];
    __shared__ float s_mx[4];
    __shared__ double s_t[FPD_DARK_MAX_KSIZE];
    __shared__ double s_l[FPD_DARK_POINTS];
    const int H = p.H, W = p.W, HW = H * W, k = p.ksize, r = k >> 1;
    float* A = reinterpret_cast<float*>(smem);       // the map, later the blurred map
    float* T = A + HW;                                // the row pass
    const int n = blockIdx.x / p.J, j = blockIdx.x % p.J;
    const bool nhwc = p.layout == FPD_DARK_NHWC;
    const float* hm = p.hm + (nhwc ? (size_t)n * HW * p.J + j : (size_t)blockIdx.x * HW);
    const size_t stride = nhwc ? (size_t)p.J : 1;
    if ((int)threadIdx.x < k) s_t[threadIdx.x] = p.taps[threadIdx.x];
    ArgMax m = {-3.4e38f, 0x7fffffff};
    for (int q = threadIdx.x; q < HW; q += blockDim.x) {
        ArgMax t = {hm[q * stride], q};
        A[q] = t.v;
        m = better(m, t);
    }
    m = block_argmax(m, s_am);                        // (its barriers also publish A and s_t)
    float cx = m.v > 0.f ? (float)(m.i % W) : 0.f;
    float cy = m.v > 0.f ? (float)(m.i / W) : 0.f;
    const int px = (int)cx, py = (int)cy;
    int refined = 0;
    if (m.v > 0.f && fpd_dark_interior(px, py, W, H)) {        // the same for every thread of the block
        for (int q = threadIdx.x; q < HW; q += blockDim.x) {
            const int y = q / W, x = q - y * W;
            const int d0 = max(0, r - x), d1 = min(k, W + r - x);
            const int at = q - r;                     // tap d reads column x - r + d of this row
            double acc = 0.0;
            for (int d = d0; d < d1; ++d) acc = fma(s_t[d], (double)A[at + d], acc);
            T[q] = (float)acc;
        }
        __syncthreads();
        float bmax = -3.4e38f;
        for (int q = threadIdx.x; q < HW; q += blockDim.x) {
            const int y = q / W, x = q - y * W;
            const int d0 = max(0, r - y), d1 = min(k, H + r - y);
            const int at = q - r * W;                 // tap d reads row y - r + d of this column
            double acc = 0.0;
            for (int d = d0; d < d1; ++d) acc = fma(s_t[d], (double)T[at + d * W], acc);
            const float b = (float)acc;
            A[q] = b;
            bmax = fmaxf(bmax, b);
        }
        const float bm = block_max(bmax, s_mx);       // (its barrier also publishes the blurred A)
        if (bm > 0.f) {
            if (threadIdx.x < FPD_DARK_POINTS) {
                int ox, oy;
                fpd_dark_tap(threadIdx.x, &ox, &oy);
                const double v = (double)A[(py + oy) * W + (px + ox)] * ((double)m.v / (double)bm);
                s_l[threadIdx.x] = log(fmax(v, 1e-10));
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                double ox, oy;
                refined = fpd_dark_step(s_l, &ox, &oy);
                if (refined) {
                    cx = fpd_dark_apply(cx, ox);
                    cy = fpd_dark_apply(cy, oy);
                }
            }
        }
    }
    if (threadIdx.x != 0) return;
    if (p.coords != nullptr) {
        p.coords[2 * blockIdx.x] = cx;
        p.coords[2 * blockIdx.x + 1] = cy;
    }
    if (p.maxvals != nullptr) p.maxvals[blockIdx.x] = m.v;
    if (p.refined != nullptr) p.refined[blockIdx.x] = refined;
    if (p.preds != nullptr) {
        map_coords(p.trans + 6 * n, cx, cy, p.preds[2 * blockIdx.x], p.preds[2 * blockIdx.x + 1]);
    } else if (p.all_preds != nullptr) {
        double t[6];
        fpd_val_inverse_affine(p.center[2 * n], p.center[2 * n + 1], p.scale[2 * n], p.box_f32, W, H, t);
        float* o = p.all_preds + ((p.row0 + n) * p.J + j) * 3;
        map_coords(t, cx, cy, o[0], o[1]);
    }
}

}  // namespace

int fpd_dark_launch(const fpd_dark_t& p, hipStream_t st) {
    const size_t lds = (size_t)2 * p.H * p.W * sizeof(float);
    static LdsAttr configured;        // per device, raised once per size (thread-safe: common.h)
    if (lds > 65536)
        if (int rc_ = configured.ensure(reinterpret_cast<const void*>(&dark_kernel), lds)) return rc_;
    FPD_LAUNCH(dark_kernel, dim3(p.N * p.J), dim3(256), lds, st, p);
    return 0;
}
