// Debug images of the train / validate loops on the device (the reference's lib/utils/vis.py renders them on the host with
// torchvision.utils.make_grid, cv2.resize, cv2.applyColorMap, cv2.circle and numpy after downloading the batch):
//   vis_minmax_kernel        min / max of the input batch, once per iteration, shared by every canvas
//   vis_max_preds_kernel     get_max_preds of a heat map in any of its three forms (one block per map, argmax.h)
//   vis_grid_kernel          make_grid(normalize=True) as bytes, one thread per canvas pixel
//   vis_joint_marks_kernel   the joint marks scattered over the composed canvas: one thread per (joint, pixel of its 7x7
//                            window); overlapping marks store the same three bytes, so no order is needed among them
//   vis_heatmap_kernel       save_batch_heatmaps: one thread per pixel of the resized image; it forms the resized pixel once
//                            and walks the J + 1 tiles of its row.  The cumulative drawing of the reference is a bit mask of
//                            the joints whose mark covers the pixel: the base of tile j+1 is marked iff a bit <= j is set.
// Per-pixel arithmetic: vis_math.h (the text a host build checks).  Every pixel depends on its own inputs only.
#include "argmax.h"
#include "common.h"
#include "vis_math.h"

#pragma clang fp contract(off)      // joint * coord_scale and the sums around it round like the host's: no fma

namespace {

// min: non-negative floats order like their bits as signed integers, negative ones in reverse as unsigned ones; max the other
// way round.  Integer atomics on the float's own word, so the result needs no decoding.
__device__ __forceinline__ void atomic_min_f32(float* p, float v) {
    if (v >= 0.f) atomicMin(reinterpret_cast<int*>(p), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned*>(p), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f32(float* p, float v) {
    if (v >= 0.f) atomicMax(reinterpret_cast<int*>(p), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned*>(p), __float_as_uint(v));
}

__global__ void vis_minmax_init_kernel(float* out) {
    out[0] = __int_as_float(0x7f800000);
    out[1] = __int_as_float((int)0xff800000u);
}

__global__ __launch_bounds__(256) void vis_minmax_kernel(const float* __restrict__ x, int64_t n, float* out) {
    __shared__ float s_lo[4], s_hi[4];
    float lo = __int_as_float(0x7f800000), hi = -lo;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = x[i] + 0.f;                        // -0 -> +0: one encoding of zero for the integer order
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); }
    atomic_min_f32(out, lo);
    atomic_max_f32(out + 1, hi);
}

// element (n, j, y, x) of a heat map [N,J,h,w] (NCHW) or [N,h,w,J] (NHWC)
template <typename T>
__device__ __forceinline__ float hm_at(const void* hm, int layout, int J, int h, int w, int64_t n, int j, int y, int x) {
    const int64_t i = layout == FPD_VIS_NHWC ? ((n * h + y) * w + x) * J + j : ((n * J + j) * h + y) * w + x;
    return DT<T>::ld((const T*)hm + i);
}

template <typename T>
__global__ __launch_bounds__(256) void vis_max_preds_kernel(const fpd_vis_max_preds_t p) {
    __shared__ ArgMax s[4];
    const int64_t n = blockIdx.x / p.J;
    const int j = blockIdx.x % p.J;
    const int hw = p.h * p.w;
    ArgMax m = {-3.4e38f, 0x7fffffff};
    for (int q = threadIdx.x; q < hw; q += blockDim.x) {
        const int y = q / p.w;
        ArgMax t = {hm_at<T>(p.hm, p.layout, p.J, p.h, p.w, n, j, y, q - y * p.w), q};
        m = better(m, t);
    }
    m = block_argmax(m, s);
    if (threadIdx.x != 0) return;
    const bool pos = m.v > 0.f;
    p.preds[2 * (int64_t)blockIdx.x] = pos ? (float)(m.i % p.w) : 0.f;
    p.preds[2 * (int64_t)blockIdx.x + 1] = pos ? (float)(m.i / p.w) : 0.f;
    p.maxvals[blockIdx.x] = m.v;
}

struct GridGeom { int xmaps, ymaps, GH, GW; };

__global__ __launch_bounds__(256) void vis_grid_kernel(const fpd_vis_joints_grid_t p, const GridGeom g) {
    const float neg_min = -p.minmax[0];
    const float d = fpd_vis_denom(p.minmax[0], p.minmax[1]);
    const int64_t total = (int64_t)g.GH * g.GW;
    const int64_t plane = (int64_t)p.H * p.W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int gy = (int)(i / g.GW), gx = (int)(i - (int64_t)gy * g.GW);
        int64_t k = -1;
        int y = gy, x = gx;
        if (p.N == 1) {
            k = 0;
        } else if (gy >= p.padding && gx >= p.padding) {
            const int r = (gy - p.padding) / (p.H + p.padding), c = (gx - p.padding) / (p.W + p.padding);
            y = (gy - p.padding) - r * (p.H + p.padding);
            x = (gx - p.padding) - c * (p.W + p.padding);
            if (y < p.H && x < p.W && r < g.ymaps && c < g.xmaps && (int64_t)r * g.xmaps + c < p.N) k = (int64_t)r * g.xmaps + c;
        }
        uint8_t b0 = 0, b1 = 0, b2 = 0;
        if (k >= 0) {
            const float* px = p.image + k * 3 * plane + (int64_t)y * p.W + x;
            b0 = fpd_vis_norm_byte(px[0], neg_min, d);
            b1 = fpd_vis_norm_byte(px[plane], neg_min, d);
            b2 = fpd_vis_norm_byte(px[2 * plane], neg_min, d);
        }
        uint8_t* o = p.canvas + 3 * i;
        o[0] = b0; o[1] = b1; o[2] = b2;
    }
}

__global__ __launch_bounds__(256) void vis_joint_marks_kernel(const fpd_vis_joints_grid_t p, const GridGeom g) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t q = t / 49;                                       // (sample, joint)
    if (q >= (int64_t)p.N * p.J) return;
    if (p.vis[q] == 0.f) return;
    const int o = (int)(t - q * 49);
    const int dy = o / 7 - 3, dx = o - (o / 7) * 7 - 3;
    if (!fpd_vis_in_ring(dx, dy)) return;
    const int k = (int)(q / p.J);
    double jx, jy;
    if (p.joints_f64) {
        const double* j = (const double*)p.joints + q * p.joints_stride;
        jx = j[0] * (double)p.coord_scale; jy = j[1] * (double)p.coord_scale;
    } else {
        const float* j = (const float*)p.joints + q * p.joints_stride;
        jx = (double)j[0] * (double)p.coord_scale; jy = (double)j[1] * (double)p.coord_scale;
    }
    const int cx = fpd_vis_mark_pos(k % g.xmaps, p.W, p.padding, jx) + dx;
    const int cy = fpd_vis_mark_pos(k / g.xmaps, p.H, p.padding, jy) + dy;
    if (cx < 0 || cx >= g.GW || cy < 0 || cy >= g.GH) return;
    uint8_t* px = p.canvas + 3 * ((int64_t)cy * g.GW + cx);
    px[0] = 255; px[1] = 0; px[2] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void vis_heatmap_kernel(const fpd_vis_heatmap_grid_t p) {
    const float neg_min = p.normalize ? -p.minmax[0] : -0.f;
    const float d = p.normalize ? fpd_vis_denom(p.minmax[0], p.minmax[1]) : 1.f;
    const int64_t total = (int64_t)p.N * p.h * p.w;
    const int64_t plane = (int64_t)p.H * p.W;
    const int64_t row_bytes = (int64_t)(p.J + 1) * p.w * 3;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int tx = (int)(i % p.w);
        const int64_t ny = i / p.w;                                 // n * h + ty: the canvas row
        const int ty = (int)(ny % p.h);
        const int64_t n = ny / p.h;
        uint8_t res[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* q = p.image + (n * 3 + c) * plane + (int64_t)(4 * ty + 1) * p.W + (4 * tx + 1);
            res[c] = fpd_vis_resize4(fpd_vis_norm_byte(q[0], neg_min, d), fpd_vis_norm_byte(q[1], neg_min, d),
                                     fpd_vis_norm_byte(q[p.W], neg_min, d), fpd_vis_norm_byte(q[p.W + 1], neg_min, d));
        }
        uint32_t marks = 0;                                         // bit k: the mark of joint k covers this pixel
        for (int k = 0; k < p.J; ++k) {
            const float* pr = p.preds + (n * p.J + k) * 2;
            if (fpd_vis_in_cross(tx - fpd_vis_trunc((double)pr[0]), ty - fpd_vis_trunc((double)pr[1]))) marks |= 1u << k;
        }
        uint8_t* o = p.canvas + ny * row_bytes + 3 * tx;
        if (marks) { o[0] = 0; o[1] = 0; o[2] = 255; }
        else { o[0] = res[0]; o[1] = res[1]; o[2] = res[2]; }
        for (int j = 0; j < p.J; ++j) {
            o += 3 * p.w;
            if ((marks >> j) & 1u) { o[0] = 0; o[1] = 0; o[2] = 255; continue; }
            const bool base_marked = (marks & ((2u << j) - 1u)) != 0;
            const uint8_t* col = p.table + 3 * (int)fpd_vis_heat_byte(hm_at<T>(p.hm, p.layout, p.J, p.h, p.w, n, j, ty, tx));
            o[0] = fpd_vis_blend(col[0], base_marked ? (uint8_t)0 : res[0]);
            o[1] = fpd_vis_blend(col[1], base_marked ? (uint8_t)0 : res[1]);
            o[2] = fpd_vis_blend(col[2], base_marked ? (uint8_t)255 : res[2]);
        }
    }
}

GridGeom grid_geom(const fpd_vis_joints_grid_t& p) {
    GridGeom g;
    g.xmaps = p.nrow < p.N ? p.nrow : p.N;
    g.ymaps = (p.N + g.xmaps - 1) / g.xmaps;
    g.GH = p.N == 1 ? p.H : (p.H + p.padding) * g.ymaps + p.padding;
    g.GW = p.N == 1 ? p.W : (p.W + p.padding) * g.xmaps + p.padding;
    return g;
}

}  // namespace

int64_t fpd_vis_joints_canvas_bytes(const fpd_vis_joints_grid_t& p) {
    const int xmaps = p.nrow < p.N ? p.nrow : p.N;
    const int64_t ymaps = (p.N + xmaps - 1) / xmaps;
    if (p.N == 1) return (int64_t)p.H * p.W * 3;
    return ((int64_t)(p.H + p.padding) * ymaps + p.padding) * ((int64_t)(p.W + p.padding) * xmaps + p.padding) * 3;
}

int fpd_vis_minmax_launch(const fpd_vis_minmax_t& p, hipStream_t st) {
    const int blocks = (int)std::min<int64_t>(cdiv64(p.n, 256 * 16), 1024);
    FPD_LAUNCH(vis_minmax_init_kernel, dim3(1), dim3(1), 0, st, p.out);
    FPD_LAUNCH(vis_minmax_kernel, dim3(blocks), dim3(256), 0, st, p.x, p.n, p.out);
    return 0;
}

int fpd_vis_max_preds_launch(const fpd_vis_max_preds_t& p, hipStream_t st) {
    if (p.dtype == FPD_BF16) FPD_LAUNCH(vis_max_preds_kernel<bf16_t>, dim3(p.N * p.J), dim3(256), 0, st, p);
    else FPD_LAUNCH(vis_max_preds_kernel<float>, dim3(p.N * p.J), dim3(256), 0, st, p);
    return 0;
}

int fpd_vis_joints_grid_launch(const fpd_vis_joints_grid_t& p, hipStream_t st) {
    const GridGeom g = grid_geom(p);
    const int blocks = (int)std::min<int64_t>(cdiv64((int64_t)g.GH * g.GW, 256), 8192);
    FPD_LAUNCH(vis_grid_kernel, dim3(blocks), dim3(256), 0, st, p, g);
    const int64_t marks = (int64_t)p.N * p.J * 49;
    if (marks > 0) FPD_LAUNCH(vis_joint_marks_kernel, dim3((unsigned)cdiv64(marks, 256)), dim3(256), 0, st, p, g);
    return 0;
}

int fpd_vis_heatmap_grid_launch(const fpd_vis_heatmap_grid_t& p, hipStream_t st) {
    const int blocks = (int)std::min<int64_t>(cdiv64((int64_t)p.N * p.h * p.w, 256), 8192);
    if (p.dtype == FPD_BF16) FPD_LAUNCH(vis_heatmap_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, p);
    else FPD_LAUNCH(vis_heatmap_kernel<float>, dim3(blocks), dim3(256), 0, st, p);
    return 0;
}
