// Inference post-processing of the validate / flip-test path on the device
// (/root/reference/lib/core/function.py:189-332 `validate`; the reference round-trips every tensor through numpy):
//   flip_w_kernel       input[:, :, :, ::-1]                                     (function.py:217-221: np.flip(input, 3))
//   flip_merge_kernel   flip_back (utils/transforms.py:15-29: reverse the width axis, swap the left/right joint
//                       channels) + the one-pixel shift of the flipped map (function.py:233-236, TEST.SHIFT_HEATMAP)
//                       + the average (output + output_flipped) * 0.5 (function.py:238), one pass
//   final_preds_kernel  get_final_preds (core/inference.py:49-79): heat-map arg-max (first maximum wins, coordinates
//                       zeroed where the maximum is not positive), the quarter-pixel shift towards the higher neighbour
//                       (TEST.POST_PROCESS) and the affine map back to image coordinates (transform_preds,
//                       utils/transforms.py:50-55: float64 [x, y, 1] . trans^T, result stored as float32)
//   val_post_kernel    one validation batch in one launch (fpd_val_post_t): the NHWC maps of the arena in, the merged NHWC
//                       fp32 map, the batch's rows of all_preds and all_boxes out; the per-sample inverse affine map is
//                       computed on the device (val_post_math.h, the text a host build checks against numpy)
// All of them are index / byte work or exact fp32 arithmetic in the reference's own operation order: results are
// bit-identical to the reference functions (tests/golden/infer_ref.npz).
#include "argmax.h"
#include "common.h"
#include "map_coords.h"
#include "val_post_math.h"

namespace {

// get_max_preds' zeroing + get_final_preds' quarter-pixel shift (inference.py:18-46,57-70) for the arg-max m of one map;
// at(y, x) reads the map
template <typename At>
__device__ __forceinline__ void peak_coords(ArgMax m, int H, int W, int post_process, At at, float& cx, float& cy) {
    cx = m.v > 0.f ? (float)(m.i % W) : 0.f;
    cy = m.v > 0.f ? (float)(m.i / W) : 0.f;
    if (post_process) {
        const int px = (int)floorf(cx + 0.5f), py = (int)floorf(cy + 0.5f);
        if (1 < px && px < W - 1 && 1 < py && py < H - 1) {
            const float dx = at(py, px + 1) - at(py, px - 1);
            const float dy = at(py + 1, px) - at(py - 1, px);
            cx += (dx > 0.f ? 0.25f : (dx < 0.f ? -0.25f : 0.f));
            cy += (dy > 0.f ? 0.25f : (dy < 0.f ? -0.25f : 0.f));
        }
    }
}

__global__ __launch_bounds__(256) void flip_w_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t rows, int W) {
    const int64_t total = rows * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / W;
        const int c = (int)(i - r * W);
        y[i] = x[r * W + (W - 1 - c)];
    }
}

// a, b: [N,J,H,W] fp32 (the module API's outputs for the image and for the flipped image); src[j] = channel of b that
// lands in channel j after flip_back's sequential pair swaps.
__global__ __launch_bounds__(256) void flip_merge_kernel(const fpd_flipmerge_t p) {
    const int64_t total = (int64_t)p.N * p.J * p.H * p.W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % p.W);
        const int64_t row = i / p.W;                         // (n*J + j)*H + y
        const int y = (int)(row % p.H);
        const int64_t nj = row / p.H;
        const int j = (int)(nj % p.J);
        const int64_t n = nj / p.J;
        // flipped-back column x holds b's column W-1-x; the shift copies column x-1 into x for x >= 1 (column 0 stays)
        const int xs = (p.shift && x >= 1) ? x - 1 : x;
        const float f = p.b[((n * p.J + p.src[j]) * p.H + y) * p.W + (p.W - 1 - xs)];
        p.y[i] = p.a != nullptr ? (p.a[i] + f) * 0.5f : f;      // a == NULL: flip_back (+ shift) only
    }
}

__global__ __launch_bounds__(256) void final_preds_kernel(const fpd_finalpreds_t p) {
    __shared__ ArgMax s[4];
    const int n = blockIdx.x / p.J;
    const int HW = p.H * p.W;
    const float* hm = p.hm + (size_t)blockIdx.x * HW;
    ArgMax m = {-3.4e38f, 0x7fffffff};
    for (int q = threadIdx.x; q < HW; q += blockDim.x) {
        ArgMax t = {hm[q], q};
        m = better(m, t);
    }
    m = block_argmax(m, s);
    if (threadIdx.x != 0) return;
    float cx, cy;
    peak_coords(m, p.H, p.W, p.post_process, [&](int y, int x) { return hm[y * p.W + x]; }, cx, cy);
    p.coords[2 * blockIdx.x] = cx;
    p.coords[2 * blockIdx.x + 1] = cy;
    p.maxvals[blockIdx.x] = m.v;
    if (p.trans != nullptr && p.preds != nullptr)
        map_coords(p.trans + 6 * n, cx, cy, p.preds[2 * blockIdx.x], p.preds[2 * blockIdx.x + 1]);
}

// merged[n,y,x,j] of fpd_val_post_t from the NHWC maps: a widened, or (a + f') * 0.5f with flip_merge_kernel's f'
template <typename T>
__device__ __forceinline__ float val_merged_at(const fpd_val_post_t& p, int64_t n, int y, int x, int j, int sj) {
    const int64_t row = (n * p.H + y) * p.W;
    const float va = DT<T>::ld((const T*)p.a + (row + x) * p.J + j);
    if (p.b == nullptr) return va;
    const int xs = (p.shift && x >= 1) ? x - 1 : x;
    const float f = DT<T>::ld((const T*)p.b + (row + (p.W - 1 - xs)) * p.J + sj);
    return (va + f) * 0.5f;
}

// One block per (sample, joint), like final_preds_kernel.  A block's loads and stores are J elements apart; the J blocks of
// a sample run side by side and share every line, and the two maps of a batch (N*H*W*J elements, 8 MiB in fp32 at
// 32x64x64x16) stay in L2.  Thread 0 re-forms the four neighbours of the peak from a and b instead of reading `merged`
// back: the same fp32 expression, no ordering between the block's own stores and loads needed.
template <typename T>
__global__ __launch_bounds__(256) void val_post_kernel(const fpd_val_post_t p) {
    __shared__ ArgMax s[4];
    const int64_t n = blockIdx.x / p.J;
    const int j = blockIdx.x % p.J;
    const int sj = p.b != nullptr ? p.src[j] : j;
    const int HW = p.H * p.W;
    ArgMax m = {-3.4e38f, 0x7fffffff};
    for (int q = threadIdx.x; q < HW; q += blockDim.x) {
        const int y = q / p.W;
        ArgMax t = {val_merged_at<T>(p, n, y, q - y * p.W, j, sj), q};
        p.merged[(n * HW + q) * p.J + j] = t.v;
        m = better(m, t);
    }
    m = block_argmax(m, s);
    if (threadIdx.x != 0) return;
    float cx, cy;
    peak_coords(m, p.H, p.W, p.post_process, [&](int y, int x) { return val_merged_at<T>(p, n, y, x, j, sj); }, cx, cy);
    const double c0 = p.center[2 * n], c1 = p.center[2 * n + 1], s0 = p.scale[2 * n], s1 = p.scale[2 * n + 1];
    double t[6];
    fpd_val_inverse_affine(c0, c1, s0, p.box_f32, p.W, p.H, t);
    float* o = p.all_preds + ((p.row0 + n) * p.J + j) * 3;
    map_coords(t, cx, cy, o[0], o[1]);
    o[2] = m.v;
    if (j == 0) {
        double* bx = p.all_boxes + (p.row0 + n) * 6;
        bx[0] = c0; bx[1] = c1; bx[2] = s0; bx[3] = s1;
        bx[4] = fpd_val_box_area(s0, s1, p.box_f32);
        bx[5] = p.score[n];
    }
}

}  // namespace

int fpd_flip_w_launch(const float* x, float* y, int64_t rows, int W, hipStream_t st) {
    const int64_t total = rows * W;
    const int blocks = (int)std::min<int64_t>(cdiv64(total, 256), 4096);
    FPD_LAUNCH(flip_w_kernel, dim3(blocks), dim3(256), 0, st, x, y, rows, W);
    return 0;
}

int fpd_flip_merge_launch(const fpd_flipmerge_t& p, hipStream_t st) {
    const int64_t total = (int64_t)p.N * p.J * p.H * p.W;
    const int blocks = (int)std::min<int64_t>(cdiv64(total, 256), 4096);
    FPD_LAUNCH(flip_merge_kernel, dim3(blocks), dim3(256), 0, st, p);
    return 0;
}

int fpd_final_preds_launch(const fpd_finalpreds_t& p, hipStream_t st) {
    FPD_LAUNCH(final_preds_kernel, dim3(p.N * p.J), dim3(256), 0, st, p);
    return 0;
}

int fpd_val_post_launch(const fpd_val_post_t& p, hipStream_t st) {
    if (p.dtype == FPD_BF16) FPD_LAUNCH(val_post_kernel<bf16_t>, dim3(p.N * p.J), dim3(256), 0, st, p);
    else FPD_LAUNCH(val_post_kernel<float>, dim3(p.N * p.J), dim3(256), 0, st, p);
    return 0;
}
