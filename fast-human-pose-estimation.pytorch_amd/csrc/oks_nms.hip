// Rescoring + OKS NMS of COCO's evaluate (the reference's lib/dataset/coco.py:334-369 over lib/nms/nms.py:75-177): all
// pictures of a validation run in ONE launch, one workgroup per picture (grid-stride when the grid is capped), the greedy
// loop inside the workgroup.
//
// Per picture of P people (any P: nothing of size P lives in LDS or registers, every person's working score lives in the
// caller's `work` buffer and is only ever touched by the thread tid == d % 256):
//   pass 0   score[d] = mean of the maxvals above in_vis_thre (float32, summed in joint order) * box_score[d] (float64);
//            work[d] = score[d]; every thread keeps the best (value, index) of its people
//   loop     block arg-max of the thread bests (ties: lower index) -> pick g, appended to keep[];
//            g's keypoints -> LDS; every thread, for its still-present people d: oks(g, d) -- computed and consumed at
//            once -- hard: oks > thresh removes d;  soft: work[d] *= exp(-oks^2 / thresh), at most 20 picks;
//            the same sweep collects the thread bests of the next round.
// Three barriers per pick.  The arithmetic restates numpy's: dx, dy, dx*dx + dy*dy in float32 with separately rounded
// products (no contraction), everything after in float64 with the divisions in the reference's order.
#include "conv_dispatch.h"

#define OKS_THREADS 256
#define OKS_WAVES (OKS_THREADS / 64)
#define OKS_MAX_J 64
#define OKS_SOFT_MAX_DETS 20
#define OKS_NONE 0x7fffffff

// a candidate beats the incumbent: larger value, or the same value at a lower index
__device__ __forceinline__ bool oks_better(double v, int i, double bv, int bi) {
    return i != OKS_NONE && (bi == OKS_NONE || v > bv || (v == bv && i < bi));
}

__global__ __launch_bounds__(OKS_THREADS) void oks_nms_kernel(const fpd_oks_nms_t a) {
#pragma clang fp contract(off)
    __shared__ float s_gx[OKS_MAX_J], s_gy[OKS_MAX_J];
    __shared__ double s_var[OKS_MAX_J];
    __shared__ double s_val[OKS_WAVES];
    __shared__ int s_idx[OKS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int J = a.J;
    const double removed = -__builtin_huge_val();
    const float vis_thre = (float)a.in_vis_thre;
    const double eps = 2.220446049250313e-16;            // np.spacing(1)
    if (tid < J) {
        const double s2 = a.sigmas[tid] * 2.0;
        s_var[tid] = s2 * s2;
    }
    for (int img = blockIdx.x; img < a.n_img; img += gridDim.x) {
        const int base = a.offsets[img];
        const int P = a.offsets[img + 1] - base;
        if (base < 0 || P < 0 || (int64_t)base + P > (int64_t)a.P_total) {      // a bad offset table: touch nothing of it
            if (tid == 0) a.n_keep[img] = -1;
            continue;
        }
        // ---- pass 0: rescoring ----
        double bv = 0.0;
        int bi = OKS_NONE;
        for (int d = tid; d < P; d += OKS_THREADS) {
            const size_t p = (size_t)base + d;
            double s = a.box_score[p];
            if (a.rescore) {
                const float* k = a.kpts + p * (size_t)J * 3;
                float sum = 0.f;
                int cnt = 0;
                for (int j = 0; j < J; ++j) {
                    const float m = k[3 * j + 2];
                    if (m > vis_thre) { sum = sum + m; ++cnt; }
                }
                s = cnt ? (double)(sum / (float)cnt) * s : 0.0 * s;
            }
            a.score[p] = s;
            a.work[p] = s;
            if (s == s && s != removed && oks_better(s, d, bv, bi)) { bv = s; bi = d; }
        }
        const int max_picks = a.soft ? (P < OKS_SOFT_MAX_DETS ? P : OKS_SOFT_MAX_DETS) : P;
        int nk = 0;
        while (true) {
            // ---- block arg-max of the thread bests ----
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (oks_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            __syncthreads();                              // the previous round's readers of s_val / s_gx are done
            if (lane == 0) { s_val[wave] = bv; s_idx[wave] = bi; }
            __syncthreads();
            double gv = s_val[0];
            int g = s_idx[0];
#pragma unroll
            for (int w = 1; w < OKS_WAVES; ++w)
                if (oks_better(s_val[w], s_idx[w], gv, g)) { gv = s_val[w]; g = s_idx[w]; }
            if (g == OKS_NONE || nk >= max_picks) break;  // (uniform: every thread reads the same four entries)
            if (tid == 0) a.keep[(size_t)base + nk] = g;
            const bool first = nk == 0;
            ++nk;
            if (tid < J) {
                const float* k = a.kpts + ((size_t)base + g) * (size_t)J * 3;
                s_gx[tid] = k[3 * tid];
                s_gy[tid] = k[3 * tid + 1];
            }
            __syncthreads();
            const double a_g = a.area[(size_t)base + g];
            // ---- oks(g, d) for every person still present; consumed at once ----
            bv = 0.0;
            bi = OKS_NONE;
            const bool want_oks = first && a.oks_first != nullptr;
            for (int d = tid; d < P; d += OKS_THREADS) {
                const size_t p = (size_t)base + d;
                double w = a.work[p];
                const bool present = d != g && w != removed && w == w;
                if (d == g) a.work[p] = removed;
                if (!present && !want_oks) continue;
                const float* k = a.kpts + p * (size_t)J * 3;
                const double half_area = (a_g + a.area[p]) / 2 + eps;
                double acc = 0.0;
                for (int j = 0; j < J; ++j) {
                    const float dx = k[3 * j] - s_gx[j];
                    const float dy = k[3 * j + 1] - s_gy[j];
                    const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
                    const double e = (double)d2 / s_var[j] / half_area / 2;
                    acc = acc + exp(-e);
                }
                const double oks = acc / (double)J;
                if (want_oks) a.oks_first[p] = oks;
                if (!present) continue;
                if (a.soft) {
                    w = w * exp(-(oks * oks) / a.oks_thre);
                    a.work[p] = w;
                } else if (oks > a.oks_thre) {
                    a.work[p] = removed;
                    continue;
                }
                if (w == w && w != removed && oks_better(w, d, bv, bi)) { bv = w; bi = d; }
            }
        }
        for (int d = nk + tid; d < P; d += OKS_THREADS) a.keep[(size_t)base + d] = -1;
        if (tid == 0) a.n_keep[img] = nk;
    }
}

int fpd_oks_nms_launch(const fpd_oks_nms_t& a, hipStream_t st) {
    int grid = a.grid > 0 ? a.grid : 4096;
    if (grid > a.n_img) grid = a.n_img;
    FPD_LAUNCH(oks_nms_kernel, dim3(grid), dim3(OKS_THREADS), 0, st, a);
    return 0;
}
