// COCO keypoint AP on the device (lib/dataset/coco_eval.py: picture_oks, detection_area, match_picture, accumulate), two kernels:
//
// coco_match_kernel        one workgroup (one wave) per picture, grid-stride when the grid is capped.
//   phase 1  every lane: the (detection, gt) pairs of the picture -> oks[d,g] (float64, the host's operation order up to the
//            exp and the sum over joints) into the caller's buffer and, when the matrix fits, into LDS; the detections' own
//            areas; per gt one byte of flags (ignored per area range, crowd)
//   phase 2  lanes 0..29, one per (area range, threshold): the greedy matching.  The host sorts the gts "counting first" and
//            breaks at the first ignored gt once a counting match is in hand; here each detection walks the counting gts,
//            then -- only without a match -- the ignored ones: the same visits in the same order, without a sort.
//   Nothing of size G has a fixed capacity: up to COCO_FAST_G gts the taken flags are a 64-bit mask per lane and the gt
//   flags live in LDS; above, both live in the caller's scratch ([31, G_total] bytes: row 0 the gt flags, row 1 + lane the
//   taken flags of that lane).  The OKS matrix is read from LDS when D * G <= COCO_OKS_LDS, from the caller's buffer otherwise.
//
// coco_accum_kernel        one workgroup of 256 per (area range, threshold): a chunked inclusive scan of (tp, fp) with a
//   carried prefix, pr = tp / (fp + tp + eps); a chunked suffix maximum from the right with a carried maximum; per recall
//   threshold a binary search for the leftmost rank with tp / npig >= thr.  Integer counts and an exact maximum: bit-equal
//   to the host given equal flags.
#include "conv_dispatch.h"

#define COCO_THREADS 64
#define COCO_MAX_J 64
#define COCO_FAST_G 64
#define COCO_OKS_LDS 1024
#define COCO_LANES (FPD_COCO_AREAS * FPD_COCO_THRS)
#define COCO_CROWD 8                                     // bit of the per-gt flag byte; bits 0..2: ignored in area range r
#define ACC_THREADS 256
#define ACC_WAVES (ACC_THREADS / 64)

__global__ __launch_bounds__(COCO_THREADS) void coco_match_kernel(const fpd_coco_match_t a) {
#pragma clang fp contract(off)
    __shared__ double s_var[COCO_MAX_J];
    __shared__ double s_oks[COCO_OKS_LDS];
    __shared__ uint8_t s_flags[COCO_FAST_G];
    const int tid = threadIdx.x;
    const int J = a.J;
    const double eps = 2.220446049250313e-16;            // np.spacing(1)
    if (tid < J) {
        const double s2 = a.sigmas[tid] * 2.0;
        s_var[tid] = s2 * s2;
    }
    __syncthreads();
    for (int img = blockIdx.x; img < a.n_img; img += gridDim.x) {
        const int gbase = a.gt_offsets[img], G = a.gt_offsets[img + 1] - gbase;
        const int dbase = a.dt_offsets[img], D = a.dt_offsets[img + 1] - dbase;
        const int64_t obase = a.oks_offsets[img];
        const int64_t pairs = (int64_t)D * G;
        if (gbase < 0 || G < 0 || (int64_t)gbase + G > (int64_t)a.G_total || dbase < 0 || D < 0 ||
            (int64_t)dbase + D > (int64_t)a.D_total || obase < 0 || obase > a.oks_total || pairs > a.oks_total - obase) {
            if (tid == 0) a.status[img] = -1;            // a bad offset table: touch nothing of it (uniform: no barrier is skipped)
            continue;
        }
        const bool fast = G <= COCO_FAST_G, oks_lds = pairs <= COCO_OKS_LDS;
        uint8_t* const g_flags = a.scratch + gbase;      // row 0 of the scratch
        // ---- phase 1: gt flags, detection areas, the OKS matrix ----
        for (int g = tid; g < G; g += COCO_THREADS) {
            const double ar = a.gt_area[gbase + g];
            const uint8_t f = a.gt_flags[gbase + g];
            uint8_t out = (f & 2) ? COCO_CROWD : 0;
#pragma unroll
            for (int r = 0; r < FPD_COCO_AREAS; ++r)
                if ((f & 1) || ar < a.area_lo[r] || ar > a.area_hi[r]) out |= (uint8_t)(1 << r);
            if (fast) {
                s_flags[g] = out;
            } else {
                g_flags[g] = out;
                for (int l = 0; l < COCO_LANES; ++l) a.scratch[(size_t)(1 + l) * a.G_total + gbase + g] = 0;
            }
        }
        for (int d = tid; d < D; d += COCO_THREADS) {
            const double* k = a.dt_kpts + (size_t)(dbase + d) * J * 3;
            double x0 = k[0], x1 = k[0], y0 = k[1], y1 = k[1];
            for (int j = 1; j < J; ++j) {
                const double x = k[3 * j], y = k[3 * j + 1];
                x0 = x < x0 ? x : x0;
                x1 = x > x1 ? x : x1;
                y0 = y < y0 ? y : y0;
                y1 = y > y1 ? y : y1;
            }
            a.dt_area[dbase + d] = (x1 - x0) * (y1 - y0);
        }
        for (int64_t p = tid; p < pairs; p += COCO_THREADS) {
            const int d = (int)(p / G), g = (int)(p % G);
            const double* kd = a.dt_kpts + (size_t)(dbase + d) * J * 3;
            const double* kg = a.gt_kpts + (size_t)(gbase + g) * J * 3;
            const double area = a.gt_area[gbase + g] + eps;
            int n_on = 0;
            for (int j = 0; j < J; ++j) n_on += kg[3 * j + 2] > 0.0;
            double acc = 0.0;
            if (n_on) {
                for (int j = 0; j < J; ++j) {
                    if (!(kg[3 * j + 2] > 0.0)) continue;
                    const double dx = kd[3 * j] - kg[3 * j], dy = kd[3 * j + 1] - kg[3 * j + 1];
                    const double e = (dx * dx + dy * dy) / s_var[j] / area / 2;
                    acc = acc + exp(-e);
                }
            } else {
                const double* b = a.gt_bbox + (size_t)(gbase + g) * 4;
                const double bx0 = b[0] - b[2], bx1 = b[0] + b[2] * 2, by0 = b[1] - b[3], by1 = b[1] + b[3] * 2;
                for (int j = 0; j < J; ++j) {
                    const double xd = kd[3 * j], yd = kd[3 * j + 1];
                    const double ax = bx0 - xd, cx = xd - bx1, ay = by0 - yd, cy = yd - by1;
                    const double dx = (ax > 0 ? ax : 0.0) + (cx > 0 ? cx : 0.0);
                    const double dy = (ay > 0 ? ay : 0.0) + (cy > 0 ? cy : 0.0);
                    const double e = (dx * dx + dy * dy) / s_var[j] / area / 2;
                    acc = acc + exp(-e);
                }
            }
            const double o = acc / (double)(n_on ? n_on : J);
            a.oks[obase + p] = o;
            if (oks_lds) s_oks[p] = o;
        }
        __syncthreads();                                 // phase 2 reads what other lanes wrote (LDS and this workgroup's global rows)
        // ---- phase 2: one lane per (area range, threshold); no barrier inside ----
        if (tid < COCO_LANES) {
            const int r = tid / FPD_COCO_THRS;
            const double lo = a.area_lo[r], hi = a.area_hi[r], thr = a.oks_thrs[tid % FPD_COCO_THRS];
            const double floor0 = thr < 1 - 1e-10 ? thr : 1 - 1e-10;
            const uint8_t ign_bit = (uint8_t)(1 << r);
            const uint8_t* flags = fast ? s_flags : g_flags;
            const double* oks = oks_lds ? s_oks : a.oks + obase;
            uint8_t* taken = a.scratch + (size_t)(1 + tid) * a.G_total + gbase;      // (general path only)
            uint64_t mask = 0;                                                       // (fast path only)
            int counted = 0;
            for (int g = 0; g < G; ++g) counted += !(flags[g] & ign_bit);
            if (tid % FPD_COCO_THRS == 0) a.gt_counted[(size_t)r * a.n_img + img] = counted;
            uint8_t* out_m = a.matched + (size_t)tid * a.D_total + dbase;
            uint8_t* out_i = a.dt_ignored + (size_t)tid * a.D_total + dbase;
            for (int d = 0; d < D; ++d) {
                const double* row = oks + (size_t)d * G;
                double best = floor0;
                int m = -1, m_ignored = 0;
                for (int pass = 0; pass < 2 && m < 0; ++pass) {
                    for (int g = 0; g < G; ++g) {
                        const uint8_t f = flags[g];
                        if (((f & ign_bit) != 0) != (pass == 1)) continue;           // the other pass's gt
                        const bool tk = fast ? ((mask >> g) & 1) != 0 : taken[g] != 0;
                        if (tk && !(f & COCO_CROWD)) continue;
                        const double o = row[g];
                        if (o < best) continue;
                        best = o;
                        m = g;
                    }
                    m_ignored = pass;
                }
                if (m >= 0) {
                    out_m[d] = 1;
                    out_i[d] = (uint8_t)m_ignored;
                    if (fast) mask |= 1ull << m;
                    else taken[m] = 1;
                } else {
                    const double ar = a.dt_area[dbase + d];
                    out_m[d] = 0;
                    out_i[d] = (ar < lo || ar > hi) ? 1 : 0;
                }
            }
        }
        if (tid == 0) a.status[img] = 0;
        __syncthreads();                                 // the next picture overwrites s_oks / s_flags
    }
}

int fpd_coco_match_launch(const fpd_coco_match_t& a, hipStream_t st) {
    int grid = a.grid > 0 ? a.grid : 8192;
    if (grid > a.n_img) grid = a.n_img;
    FPD_LAUNCH(coco_match_kernel, dim3(grid), dim3(COCO_THREADS), 0, st, a);
    return 0;
}

// inclusive scans over the 256 threads of a block; `carry` (the value in front of / behind the chunk) is folded in
__device__ __forceinline__ long long acc_scan_add(long long v, long long* s_w, int lane, int wave) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    __syncthreads();                                     // the previous chunk's readers of s_w are done
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) v += s_w[w];
    return v;
}

__device__ __forceinline__ double acc_scan_max_right(double v, double* s_w, int lane, int wave) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_down(v, o, 64);
        if (lane + o < 64 && u > v) v = u;
    }
    __syncthreads();
    if (lane == 0) s_w[wave] = v;
    __syncthreads();
    for (int w = wave + 1; w < ACC_WAVES; ++w) v = s_w[w] > v ? s_w[w] : v;
    return v;
}

__global__ __launch_bounds__(ACC_THREADS) void coco_accum_kernel(const fpd_coco_accum_t a) {
#pragma clang fp contract(off)
    __shared__ long long s_cnt[ACC_WAVES];
    __shared__ double s_max[ACC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, r = b / FPD_COCO_THRS, k = b % FPD_COCO_THRS;
    const int D = a.D_total;
    const int npig = a.npig[r];
    const double eps = 2.220446049250313e-16;
    if (npig <= 0) {                                     // no gt counts in this range: the tables keep -1 (uniform)
        for (int q = tid; q < a.n_rec; q += ACC_THREADS) a.precision[((size_t)k * a.n_rec + q) * FPD_COCO_AREAS + r] = -1.0;
        if (tid == 0) { a.recall[k * FPD_COCO_AREAS + r] = -1.0; a.status[b] = 0; }
        return;
    }
    const uint8_t* matched = a.matched + (size_t)b * D;
    const uint8_t* ignored = a.dt_ignored + (size_t)b * D;
    int32_t* tp_out = a.tp + (size_t)b * D;
    double* env = a.env + (size_t)b * D;
    // ---- forward: (tp, fp) packed into one 64-bit count (tp low, fp high; D < 2^31), carried across chunks ----
    long long carry = 0;
    int bad = 0;
    for (int c = 0; c < D; c += ACC_THREADS) {           // (uniform trip count: the scans hold barriers)
        const int i = c + tid;
        long long v = 0;
        if (i < D) {
            const int o = a.order[i];
            if (o < 0 || o >= D) {
                bad = 1;
            } else if (!ignored[o]) {
                v = matched[o] ? 1ll : (1ll << 32);
            }
        }
        v = acc_scan_add(v, s_cnt, lane, wave) + carry;
        if (i < D) {
            const double tp = (double)(int)(v & 0xffffffffll), fp = (double)(int)(v >> 32);
            tp_out[i] = (int)(v & 0xffffffffll);
            env[i] = tp / (fp + tp + eps);
        }
        carry += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
    bad = __syncthreads_or(bad);
    // ---- backward: non-increasing from the right = suffix maximum, the maximum of the chunks behind carried ----
    double right = -1.0;                                 // below every precision (>= 0)
    const int chunks = (D + ACC_THREADS - 1) / ACC_THREADS;
    for (int c = (chunks - 1) * ACC_THREADS; c >= 0; c -= ACC_THREADS) {
        const int i = c + tid;
        double v = i < D ? env[i] : -1.0;                // (each thread rereads its own write of the forward pass)
        v = acc_scan_max_right(v, s_max, lane, wave);
        v = right > v ? right : v;
        if (i < D) env[i] = v;
        double m = s_max[0];
#pragma unroll
        for (int w = 1; w < ACC_WAVES; ++w) m = s_max[w] > m ? s_max[w] : m;
        right = right > m ? right : m;
    }
    __syncthreads();                                     // the searches below read other threads' tp / env
    // ---- per recall threshold: the leftmost rank with tp / npig >= thr ----
    const double n = (double)npig;
    for (int q = tid; q < a.n_rec; q += ACC_THREADS) {
        const double thr = a.rec_thrs[q];
        int lo = 0, hi = D;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if ((double)tp_out[mid] / n < thr) lo = mid + 1;
            else hi = mid;
        }
        a.precision[((size_t)k * a.n_rec + q) * FPD_COCO_AREAS + r] = lo < D ? env[lo] : 0.0;
    }
    if (tid == 0) {
        a.recall[k * FPD_COCO_AREAS + r] = D ? (double)tp_out[D - 1] / n : 0.0;
        a.status[b] = bad ? -1 : 0;
    }
}

int fpd_coco_accumulate_launch(const fpd_coco_accum_t& a, hipStream_t st) {
    FPD_LAUNCH(coco_accum_kernel, dim3(COCO_LANES), dim3(ACC_THREADS), 0, st, a);
    return 0;
}
