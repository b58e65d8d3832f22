// JointsOHKMMSELoss (online hard keypoint mining) for the fused train step: pose + distillation term of every stack, forward and
// gradient, in two launches.  Replaces the reference's lib/core/loss.py:42-84 as lib/core/function.py:128-134 would call it
// (2*S criterion calls + autograd).  Per criterion call, L[n,j] = 0.5 w[n,j]^2 / HW * sum_x (p - r)^2, the k joints with the largest
// L[n,:] of every sample are kept (among equal L the LOWER joint index wins), loss = 1/(B k) * sum of the kept L.  k = J keeps
// every joint = JointsMSELoss, which is how a mixed pair (one criterion OHKM, the other MSE) is evaluated.
//
// Fixed order throughout, no floating-point atomics but the two grid-aligned loss terms (see loss_common.h): results are
// bit-repeatable and nothing needs zeroing but `losses`.
//   1. ohkm_rows_kernel: block = (image, chunk of 128-pixel tiles); reads every stack's map, the target (turned through LDS like
//      loss_kernel) and the teacher map once and stores its partial sum w^2 (p-r)^2 of every (stack, term, joint) to its
//      own slab of the caller's scratch: double [B][chunks][S][2][J].
//   2. ohkm_grad_kernel: same grid; a block adds the slabs of its image in chunk order (fp64), ranks the joints of every
//      (stack, term) into a one-word mask, and writes the masked gradient of its pixels with one rounding.  The chunk-0 block
//      of an image adds the image's two loss terms and stores the masks.
#include "conv_dispatch.h"
#include "loss_common.h"

namespace {

constexpr int PT = 128;                  // pixels per LDS tile of the target
constexpr int MAX_BLOCKS = 512;          // a block of launch 2 re-reads the slabs of its image: few chunks per image

// V joints per thread: a 16-byte vector (J a multiple of it, aligned maps) or one element (any J).  A thread keeps ONE joint
// vector jv = tid % vpad for all its pixels, so its sums stay in registers: SMAX stacks x 2 terms x V joints.
template <typename T, int V, int SMAX>
__global__ __launch_bounds__(256) void ohkm_rows_kernel(const fpd_loss_ohkm_t k, const LossGeo geo) {
    const fpd_loss_t& a = k.base;
    __shared__ float s_tg[PT * 33];
    __shared__ double s_w[4][SMAX * 2 * 32];     // per wave: [stack][term][joint]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int J = a.J, HW = a.H * a.W, LDJ = J + 1, S = a.S;
    const int tiles_per_img = cdiv_dev(HW, PT);
    const int b = blockIdx.x / geo.cpi, tile0 = (blockIdx.x - b * geo.cpi) * geo.tpb;
    const int jv = tid & (geo.vpad - 1), pl = tid / geo.vpad, ppi = 256 / geo.vpad, j0 = jv * V;
    const bool on = j0 < J;
    const T* tch = reinterpret_cast<const T*>(a.teacher);
    float w2[V], w2k[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const float wgt = on ? a.weight[b * J + j0 + e] : 0.f;
        const float wk = (on && a.weight_kd) ? a.weight_kd[b * J + j0 + e] : wgt;
        w2[e] = wgt * wgt; w2k[e] = wk * wk;
    }
    float acc[SMAX][2][V];
#pragma unroll
    for (int s = 0; s < SMAX; ++s)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[s][0][e] = acc[s][1][e] = 0.f;
    for (int tt = tile0; tt < min(tile0 + geo.tpb, tiles_per_img); ++tt) {
        const int p0 = tt * PT;
        __syncthreads();                         // the previous tile's targets have been read
        load_target_tile<PT>(a, b, p0, s_tg);
        __syncthreads();
        if (!on) continue;
        for (int p = pl; p < PT && p0 + p < HW; p += ppi) {
            const size_t off = ((size_t)b * HW + p0 + p) * J + j0;
            float g[V], t[V];
#pragma unroll
            for (int e = 0; e < V; ++e) g[e] = s_tg[p * LDJ + j0 + e];
            ld_vec<T, V>(tch + off, t);
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                if (s >= S) break;
                float pv[V];
                ld_vec<T, V>(reinterpret_cast<const T*>(a.out[s]) + off, pv);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float dg = pv[e] - g[e], dt = pv[e] - t[e];
                    acc[s][0][e] += w2[e] * dg * dg;
                    acc[s][1][e] += w2k[e] * dt * dt;
                }
            }
        }
    }
    // lanes vpad apart hold the same joints: butterfly over them, lanes [0, vpad) of a wave end up with its sums
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
        if (s >= S) break;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < V; ++e) {
                double v = (double)acc[s][t][e];
                for (int o = 32; o >= geo.vpad; o >>= 1) v += __shfl_xor(v, o, 64);
                if (on && lane < geo.vpad) s_w[wave][(s * 2 + t) * 32 + j0 + e] = v;
            }
    }
    __syncthreads();
    double* slab = reinterpret_cast<double*>(k.scratch) + (size_t)blockIdx.x * S * 2 * J;
    for (int i = tid; i < S * 2 * J; i += 256) {
        const int q = i / J, j = i - q * J;
        slab[i] = ((s_w[0][q * 32 + j] + s_w[1][q * 32 + j]) + s_w[2][q * 32 + j]) + s_w[3][q * 32 + j];
    }
}

template <typename T, int V, int SMAX>
__global__ __launch_bounds__(256) void ohkm_grad_kernel(const fpd_loss_ohkm_t k, const LossGeo geo) {
    const fpd_loss_t& a = k.base;
    __shared__ float s_tg[PT * 33];
    __shared__ double s_row[SMAX * 2 * 32];      // sum w^2 (p-r)^2 over the image: [stack][term][joint]
    __shared__ double s_pair[SMAX * 2];
    __shared__ unsigned s_mask[SMAX * 2];
    const int tid = threadIdx.x;
    const int J = a.J, HW = a.H * a.W, LDJ = J + 1, S = a.S, nq = 2 * S;
    const int tiles_per_img = cdiv_dev(HW, PT);
    const int b = blockIdx.x / geo.cpi, chunk = blockIdx.x - b * geo.cpi, tile0 = chunk * geo.tpb;
    bool grads = false;
    for (int s = 0; s < S; ++s) grads |= a.dout[s] != nullptr;
    if (chunk != 0 && !grads) return;            // forward only: the chunk-0 block of an image does all there is to do
    if (tid < SMAX * 2) s_mask[tid] = 0u;
    const double* slabs = reinterpret_cast<const double*>(k.scratch) + (size_t)b * geo.cpi * nq * J;
    for (int i = tid; i < nq * J; i += 256) {
        double v = 0.0;
        for (int c = 0; c < geo.cpi; ++c) v += slabs[(size_t)c * nq * J + i];
        const int q = i / J;
        s_row[q * 32 + i - q * J] = v;
    }
    __syncthreads();
    // joint j is kept iff fewer than k joints come before it in the order (larger sum first, lower index first among equals);
    // the constant factor 0.5 / HW between the sums and L does not change the order
    for (int i = tid; i < nq * J; i += 256) {
        const int q = i / J, j = i - q * J, kk = (q & 1) ? k.topk_kd : k.topk_pose;
        const double v = s_row[q * 32 + j];
        const bool vn = v != v;                  // a NaN sum (diverged maps) ranks as the largest value, like torch.topk: still k bits
        int rank = 0;
        for (int m = 0; m < J; ++m) {
            const double u = s_row[q * 32 + m];
            const bool un = u != u;
            const bool before = un ? !vn : (!vn && u > v), same = un ? vn : u == v;
            rank += (before || (same && m < j)) ? 1 : 0;
        }
        if (rank < kk) atomicOr(&s_mask[q], 1u << j);
    }
    __syncthreads();
    const double bhw = (double)a.B * HW;
    if (chunk == 0) {
        if (tid < nq) {
            const unsigned m = s_mask[tid];
            double v = 0.0;
            for (int j = 0; j < J; ++j)
                if (m >> j & 1u) v += s_row[tid * 32 + j];
            s_pair[tid] = v;
            if (k.masks != nullptr) k.masks[(size_t)tid * a.B + b] = m;
        }
        __syncthreads();
        if (tid < 2) {
            double v = 0.0;
            for (int s = 0; s < S; ++s) v += s_pair[s * 2 + tid];
            v *= 0.5 / (bhw * (tid ? k.topk_kd : k.topk_pose));
            loss_add_aligned(a.losses, tid, v);
        }
    }
    if (!grads) return;
    const int jv = tid & (geo.vpad - 1), pl = tid / geo.vpad, ppi = 256 / geo.vpad, j0 = min(jv * V, 31);
    const bool on = jv * V < J;
    const T* tch = reinterpret_cast<const T*>(a.teacher);
    const float cp = (float)((double)a.grad_scale * (1.0 - (double)a.alpha) / (bhw * k.topk_pose));
    const float ck = (float)((double)a.grad_scale * (double)a.alpha / (bhw * k.topk_kd));
    float cw[V], cwk[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const float wgt = on ? a.weight[b * J + j0 + e] : 0.f;
        const float wk = (on && a.weight_kd) ? a.weight_kd[b * J + j0 + e] : wgt;
        cw[e] = cp * (wgt * wgt); cwk[e] = ck * (wk * wk);
    }
    unsigned mp[SMAX], mk[SMAX];                 // the masks, shifted to this thread's joints
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
        mp[s] = s < S ? s_mask[2 * s] >> j0 : 0u;
        mk[s] = s < S ? s_mask[2 * s + 1] >> j0 : 0u;
    }
    for (int tt = tile0; tt < min(tile0 + geo.tpb, tiles_per_img); ++tt) {
        const int p0 = tt * PT;
        __syncthreads();
        load_target_tile<PT>(a, b, p0, s_tg);
        __syncthreads();
        if (!on) continue;
        for (int p = pl; p < PT && p0 + p < HW; p += ppi) {
            const size_t off = ((size_t)b * HW + p0 + p) * J + j0;
            float g[V], t[V];
#pragma unroll
            for (int e = 0; e < V; ++e) g[e] = s_tg[p * LDJ + j0 + e];
            ld_vec<T, V>(tch + off, t);
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                if (s >= S) break;
                if (a.dout[s] == nullptr) continue;
                float pv[V], d[V];
                ld_vec<T, V>(reinterpret_cast<const T*>(a.out[s]) + off, pv);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float c0 = (mp[s] >> e & 1u) ? cw[e] : 0.f, c1 = (mk[s] >> e & 1u) ? cwk[e] : 0.f;
                    d[e] = c0 * (pv[e] - g[e]) + c1 * (pv[e] - t[e]);
                }
                st_vec<T, V>(reinterpret_cast<T*>(a.dout[s]) + off, d);
            }
        }
    }
}

template <typename T, int V, int SMAX>
void ohkm_launch(const fpd_loss_ohkm_t& k, const LossGeo& g, hipStream_t st) {
    const dim3 grid((unsigned)(k.base.B * g.cpi));
    FPD_LAUNCH((ohkm_rows_kernel<T, V, SMAX>), grid, dim3(256), 0, st, k, g);
    FPD_LAUNCH((ohkm_grad_kernel<T, V, SMAX>), grid, dim3(256), 0, st, k, g);
}

}  // namespace

int64_t fpd_loss_ohkm_scratch_size(const fpd_loss_t& a) {
    const LossGeo g = loss_geo(a, 1, PT, MAX_BLOCKS);
    return (int64_t)a.B * g.cpi * a.S * 2 * a.J * (int64_t)sizeof(double);
}

int fpd_loss_ohkm_launch(const fpd_loss_ohkm_t& k, hipStream_t st) {
    loss_dispatch(k.base, [&](auto t, auto v) {
        using T = typename decltype(t)::type;
        constexpr int V = decltype(v)::value;
        const LossGeo g = loss_geo(k.base, V, PT, MAX_BLOCKS);
        loss_dispatch_stacks(k.base.S, [&](auto smax) { ohkm_launch<T, V, decltype(smax)::value>(k, g, st); });
    });
    return 0;
}
