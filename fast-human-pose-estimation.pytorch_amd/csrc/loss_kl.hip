// JointsKLDLoss (soft-label KL over the spatial softmax of a heat map) for either term of the fused train step, the other term
// staying JointsMSELoss: pose + distillation term of every stack, forward and gradient, in two launches.  Per criterion call
// (maps s against r = target / teacher map, weight w, temperature T; p = softmax(s/T), q = softmax(r/T) over the hw pixels):
//   L[n,j] = w T^2 sum_x q_x ((r_x - s_x)/T - lse(r/T) + lse(s/T)),  loss = 1/(B J) sum L,  dloss/ds_x = w T (p_x - q_x) / (B J).
// With M = max_x of a row and Z = sum_x exp((x - M)/T), lse = M/T + log Z, so the bracket is a_x - b_x - log Z_r + log Z_s with
// a = (r - M_r)/T, b = (s - M_s)/T: the maxima cancel and nothing large is subtracted.  As sum_x q_x = 1 the two logarithms
// enter once per row, in fp64; what is summed over the pixels is exp(a_x) (a_x - b_x) / Z_r.  q_x == 0 contributes an exact 0,
// no logarithm of a probability is taken, and a reference row that equals the student row gives exactly 0 (same statistics
// routine, same order, a_x - b_x == 0).
//
// Fixed order throughout, no floating-point atomics but the grid-aligned loss terms (see loss_common.h): results are
// bit-repeatable and nothing needs zeroing but `losses`.  Geometry, the LDS turn of an NCHW target and the vector / scalar joint
// split are loss_common.h's, shared with loss_ohkm.hip.
//   1. kl_rows_kernel: block = (image, chunk of 128-pixel tiles).  Pass A takes the maximum of every row over the block's
//      pixels and sums the MSE terms; pass B (the same pixels, now cache-resident) sums exp((x - M)/T) row by row -- one exp per
//      element, no rescaling.  The block stores (M, Z) of every row and its two MSE sums to its own slab of the caller's scratch.
//   2. kl_grad_kernel: same grid; a block merges the slabs of its image in chunk order (fp64, the usual rescaling rule), walks
//      its pixels once more, writes the gradient with one rounding and adds its share of the two loss terms.
#include "conv_dispatch.h"
#include "loss_common.h"

// "equal rows give exactly zero" needs a product rounded the same way wherever it is formed: no contraction into an fma
#pragma clang fp contract(off)

namespace {

constexpr int PT = 128;                  // pixels per LDS tile of the target
constexpr int MAX_BLOCKS = 512;          // a block of launch 2 re-reads the slabs of its image: few chunks per image

// Rows of statistics.  Maxima do not depend on the temperature: [0, S) the stacks, S the target, S + 1 the teacher map.
// Sums do: 2 s + t the stack s at the temperature of term t (0 pose, 1 kd), 2 S the target (pose), 2 S + 1 the teacher (kd).
// Slab of one block, in doubles: M [S + 2][J], Z [2 S + 2][J], the two MSE sums.
__host__ __device__ __forceinline__ int slab_doubles(int S, int J) { return (3 * S + 4) * J + 2; }

// V joints per thread: a 16-byte vector (J a multiple of it, aligned maps) or one element (any J).  A thread keeps ONE joint
// vector jv = tid % vpad for all its pixels.  Which term is KL is compiled in, so that a launch carries the state of its own
// terms only; the row statistics of the second launch stay in LDS (a thread has few pixels: registers would buy nothing).
template <typename T, int V, int SMAX, bool KLP, bool KLK>
__global__ __launch_bounds__(256) void kl_rows_kernel(const fpd_loss_kl_t k, const LossGeo geo) {
    const fpd_loss_t& a = k.base;
    constexpr int NM = SMAX + 2, NZ = 2 * SMAX + 2;
    __shared__ float s_tg[PT * 33];
    __shared__ float s_m[4][NM * 32];            // per wave: maxima
    __shared__ float s_mb[NM * 32];              // of the block
    __shared__ double s_z[4][NZ * 32];           // per wave: sums
    __shared__ double s_mse[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int J = a.J, HW = a.H * a.W, LDJ = J + 1, S = a.S;
    const int tiles_per_img = cdiv_dev(HW, PT);
    const int b = blockIdx.x / geo.cpi, tile0 = (blockIdx.x - b * geo.cpi) * geo.tpb;
    const int tile1 = min(tile0 + geo.tpb, tiles_per_img);
    const int jv = tid & (geo.vpad - 1), pl = tid / geo.vpad, ppi = 256 / geo.vpad, j0 = jv * V;
    const bool on = j0 < J;
    constexpr bool klp = KLP, klk = KLK;         // which term is KL (the other is MSE): compiled in, each keeps only its own state
    const float itp = 1.f / k.temp_pose, itk = 1.f / k.temp_kd;
    const T* tch = reinterpret_cast<const T*>(a.teacher);
    const float NEG = -__builtin_inff();

    // pass A: the maximum of every row over the block's pixels, and the MSE terms
    {
        float w2[V], w2k[V], mx[NM][V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float wgt = on ? a.weight[b * J + j0 + e] : 0.f;
            const float wk = (on && a.weight_kd) ? a.weight_kd[b * J + j0 + e] : wgt;
            w2[e] = wgt * wgt; w2k[e] = wk * wk;
#pragma unroll
            for (int r = 0; r < NM; ++r) mx[r][e] = NEG;
        }
        float pose = 0.f, kd = 0.f;
        for (int tt = tile0; tt < tile1; ++tt) {
            const int p0 = tt * PT;
            __syncthreads();                     // the previous tile's targets have been read
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
                for (int e = 0; e < V; ++e) {
                    if (klp) mx[SMAX][e] = fmaxf(mx[SMAX][e], g[e]);
                    if (klk) mx[SMAX + 1][e] = fmaxf(mx[SMAX + 1][e], t[e]);
                }
#pragma unroll
                for (int s = 0; s < SMAX; ++s) {
                    if (s >= S) break;
                    float pv[V];
                    ld_vec<T, V>(reinterpret_cast<const T*>(a.out[s]) + off, pv);
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        mx[s][e] = fmaxf(mx[s][e], pv[e]);
                        if (!klp) { const float dg = pv[e] - g[e]; pose += w2[e] * dg * dg; }
                        if (!klk) { const float dt = pv[e] - t[e]; kd += w2k[e] * dt * dt; }
                    }
                }
            }
        }
        // lanes vpad apart hold the same joints: butterfly over them, then over the four waves through LDS
#pragma unroll
        for (int r = 0; r < NM; ++r)
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float v = mx[r][e];
                for (int o = 32; o >= geo.vpad; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
                if (on && lane < geo.vpad) s_m[wave][r * 32 + j0 + e] = v;
            }
        const double dp = wave_sum_d((double)pose), dk = wave_sum_d((double)kd);
        if (lane == 0) { s_mse[0][wave] = dp; s_mse[1][wave] = dk; }
    }
    __syncthreads();
    for (int i = tid; i < NM * 32; i += 256)
        if ((i & 31) < J) s_mb[i] = fmaxf(fmaxf(s_m[0][i], s_m[1][i]), fmaxf(s_m[2][i], s_m[3][i]));
    __syncthreads();

    // pass B, row by row (the same pixels, now cache-resident): sums of exp((x - M) / T), one exp per element and temperature
    for (int r = 0; r < S + 2; ++r) {
        const bool tgt = r == S, tea = r == S + 1;
        const bool zp = klp && !tea, zk = klk && !tgt;              // (block-uniform) which temperatures this row is summed at
        if (!zp && !zk) continue;
        const int mr = r < S ? r : SMAX + r - S;
        float m[V], z0[V], z1[V];
#pragma unroll
        for (int e = 0; e < V; ++e) { m[e] = on ? s_mb[mr * 32 + j0 + e] : 0.f; z0[e] = z1[e] = 0.f; }
        const T* src = tea ? tch : reinterpret_cast<const T*>(a.out[tgt ? 0 : r]);
        for (int tt = tile0; tt < tile1; ++tt) {
            const int p0 = tt * PT;
            if (tgt && geo.tpb > 1) {            // (with one tile per block pass A has left it in place)
                __syncthreads();
                load_target_tile<PT>(a, b, p0, s_tg);
                __syncthreads();
            }
            if (!on) continue;
            for (int p = pl; p < PT && p0 + p < HW; p += ppi) {
                float x[V];
                if (tgt) {
#pragma unroll
                    for (int e = 0; e < V; ++e) x[e] = s_tg[p * LDJ + j0 + e];
                } else {
                    ld_vec<T, V>(src + ((size_t)b * HW + p0 + p) * J + j0, x);
                }
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float c = x[e] - m[e];
                    if (zp) z0[e] += expf(c * itp);
                    if (zk) z1[e] += expf(c * itk);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            double v0 = (double)z0[e], v1 = (double)z1[e];
            for (int o = 32; o >= geo.vpad; o >>= 1) { v0 += __shfl_xor(v0, o, 64); v1 += __shfl_xor(v1, o, 64); }
            if (on && lane < geo.vpad) {
                if (r < S) { s_z[wave][(2 * r) * 32 + j0 + e] = v0; s_z[wave][(2 * r + 1) * 32 + j0 + e] = v1; }
                else s_z[wave][(2 * SMAX + r - S) * 32 + j0 + e] = tgt ? v0 : v1;
            }
        }
    }
    __syncthreads();
    double* slab = reinterpret_cast<double*>(k.scratch) + (size_t)blockIdx.x * slab_doubles(S, J);
    for (int i = tid; i < (S + 2) * J; i += 256) {
        const int r = i / J, j = i - r * J;
        slab[i] = (double)s_mb[(r < S ? r : SMAX + r - S) * 32 + j];
    }
    double* zs = slab + (S + 2) * J;
    for (int i = tid; i < (2 * S + 2) * J; i += 256) {
        const int r = i / J, j = i - r * J, term = r & 1, rr = (r < 2 * S ? r : 2 * SMAX + r - 2 * S) * 32 + j;
        zs[i] = (term ? klk : klp) ? ((s_z[0][rr] + s_z[1][rr]) + s_z[2][rr]) + s_z[3][rr] : 0.0;      // (a sum nobody asked for was not formed)
    }
    if (tid < 2) zs[(2 * S + 2) * J + tid] = ((s_mse[tid][0] + s_mse[tid][1]) + s_mse[tid][2]) + s_mse[tid][3];
}

template <typename T, int V, int SMAX, bool KLP, bool KLK>
__global__ __launch_bounds__(256) void kl_grad_kernel(const fpd_loss_kl_t k, const LossGeo geo) {
    const fpd_loss_t& a = k.base;
    constexpr int NM = SMAX + 2, NZ = 2 * SMAX + 2;
    __shared__ float s_tg[PT * 33];
    __shared__ float s_m[NM * 32];               // row maxima of the image
    __shared__ float s_izf[NZ * 32];             // 1 / Z, rounded once
    __shared__ double s_iz[NZ * 32];             // 1 / Z
    __shared__ double s_lz[NZ * 32];             // log Z, then (chunk 0) w (log Z_s - log Z_r) of a stack's rows
    __shared__ double s_wz[2][32];               // w / Z of the reference row of either term
    __shared__ float s_c[2][32];                 // coefficient of either term in the gradient
    __shared__ double s_acc[2][4];
    __shared__ double s_mse[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int J = a.J, HW = a.H * a.W, LDJ = J + 1, S = a.S;
    const int tiles_per_img = cdiv_dev(HW, PT);
    const int b = blockIdx.x / geo.cpi, chunk = blockIdx.x - b * geo.cpi, tile0 = chunk * geo.tpb;
    const int tile1 = min(tile0 + geo.tpb, tiles_per_img);
    constexpr bool klp = KLP, klk = KLK;         // which term is KL (the other is MSE): compiled in, each keeps only its own state
    const float itp = 1.f / k.temp_pose, itk = 1.f / k.temp_kd;
    const int sd = slab_doubles(S, J), nm = (S + 2) * J, nz = (2 * S + 2) * J;
    const double* slabs = reinterpret_cast<const double*>(k.scratch) + (size_t)b * geo.cpi * sd;
    // merge the chunks of this image, in chunk order: M = max M_c, Z = sum_c Z_c exp((M_c - M) / T)
    for (int i = tid; i < nz; i += 256) {
        const int r = i / J, j = i - r * J;
        const int term = r & 1, mr = r < 2 * S ? r >> 1 : S + term;     // the row of maxima this sum was taken against
        const int rr = (r < 2 * S ? r : 2 * SMAX + term) * 32 + j;
        if (!(term ? klk : klp)) { s_iz[rr] = 0.0; s_lz[rr] = 0.0; s_izf[rr] = 0.f; continue; }
        const double it = 1.0 / (double)(term ? k.temp_kd : k.temp_pose);
        const double* pm = slabs + mr * J + j;
        const double* pz = slabs + nm + i;
        double m = pm[0];
#pragma unroll 8
        for (int c = 1; c < geo.cpi; ++c) m = fmax(m, pm[(size_t)c * sd]);
        double zz = 0.0;
#pragma unroll 4
        for (int c = 0; c < geo.cpi; ++c) {
            const double mc = pm[(size_t)c * sd], zc = pz[(size_t)c * sd];
            zz += mc == m ? zc : zc * exp((mc - m) * it);
        }
        const double inv = 1.0 / zz;
        s_iz[rr] = inv; s_izf[rr] = (float)inv; s_lz[rr] = log(zz);
        if (r >= 2 * S || term == (klp ? 0 : 1)) s_m[(mr < S ? mr : SMAX + mr - S) * 32 + j] = (float)m;    // (one writer per row)
    }
    if (tid < 2) {
        double v = 0.0;
#pragma unroll 8
        for (int c = 0; c < geo.cpi; ++c) v += slabs[(size_t)c * sd + nm + nz + tid];
        s_mse[tid] = v;
    }
    __syncthreads();
    // d = gs ((1 - alpha) X + alpha Y) as in loss_adam.hip; an MSE term is w^2 (p - r), a KL term hw w T (softmax - softmax)
    if (tid < 2 * J) {
        const int term = tid >= J, j = tid - term * J;
        const float w = ((term && a.weight_kd) ? a.weight_kd : a.weight)[b * J + j];
        const bool kl = term ? klk : klp;
        s_c[term][j] = kl ? (float)HW * (term ? k.temp_kd : k.temp_pose) * w : w * w;
        s_wz[term][j] = kl ? (double)w * s_iz[(2 * SMAX + term) * 32 + j] : 0.0;
    }
    if (chunk == 0) {            // what enters a KL term once per row: w (log Z_s - log Z_r), left in the stack's slot of s_lz
        for (int i = tid; i < 2 * S * J; i += 256) {
            const int r = i / J, j = i - r * J, term = r & 1;
            const float* wgt = (term && a.weight_kd) ? a.weight_kd : a.weight;
            const double v = (term ? klk : klp) ? (double)wgt[b * J + j] * (s_lz[r * 32 + j] - s_lz[(2 * SMAX + term) * 32 + j]) : 0.0;
            s_lz[r * 32 + j] = v;                // (every thread reads the reference slots, which stay, and writes only its own)
        }
    }
    const int jv = tid & (geo.vpad - 1), pl = tid / geo.vpad, ppi = 256 / geo.vpad, j0 = jv * V;
    const bool on = j0 < J;
    const T* tch = reinterpret_cast<const T*>(a.teacher);
    const double cnt = (double)a.B * J * HW;
    const float gs = a.grad_scale / (float)cnt, ca = 1.f - a.alpha;
    double vp = 0.0, vk = 0.0;                   // sum over this thread's pixels and joints of w / Z_r exp(a) sum_s (a - b_s)
    for (int tt = tile0; tt < tile1; ++tt) {
        const int p0 = tt * PT;
        __syncthreads();
        load_target_tile<PT>(a, b, p0, s_tg);
        __syncthreads();
        if (!on) continue;
        for (int p = pl; p < PT && p0 + p < HW; p += ppi) {
            const size_t off = ((size_t)b * HW + p0 + p) * J + j0;
            float g[V], t[V], ag[V], eg[V], at[V], et[V], up[V], uk[V];      // u: sum over the stacks of a - b_s
#pragma unroll
            for (int e = 0; e < V; ++e) g[e] = s_tg[p * LDJ + j0 + e];
            ld_vec<T, V>(tch + off, t);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                ag[e] = eg[e] = at[e] = et[e] = up[e] = uk[e] = 0.f;
                if (klp) { ag[e] = (g[e] - s_m[SMAX * 32 + j0 + e]) * itp; eg[e] = expf(ag[e]); }
                if (klk) { at[e] = (t[e] - s_m[(SMAX + 1) * 32 + j0 + e]) * itk; et[e] = expf(at[e]); }
            }
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                if (s >= S) break;
                const bool wr = a.dout[s] != nullptr;
                float pv[V], d[V];
                ld_vec<T, V>(reinterpret_cast<const T*>(a.out[s]) + off, pv);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float c = pv[e] - s_m[s * 32 + j0 + e];
                    float x, y;
                    if (klp) {
                        const float bp = c * itp;
                        up[e] += ag[e] - bp;
                        x = wr ? expf(bp) * s_izf[(2 * s) * 32 + j0 + e] - eg[e] * s_izf[(2 * SMAX) * 32 + j0 + e] : 0.f;
                    } else x = pv[e] - g[e];
                    if (klk) {
                        const float bk = c * itk;
                        uk[e] += at[e] - bk;
                        y = wr ? expf(bk) * s_izf[(2 * s + 1) * 32 + j0 + e] - et[e] * s_izf[(2 * SMAX + 1) * 32 + j0 + e] : 0.f;
                    } else y = pv[e] - t[e];
                    d[e] = gs * (ca * s_c[0][j0 + e] * x + a.alpha * s_c[1][j0 + e] * y);
                }
                if (wr) st_vec<T, V>(reinterpret_cast<T*>(a.dout[s]) + off, d);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {        // (the products of two floats are exact in fp64)
                if (klp) vp += s_wz[0][j0 + e] * ((double)eg[e] * (double)up[e]);
                if (klk) vk += s_wz[1][j0 + e] * ((double)et[e] * (double)uk[e]);
            }
        }
    }
    // this block's share of the two loss terms; the chunk-0 block adds what enters once per row
    vp = wave_sum_d(vp); vk = wave_sum_d(vk);
    if (lane == 0) { s_acc[0][wave] = vp; s_acc[1][wave] = vk; }
    __syncthreads();
    if (tid < 2) {
        const bool kl = tid ? klk : klp;
        if (!kl && chunk != 0) return;           // an MSE term leaves through the chunk-0 block of its image
        double v;
        if (kl) {
            const double temp = (double)(tid ? k.temp_kd : k.temp_pose);
            v = ((s_acc[tid][0] + s_acc[tid][1]) + s_acc[tid][2]) + s_acc[tid][3];
            if (chunk == 0) {
                for (int s = 0; s < S; ++s)
                    for (int j = 0; j < J; ++j) v += s_lz[(2 * s + tid) * 32 + j];
            }
            v *= temp * temp / ((double)a.B * J);
        } else {
            v = s_mse[tid] * (0.5 / cnt);
        }
        loss_add_aligned(a.losses, tid, v);
    }
}

template <typename T, int V, int SMAX, bool KLP, bool KLK>
void kl_launch_m(const fpd_loss_kl_t& k, const LossGeo& g, hipStream_t st) {
    const dim3 grid((unsigned)(k.base.B * g.cpi));
    FPD_LAUNCH((kl_rows_kernel<T, V, SMAX, KLP, KLK>), grid, dim3(256), 0, st, k, g);
    FPD_LAUNCH((kl_grad_kernel<T, V, SMAX, KLP, KLK>), grid, dim3(256), 0, st, k, g);
}
template <typename T, int V, int SMAX>
void kl_launch(const fpd_loss_kl_t& k, const LossGeo& g, hipStream_t st) {
    if (k.kl_pose && k.kl_kd) kl_launch_m<T, V, SMAX, true, true>(k, g, st);
    else if (k.kl_pose) kl_launch_m<T, V, SMAX, true, false>(k, g, st);
    else kl_launch_m<T, V, SMAX, false, true>(k, g, st);
}
}  // namespace

int64_t fpd_loss_kl_scratch_size(const fpd_loss_t& a) {
    const LossGeo g = loss_geo(a, 1, PT, MAX_BLOCKS);
    return (int64_t)a.B * g.cpi * slab_doubles(a.S, a.J) * (int64_t)sizeof(double);
}

int fpd_loss_kl_launch(const fpd_loss_kl_t& k, hipStream_t st) {
    loss_dispatch(k.base, [&](auto t, auto v) {
        using T = typename decltype(t)::type;
        constexpr int V = decltype(v)::value;
        const LossGeo g = loss_geo(k.base, V, PT, MAX_BLOCKS);
        loss_dispatch_stacks(k.base.S, [&](auto smax) { kl_launch<T, V, decltype(smax)::value>(k, g, st); });
    });
    return 0;
}
