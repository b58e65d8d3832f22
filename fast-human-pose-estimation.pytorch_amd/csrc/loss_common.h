// What the fused loss kernels (loss_adam.hip: MSE, loss_ohkm.hip, loss_kl.hip) have in common: vector loads and stores of a joint
// vector, the LDS turn of a target tile, the launch geometry, the vector / scalar decision, the dtype x V and SMAX dispatch and
// the grid-aligned loss add.  Loads, stores and index arithmetic only: the per-element arithmetic of a criterion stays in its own
// file, under that file's floating-point contraction setting (loss_kl.hip turns contraction off, the others do not).
#pragma once
#include <climits>

#include "common.h"

// V joints of one pixel: a 16-byte vector (V = DT<T>::VEC) or one element (V = 1)
template <typename T, int V>
__device__ __forceinline__ void ld_vec(const T* p, float* f) {
    if constexpr (V == 1) f[0] = DT<T>::ld(p);
    else DT<T>::unpack(*reinterpret_cast<const uint4*>(p), f);
}
template <typename T, int V>
__device__ __forceinline__ void st_vec(T* p, const float* f) {
    if constexpr (V == 1) DT<T>::st(p, f[0]);
    else *reinterpret_cast<uint4*>(p) = DT<T>::pack(f);
}

// targets of pixels [p0, p0 + PT) of image b -> s_tg[pixel][joint] (rows padded to J + 1); callers synchronise around it.  The fp32
// target arrives in the loader's NCHW layout: it is read coalesced along hw and turned through LDS, so that the NHWC maps are
// read and written with consecutive lanes on consecutive joints.
template <int PT>
__device__ __forceinline__ void load_target_tile(const fpd_loss_t& a, int b, int p0, float* s_tg) {
    const int J = a.J, HW = a.H * a.W, LDJ = J + 1, tid = threadIdx.x;
    if (a.target_nchw) {
        for (int i = tid; i < J * PT; i += 256) {
            const int j = i / PT, p = i - j * PT;
            s_tg[p * LDJ + j] = (p0 + p < HW) ? a.target[((size_t)b * J + j) * HW + p0 + p] : 0.f;
        }
    } else {
        for (int i = tid; i < J * PT; i += 256) {
            const int p = i / J, j = i - p * J;
            s_tg[p * LDJ + j] = (p0 + p < HW) ? a.target[((size_t)b * HW + p0 + p) * J + j] : 0.f;
        }
    }
}

// Order-independent sum over the blocks (bit-repeatable losses): every contribution is rounded to a multiple of 2^-44 (5.7e-14),
// so the fp64 additions are EXACT while the loss stays below 2^9 -- whatever order they arrive in.
__device__ __forceinline__ void loss_add_aligned(double* losses, int i, double v) {
    const double q = 17592186044416.0;           // 2^44
    atomicAdd(losses + i, rint(v * q) / q);
}

struct LossGeo {
    int tpb;       // tiles a block walks
    int cpi;       // chunks (= blocks) per image
    int vpad;      // joint vectors per pixel, rounded up to a power of two: lanes vpad apart hold the same joints
};
// Blocks of tpb PT-pixel tiles of one image, the fewest tiles per block that keep the grid within max_blocks (tpb and cpi do not
// depend on the vector width V).
static inline LossGeo loss_geo(const fpd_loss_t& a, int V, int PT, int max_blocks) {
    LossGeo g;
    const int tpi = cdiv(a.H * a.W, PT);
    g.tpb = 1;
    while (a.B * cdiv(tpi, g.tpb) > max_blocks && g.tpb < tpi) ++g.tpb;
    g.cpi = cdiv(tpi, g.tpb);
    g.vpad = 1;
    while (g.vpad * V < a.J) g.vpad <<= 1;
    return g;
}

// The one place that decides vector or scalar: 16-byte vectors of joints need J a multiple of the vector and every map a kernel
// touches that way (teacher, out[s], dout[s]; a null dout[s] is not written) on a 16-byte boundary.  Else one element per thread.
static inline int loss_vector_width(const fpd_loss_t& a) {
    const int vec = a.dtype == FPD_BF16 ? DT<bf16_t>::VEC : DT<float>::VEC;
    bool aligned = a.J % vec == 0 && ((uintptr_t)a.teacher & 15) == 0;
    for (int s = 0; s < a.S; ++s) aligned = aligned && ((uintptr_t)a.out[s] & 15) == 0 && ((uintptr_t)a.dout[s] & 15) == 0;
    return aligned ? vec : 1;
}

// f(type_c<T>, int_c<V>): T the storage type of a.dtype, V = loss_vector_width(a) as a constant
template <typename T>
struct type_c { using type = T; };
template <int N>
using int_c = std::integral_constant<int, N>;
template <typename F>
void loss_dispatch(const fpd_loss_t& a, F&& f) {
    const bool vec = loss_vector_width(a) > 1;
    if (a.dtype == FPD_BF16) {
        if (vec) f(type_c<bf16_t>{}, int_c<DT<bf16_t>::VEC>{});
        else f(type_c<bf16_t>{}, int_c<1>{});
    } else {
        if (vec) f(type_c<float>{}, int_c<DT<float>::VEC>{});
        else f(type_c<float>{}, int_c<1>{});
    }
}
// f(int_c<SMAX>): the register budget of per-stack state follows the stack count
template <typename F>
void loss_dispatch_stacks(int S, F&& f) {
    if (S == 1) f(int_c<1>{});
    else if (S == 2) f(int_c<2>{});
    else if (S <= 4) f(int_c<4>{});
    else f(int_c<FPD_MAX_STACKS>{});
}
