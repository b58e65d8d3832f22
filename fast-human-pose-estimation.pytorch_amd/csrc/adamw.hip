// torch.optim.AdamW (decoupled weight decay, optional AMSGrad, optional per-element exemption from the decay) over one flat
// fp32 arena (include/fpd_amd.h, fpd_adamw_t): one streaming launch + a one-thread tick of the step counter.  The arithmetic
// is csrc/adamw_math.h, which a host build checks against numpy (tests/test_adamw_cpu.py).  28 bytes move per element (param,
// grad, m, v read; param, m, v written), 36 with AMSGrad, + 2 with the bf16 copy, + 1/8 with the exemption mask: no LDS, no
// atomics, one writer per element.
#include <float.h>
#include "flat_stream.h"
#include "adamw_math.h"

namespace {

// The walk over the arenas (csrc/flat_stream.h) with the update stated once.  Element i's exemption is bit i & 31 of mask word
// i >> 5; the four elements of a vector lie in one word.  MASKED is a template parameter so that the load of that word stands
// unconditionally in its loop, where the four elements of a vector share it.
template <bool AMS, bool MASKED>
__device__ __forceinline__ void adamw_walk(const fpd_adamw_t& a, int64_t nvec, const fpd_adamw_coef_t& c, bool decay, const uint32_t* mask) {
    bf16_t* lp = reinterpret_cast<bf16_t*>(a.param_lp);
    const auto decays = [&](int64_t i) { return MASKED ? !((mask[i >> 5] >> (uint32_t)(i & 31)) & 1u) : decay; };
    if constexpr (AMS)
        flat_walk(a.n, nvec, lp, [&](int64_t i, float& p, float g, float& m, float& v, float& x) {
            p = fpd_adamw_update(p, g, &m, &v, &x, decays(i), c);
        }, a.param, a.grad, a.m, a.v, a.vmax);
    else
        flat_walk(a.n, nvec, lp, [&](int64_t i, float& p, float g, float& m, float& v) {
            p = fpd_adamw_update(p, g, &m, &v, nullptr, decays(i), c);
        }, a.param, a.grad, a.m, a.v);
}

// Every thread forms the coefficients itself from the step counter (two pow() in double), and no block can see the counter
// move: the tick is a launch of its own behind this one.
template <bool AMS>
__global__ __launch_bounds__(256) void adamw_kernel(const fpd_adamw_t a, const int64_t nvec) {
    float bc1 = a.bias_corr1, bc2 = a.bias_corr2, lr = a.lr;
    if (a.step_dev != nullptr) fpd_adamw_bias_corrections(a.beta1, a.beta2, *a.step_dev, &bc1, &bc2);
    if (a.lr_dev != nullptr) lr = *a.lr_dev;
    const fpd_adamw_coef_t c = fpd_adamw_coefs(lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.grad_scale, bc1, bc2);
    const bool decay = a.weight_decay != 0.f;
    if (decay && a.no_decay_bits != nullptr)                       // without a decay nobody reads the mask
        adamw_walk<AMS, true>(a, nvec, c, decay, a.no_decay_bits);
    else
        adamw_walk<AMS, false>(a, nvec, c, decay, nullptr);
}

}  // namespace

// Validation and the launch's geometry: the launch below and the query fpd_adamw_geometry() both come through here.  Pure
// host code: counts, coefficients and addresses are looked at, nothing is dereferenced.
int fpd_adamw_geometry_of(const fpd_adamw_t& a, int* blocks, int64_t* nvec) {
    if (const int rc = require_flat_n("adamw", a.n)) return rc;
    FPD_REQUIRE(a.param != nullptr && a.grad != nullptr && a.m != nullptr && a.v != nullptr, "adamw: null pointer (param, grad, m or v)");
    FPD_REQUIRE(a.weight_decay >= 0.f && a.weight_decay <= FLT_MAX, "adamw: invalid weight_decay value %g", (double)a.weight_decay);
    FPD_REQUIRE(a.beta1 >= 0.f && a.beta1 < 1.f, "adamw: invalid beta parameter at index 0: %g", (double)a.beta1);
    FPD_REQUIRE(a.beta2 >= 0.f && a.beta2 < 1.f, "adamw: invalid beta parameter at index 1: %g", (double)a.beta2);
    FPD_REQUIRE(a.eps >= 0.f, "adamw: invalid epsilon value %g", (double)a.eps);
    FPD_REQUIRE((((uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.m | (uintptr_t)a.v | (uintptr_t)a.vmax | (uintptr_t)a.lr_dev |
                  (uintptr_t)a.no_decay_bits) & 3) == 0 && ((uintptr_t)a.param_lp & 1) == 0 && ((uintptr_t)a.step_dev & 7) == 0,
                "adamw: a pointer is misaligned (4 bytes; param_lp 2, step_dev 8)");
    byte_range r[9];
    int nr = 0;
    const uint64_t fb = 4 * (uint64_t)a.n;
    if (a.n > 0) {
        r[nr++] = range_of(a.param, fb, true, "param");
        r[nr++] = range_of(a.grad, fb, false, "grad");
        r[nr++] = range_of(a.m, fb, true, "m");
        r[nr++] = range_of(a.v, fb, true, "v");
        if (a.vmax != nullptr) r[nr++] = range_of(a.vmax, fb, true, "vmax");
        if (a.param_lp != nullptr) r[nr++] = range_of(a.param_lp, fb / 2, true, "param_lp");
        if (a.no_decay_bits != nullptr) r[nr++] = range_of(a.no_decay_bits, 4 * (uint64_t)((a.n + 31) / 32), false, "no_decay_bits");
    }
    if (a.lr_dev != nullptr) r[nr++] = range_of(a.lr_dev, 4, false, "lr_dev");
    if (a.step_dev != nullptr) r[nr++] = range_of(a.step_dev, 8, true, "step_dev");
    if (const int rc = require_disjoint("adamw", r, nr)) return rc;
    flat_geometry(a.n, (uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.m | (uintptr_t)a.v | (uintptr_t)a.vmax, a.param_lp, nvec, blocks);
    return 0;
}

int fpd_adamw_launch(const fpd_adamw_t& a, hipStream_t st) {
    int blocks = 0;
    int64_t nvec = 0;
    const int rc = fpd_adamw_geometry_of(a, &blocks, &nvec);
    if (rc) return rc;
    if (a.vmax != nullptr)
        FPD_LAUNCH(adamw_kernel<true>, dim3(blocks), dim3(256), 0, st, a, nvec);
    else
        FPD_LAUNCH(adamw_kernel<false>, dim3(blocks), dim3(256), 0, st, a, nvec);
    if (a.step_dev != nullptr) FPD_LAUNCH(tick_kernel, dim3(1), dim3(1), 0, st, a.step_dev);
    return 0;
}
