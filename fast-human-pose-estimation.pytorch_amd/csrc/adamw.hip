// torch.optim.AdamW (decoupled weight decay, optional AMSGrad, optional per-element exemption from the decay) over one flat
// fp32 arena (include/fpd_amd.h, fpd_adamw_t): one streaming launch + a one-thread tick of the step counter.  The arithmetic
// is csrc/adamw_math.h, which a host build checks against numpy (tests/test_adamw_cpu.py).  28 bytes move per element (param,
// grad, m, v read; param, m, v written), 36 with AMSGrad, + 2 with the bf16 copy, + 1/8 with the exemption mask: no LDS, no
// atomics, one writer per element.
#include <float.h>
#include "common.h"
#include "conv_dispatch.h"
#include "adamw_math.h"

namespace {

// Every thread forms the coefficients itself from the step counter (two pow() in double), and no block can see the counter
// move: the tick is a launch of its own behind this one, as in fpd_adam and fpd_ema.
// nvec 16-byte vectors (0 when an arena is off the 16-byte grid), then elements [4 nvec, n) one by one.  A vector at index i
// covers elements 4 i .. 4 i + 3, which lie in one mask word: i >> 3, from bit 4 (i & 7).
template <bool AMS>
__global__ __launch_bounds__(256) void adamw_kernel(const fpd_adamw_t a, const int64_t nvec) {
    float bc1 = a.bias_corr1, bc2 = a.bias_corr2, lr = a.lr;
    if (a.step_dev != nullptr) fpd_adamw_bias_corrections(a.beta1, a.beta2, *a.step_dev, &bc1, &bc2);
    if (a.lr_dev != nullptr) lr = *a.lr_dev;
    const fpd_adamw_coef_t c = fpd_adamw_coefs(lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.grad_scale, bc1, bc2);
    const bool decay = a.weight_decay != 0.f;
    const uint32_t* mask = decay ? a.no_decay_bits : nullptr;      // without a decay nobody reads the mask
    bf16_t* lp = reinterpret_cast<bf16_t*>(a.param_lp);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    float4* p4 = reinterpret_cast<float4*>(a.param);
    const float4* g4 = reinterpret_cast<const float4*>(a.grad);
    float4* m4 = reinterpret_cast<float4*>(a.m);
    float4* v4 = reinterpret_cast<float4*>(a.v);
    float4* x4 = reinterpret_cast<float4*>(a.vmax);
    for (int64_t i = tid; i < nvec; i += nthr) {
        float4 p = p4[i], m = m4[i], v = v4[i], x = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 g = g4[i];
        if (AMS) x = x4[i];
        const uint32_t ex = mask != nullptr ? (mask[i >> 3] >> (4 * (uint32_t)(i & 7))) & 15u : 0u;
        p.x = fpd_adamw_update(p.x, g.x, &m.x, &v.x, AMS ? &x.x : nullptr, decay && !(ex & 1u), c);
        p.y = fpd_adamw_update(p.y, g.y, &m.y, &v.y, AMS ? &x.y : nullptr, decay && !(ex & 2u), c);
        p.z = fpd_adamw_update(p.z, g.z, &m.z, &v.z, AMS ? &x.z : nullptr, decay && !(ex & 4u), c);
        p.w = fpd_adamw_update(p.w, g.w, &m.w, &v.w, AMS ? &x.w : nullptr, decay && !(ex & 8u), c);
        m4[i] = m; v4[i] = v; p4[i] = p;
        if (AMS) x4[i] = x;
        if (lp) *reinterpret_cast<uint2*>(lp + 4 * i) = make_uint2(f2bf_pk(p.x, p.y), f2bf_pk(p.z, p.w));
    }
    for (int64_t i = 4 * nvec + tid; i < a.n; i += nthr) {
        float m = a.m[i], v = a.v[i], x = 0.f;
        if (AMS) x = a.vmax[i];
        const bool ex = mask != nullptr && ((mask[i >> 5] >> (uint32_t)(i & 31)) & 1u);
        const float p = fpd_adamw_update(a.param[i], a.grad[i], &m, &v, AMS ? &x : nullptr, decay && !ex, c);
        a.m[i] = m; a.v[i] = v; a.param[i] = p;
        if (AMS) a.vmax[i] = x;
        if (lp) lp[i] = f2bf(p);
    }
}
__global__ void adamw_tick_kernel(int64_t* step) { *step += 1; }

struct byte_range { uintptr_t lo, hi; bool written; const char* name; };
inline bool overlap(const byte_range& p, const byte_range& q) { return p.lo < q.hi && q.lo < p.hi; }

}  // namespace

// Validation and the launch's geometry: the launch below and the query fpd_adamw_geometry() both come through here.  Pure
// host code: counts, coefficients and addresses are looked at, nothing is dereferenced.
int fpd_adamw_geometry_of(const fpd_adamw_t& a, int* blocks, int64_t* nvec) {
    FPD_REQUIRE(a.n >= 0, "adamw: n = %lld is negative", (long long)a.n);
    FPD_REQUIRE(a.n < ((int64_t)1 << 60), "adamw: n = %lld is too large", (long long)a.n);
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
    const uintptr_t fb = 4 * (uintptr_t)a.n;
    if (a.n > 0) {
        r[nr++] = {(uintptr_t)a.param, (uintptr_t)a.param + fb, true, "param"};
        r[nr++] = {(uintptr_t)a.grad, (uintptr_t)a.grad + fb, false, "grad"};
        r[nr++] = {(uintptr_t)a.m, (uintptr_t)a.m + fb, true, "m"};
        r[nr++] = {(uintptr_t)a.v, (uintptr_t)a.v + fb, true, "v"};
        if (a.vmax != nullptr) r[nr++] = {(uintptr_t)a.vmax, (uintptr_t)a.vmax + fb, true, "vmax"};
        if (a.param_lp != nullptr) r[nr++] = {(uintptr_t)a.param_lp, (uintptr_t)a.param_lp + fb / 2, true, "param_lp"};
        if (a.no_decay_bits != nullptr)
            r[nr++] = {(uintptr_t)a.no_decay_bits, (uintptr_t)a.no_decay_bits + 4 * (uintptr_t)((a.n + 31) / 32), false, "no_decay_bits"};
    }
    if (a.lr_dev != nullptr) r[nr++] = {(uintptr_t)a.lr_dev, (uintptr_t)a.lr_dev + 4, false, "lr_dev"};
    if (a.step_dev != nullptr) r[nr++] = {(uintptr_t)a.step_dev, (uintptr_t)a.step_dev + 8, true, "step_dev"};
    for (int i = 0; i < nr; ++i)
        for (int j = i + 1; j < nr; ++j)
            FPD_REQUIRE(!((r[i].written || r[j].written) && overlap(r[i], r[j])), "adamw: %s overlaps %s (a written range must not alias another)",
                        r[i].name, r[j].name);
    const uintptr_t bits = (uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.m | (uintptr_t)a.v | (uintptr_t)a.vmax;
    const bool aligned = (bits & 15) == 0 && ((uintptr_t)a.param_lp & 7) == 0;
    *nvec = aligned ? a.n / 4 : 0;
    const int64_t rest = a.n - 4 * *nvec;
    *blocks = grid_for(*nvec > rest ? *nvec : rest);
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
    if (a.step_dev != nullptr) FPD_LAUNCH(adamw_tick_kernel, dim3(1), dim3(1), 0, st, a.step_dev);
    return 0;
}
