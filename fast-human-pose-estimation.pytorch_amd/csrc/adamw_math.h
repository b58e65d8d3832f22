// The arithmetic of AdamW / AMSGrad over a flat arena (include/fpd_amd.h, fpd_adamw_t), in the operation order of the numpy
// restatement (tests/_adamw_ref.py), one float32 rounding per operation, never fused:
//   t = step_done + 1;  bc1 = (float)(1 - pow((double)beta1, t));  bc2 likewise        pow() in double on the float32 betas
//   step_size = lr / bc1;  inv_sqrt_bc2 = 1 / sqrtf(bc2);  keep = 1 - lr * weight_decay
//   g = grad * grad_scale
//   p = p * keep                      only where the element decays: torch's param.mul_(1 - lr * wd), BEFORE the moments
//   m = beta1 * m + (1 - beta1) * g
//   v = beta2 * v + ((1 - beta2) * g) * g
//   vmax = (v > vmax || v != v) ? v : vmax;  vhat = vmax       AMSGrad (torch.maximum: a NaN wins); else vhat = v
//   denom = sqrtf(vhat) * inv_sqrt_bc2 + eps
//   p = p - step_size * (m / denom)
// This is csrc/loss_adam.hip adam_kernel (tests/_adam_ref.py restated()) with two insertions, the decay and the running
// maximum.  Host and device compile the same text with contraction off, so a host build is checked against numpy bit for bit
// without a GPU (tests/test_adamw_cpu.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if !defined(FPD_HD)
#if defined(__HIPCC__)
#define FPD_HD __host__ __device__
#else
#define FPD_HD
#endif
#endif

// what one launch applies to every element
typedef struct { float beta1, beta2, omb1, omb2, eps, step_size, inv_sqrt_bc2, keep, grad_scale; } fpd_adamw_coef_t;

// bias corrections of the step that follows `step_done` finished ones
FPD_HD static inline void fpd_adamw_bias_corrections(float beta1, float beta2, int64_t step_done, float* bc1, float* bc2) {
#pragma clang fp contract(off)
    const double t = (double)(step_done + 1);
    *bc1 = (float)(1.0 - pow((double)beta1, t));
    *bc2 = (float)(1.0 - pow((double)beta2, t));
}

FPD_HD static inline fpd_adamw_coef_t fpd_adamw_coefs(float lr, float beta1, float beta2, float eps, float weight_decay,
                                                      float grad_scale, float bc1, float bc2) {
#pragma clang fp contract(off)
    fpd_adamw_coef_t c;
    c.beta1 = beta1; c.beta2 = beta2; c.omb1 = 1.f - beta1; c.omb2 = 1.f - beta2;
    c.eps = eps; c.grad_scale = grad_scale;
    c.step_size = lr / bc1;
    c.inv_sqrt_bc2 = 1.f / sqrtf(bc2);
    const float lw = lr * weight_decay;
    c.keep = 1.f - lw;
    return c;
}

// One element.  decays: the decay reaches this element (weight_decay != 0 and no bit in the exemption mask).  vmax: the
// element's running maximum, NULL without AMSGrad.  Returns the new parameter; m, v and *vmax are updated in place.
FPD_HD static inline float fpd_adamw_update(float p, float grad, float* m, float* v, float* vmax, int decays, const fpd_adamw_coef_t c) {
#pragma clang fp contract(off)
    const float g = grad * c.grad_scale;
    if (decays) p = p * c.keep;
    const float bm = c.beta1 * *m, gm = c.omb1 * g;
    const float mn = bm + gm;
    const float bv = c.beta2 * *v, g1 = c.omb2 * g;
    const float g2 = g1 * g;
    const float vn = bv + g2;
    float vhat = vn;
    if (vmax != 0) {
        const float old = *vmax;
        vhat = (vn > old || vn != vn) ? vn : old;
        *vmax = vhat;
    }
    const float root = sqrtf(vhat);
    const float scaled = root * c.inv_sqrt_bc2;
    const float denom = scaled + c.eps;
    const float q = mn / denom;
    const float upd = c.step_size * q;
    *m = mn; *v = vn;
    return p - upd;
}
