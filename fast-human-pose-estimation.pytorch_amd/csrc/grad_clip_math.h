// The arithmetic of global gradient-norm clipping (include/fpd_amd.h, fpd_grad_clip_t) behind the float64 sum of squares S,
// in the operation order of torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False) and of the numpy
// restatement (tests/_clip_ref.py):
//   norm = (float)sqrt(S)                     float64 square root, ONE rounding into float32
//   coef = max_norm / (norm + 1e-6f)          two float32 operations
//   coef = coef > 1 ? 1 : coef                torch's clamp(max=1): a NaN stays a NaN, so no fminf
//   g'   = g * coef                           one float32 rounding
// max_norm = +inf gives coef = 1 by the formula (inf > 1); a non-finite norm gives coef 0 (norm = inf, finite max_norm) or
// NaN (norm NaN, or inf / inf), which the scale then writes into every element, as torch does.
// Host and device compile the same text, so a host build is checked against numpy bit for bit without a GPU
// (tests/test_clip_cpu.py).
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

FPD_HD static inline float fpd_clip_norm(double sumsq) { return (float)sqrt(sumsq); }

FPD_HD static inline float fpd_clip_coef(float norm, float max_norm) {
#pragma clang fp contract(off)
    const float denom = norm + 1e-6f;
    const float coef = max_norm / denom;
    return coef > 1.0f ? 1.0f : coef;
}

FPD_HD static inline float fpd_clip_scale(float g, float coef) { return g * coef; }
