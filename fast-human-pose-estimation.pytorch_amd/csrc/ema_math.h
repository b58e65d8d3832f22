// The arithmetic of the weight average (include/fpd_amd.h, fpd_ema_t): the weight of one update from the number of updates
// done so far, and the update of one element, in the operation order of the numpy restatement (tests/_ema_ref.py):
//   u = updates_done + 1
//   d = warmup ? min(decay, (1 + u) / (10 + u)) : decay         float64; one division, no pow, nothing of libm
//   w = (float)(1 - d)                                          one rounding into float32
//   e' = e + w * (x - e)                                        three float32 roundings, never fused
// The warm-up is timm's ModelEmaV3 / the ExpMomentumEMA ramp: the average follows the weights closely while they still move
// fast (d = 2/11 at the first update) and reaches `decay` once (1 + u) / (10 + u) overtakes it (u = 44 990 for 0.9998).
// Host and device compile the same text with contraction off, so a host build is checked against numpy bit for bit without
// a GPU (tests/test_ema_cpu.py).
#pragma once
#include <stdint.h>

#if !defined(FPD_HD)
#if defined(__HIPCC__)
#define FPD_HD __host__ __device__
#else
#define FPD_HD
#endif
#endif

// updates_done < 2^52 converts exactly; decay in [0, 1) (the entry point refuses anything else)
FPD_HD static inline float fpd_ema_weight(int64_t updates_done, double decay, int warmup) {
#pragma clang fp contract(off)
    const double u = (double)(updates_done + 1);
    double d = decay;
    if (warmup) {
        const double ramp = (1.0 + u) / (10.0 + u);
        if (ramp < d) d = ramp;
    }
    return (float)(1.0 - d);
}

FPD_HD static inline float fpd_ema_update(float e, float x, float w) {
#pragma clang fp contract(off)
    const float diff = x - e;
    const float step = w * diff;
    return e + step;
}
