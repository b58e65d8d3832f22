"""numpy restatement of csrc/grad_clip_math.h (global gradient-norm clipping, utils.GradClipper / fpd_grad_clip), in its
operation order -- torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False):
    S = sum (double)g * (double)g        every product exact in float64; math.fsum adds them with ONE rounding
    norm = float32(sqrt(S))              float64 square root, one rounding into float32
    coef = max_norm / (norm + 1e-6f)     two float32 operations
    coef = 1 if coef > 1 else coef       a NaN stays a NaN
    g' = float32(g * coef)               one float32 rounding
numpy rounds every float32 operation on its own."""
import math

import numpy as np

EPS = np.float32(1e-6)


def sumsq(g):
    """Correctly rounded float64 sum of the exact squares (inf / NaN propagate as in IEEE addition)."""
    sq = np.asarray(g, np.float32).astype(np.float64) ** 2
    if not np.isfinite(sq).all():
        with np.errstate(all='ignore'):
            return float(sq.sum())
    return math.fsum(sq.tolist())


def norm_of(S):
    with np.errstate(all='ignore'):
        return np.float32(np.sqrt(np.float64(S)))


def coef_of(norm, max_norm):
    norm, max_norm = np.float32(norm), np.float32(max_norm)
    with np.errstate(all='ignore'):
        denom = np.float32(norm + EPS)
        coef = np.float32(max_norm / denom)
    return np.float32(1.0) if coef > np.float32(1.0) else coef


def scale(g, coef):
    with np.errstate(all='ignore'):
        return (np.asarray(g, np.float32) * np.float32(coef)).astype(np.float32)


def clip(g, max_norm):
    """(norm, coef, clipped gradient) of one call; the gradient is returned as it is when coef == 1 exactly."""
    g = np.asarray(g, np.float32)
    norm = norm_of(sumsq(g))
    coef = coef_of(norm, max_norm)
    return norm, coef, (g.copy() if coef == np.float32(1.0) else scale(g, coef))


# ---- dyadic gradients: s * m * 2^-6 with m in {0, 1, 2, 3}; every square is an integer multiple of 2^-12 and every partial sum
#      of fewer than 2^49 of them is exact in float64 IN ANY ORDER, so the device's norm has exactly one legal value ----

def dyadic(n, seed=0):
    rng = np.random.RandomState(seed)
    m = rng.randint(0, 4, n).astype(np.int64)
    s = rng.randint(0, 2, n).astype(np.int64) * 2 - 1
    return (s * m).astype(np.float32) * np.float32(2.0 ** -6), m


def dyadic_norm(m):
    """float32(sqrt(float64(S_int * 2^-12))) with S_int the exact integer sum of the squares."""
    s_int = int((np.asarray(m, np.int64) ** 2).sum())
    assert s_int < 2 ** 53
    return norm_of(np.float64(s_int) * np.float64(2.0 ** -12))


def next_after(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf), dtype=np.float32)


def math_cases():
    """(S, max_norm) pairs for the host build: ordinary values, norm + 1e-6f rounding back to norm, coef on both sides of 1 by
    one ulp, S = 0 / inf / NaN, max_norm = inf."""
    out = []
    rng = np.random.RandomState(7)
    for S in list(10.0 ** rng.uniform(-12, 12, 24)) + [0.0, 1.0, 4.0, 2.0 ** -140, 1e-300, 3.0e38 ** 2, 1e300, np.inf, np.nan]:
        norm = norm_of(S)
        ms = [1e-3, 0.05, 1.0, 10.0, 1e6, np.inf]
        if np.isfinite(norm) and norm > 0:
            denom = np.float32(norm + EPS)
            ms += [denom, next_after(denom, True), next_after(denom, False), norm, np.float32(norm * np.float32(0.5))]
        out += [(float(S), np.float32(m)) for m in ms]
    # norm + 1e-6f == norm from 2^5 on (half an ulp of 32 is 1.9e-6): max_norm == norm then gives coef == 1 exactly
    for norm in (32.0, 100.0, 4096.0):
        out.append((float(norm) ** 2, np.float32(norm)))
    return out
