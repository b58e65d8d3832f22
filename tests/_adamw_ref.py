"""What the AdamW tests compare against: torch.optim.AdamW on the CPU and a numpy restatement, never this library.

Shared by tests/test_adamw_cpu.py and tests/test_adamw_gpu.py:

* restated(): the arithmetic of csrc/adamw_math.h in float32 numpy, one rounding per operation -- tests/_adam_ref.restated
  (the formula the Adam tests hold the bar of 2 against) with two insertions: p = p * (1 - lr * wd) in front of the moments
  where the element decays, and vmax = maximum(vmax, v) (a NaN wins) under AMSGrad.  A kernel has to give its bits.
* adamw_trajectory(): torch.optim.AdamW (foreach False) over one tensor in float32 or float64.  The criterion for general
  inputs is tests/_sgd_ref.assert_as_close_as_fp32: as far from float64 torch as twice what float32 torch is.
* three MUTANTS of the restatement that show the bar has teeth: 'l2' (the decay added to the gradient, as torch.optim.Adam
  does), 'no_decay' and 'no_max' (AMSGrad without the running maximum).  'no_max' shows only from the 'zero' start: from
  'randn' the parameter's own rounding (2^-24 of a value of size 1) hides a step of 2.5e-4 that is off by a few percent on
  few elements.
* the dyadic trajectory: betas 0, eps 0, weight decay 0.5, lrs (0.25, 0.25, 0.125), parameters k/8, gradients +-2^-j: every
  intermediate is exact in float32, so float32 torch, float64 torch and a kernel agree bit for bit on every element.
"""
import numpy as np
import torch

from tests._adam_ref import BETAS, EPS, LR, LRS, REGIMES, STARTS, bias_corrections, gradients as _adam_gradients, ratio, start  # noqa: F401

WDS = (0.01, 0.25)
ALL_REGIMES = REGIMES + ('shrink',)
MUTANTS = ('l2', 'no_decay', 'no_max')
DYADIC_LRS = (0.25, 0.25, 0.125)
DYADIC_WD = 0.5


def gradients(regime, n, steps=3, seed=0):
    """tests/_adam_ref.gradients, plus 'shrink': 0.01 randn, a fresh draw every step, 4 times smaller from step to step."""
    if regime != 'shrink':
        return _adam_gradients(regime, n, steps, seed)
    gen = torch.Generator().manual_seed(300 + seed)
    return [0.01 * 0.25 ** t * torch.randn(n, generator=gen) for t in range(steps)]


def adamw_trajectory(p0, grads, lrs=LRS, betas=BETAS, eps=EPS, weight_decay=0.01, amsgrad=False, dtype=torch.float32):
    """torch.optim.AdamW over one tensor -> (parameters, exp_avg, exp_avg_sq, max_exp_avg_sq or None) after the last step."""
    p = torch.nn.Parameter(p0.detach().to(dtype).clone())
    opt = torch.optim.AdamW([p], lr=lrs[0], betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, foreach=False, fused=False)
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]['lr'] = lr
        p.grad = g.detach().to(dtype).clone()
        opt.step()
    st = opt.state[p]
    mx = st['max_exp_avg_sq'].detach().clone() if amsgrad else None
    return p.detach().clone(), st['exp_avg'].detach().clone(), st['exp_avg_sq'].detach().clone(), mx


def restated(p0, grads, lrs=LRS, betas=BETAS, eps=EPS, weight_decay=0.01, amsgrad=False, grad_scale=1.0, exempt=None, mutant=None,
             state=None, first_step=1):
    """csrc/adamw_math.h in float32 numpy -> dict(p, m, v, vmax or None) of float32 CPU tensors.
    exempt: bool array, True = the element does not decay.  state: (m, v, vmax or None) to continue from, with first_step the
    number of the first step taken here."""
    f = np.float32
    p = p0.detach().numpy().astype(f).copy()
    if state is None:
        m, v, vmax = np.zeros_like(p), np.zeros_like(p), (np.zeros_like(p) if amsgrad else None)
    else:
        m, v = (x.detach().numpy().astype(f).copy() for x in state[:2])
        vmax = state[2].detach().numpy().astype(f).copy() if amsgrad else None
    b1, b2, e, one, wd = f(betas[0]), f(betas[1]), f(eps), f(1.0), f(weight_decay)
    decays = np.ones(p.shape, bool) if exempt is None else ~np.asarray(exempt, bool)
    if weight_decay == 0 or mutant == 'no_decay':
        decays = np.zeros(p.shape, bool)
    with np.errstate(invalid='ignore', divide='ignore'):
        for t, (g, lr) in enumerate(zip(grads, lrs), start=first_step):
            bc1, bc2 = bias_corrections(t, betas)
            step_size, inv = f(lr) / bc1, one / np.sqrt(bc2)
            g = g.detach().numpy().astype(f) * f(grad_scale)
            if mutant == 'l2':
                g = np.where(decays, g + wd * p, g).astype(f)
            else:
                lw = f(lr) * wd
                keep = one - lw
                p = np.where(decays, p * keep, p).astype(f)
            m = b1 * m + (one - b1) * g
            v = b2 * v + ((one - b2) * g) * g
            vhat = v
            if amsgrad:
                vmax = np.where((v > vmax) | np.isnan(v), v, vmax).astype(f)
                vhat = v if mutant == 'no_max' else vmax
            denom = np.sqrt(vhat) * inv + e
            p = p - step_size * (m / denom)
            assert p.dtype == f and m.dtype == f and v.dtype == f and denom.dtype == f and g.dtype == f
    t = torch.from_numpy
    return dict(p=t(p), m=t(m), v=t(v), vmax=t(vmax) if amsgrad else None)


def dyadic_inputs(n, seed=0):
    """The dyadic trajectory's inputs: parameters k/8 (|k| <= 16), one gradient +-2^-j (j in 0..3, never zero) per lr of DYADIC_LRS."""
    gen = torch.Generator().manual_seed(70 + seed)
    p0 = torch.randint(-16, 17, (n,), generator=gen).float() / 8
    grads = [0.5 ** torch.randint(0, 4, (n,), generator=gen).float() * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)
             for _ in DYADIC_LRS]
    return p0, grads


def dyadic_trajectory(p0, grads, amsgrad, dtype=torch.float32):
    return adamw_trajectory(p0, grads, DYADIC_LRS, (0.0, 0.0), 0.0, DYADIC_WD, amsgrad, dtype)


def mask_words(exempt):
    """bool array -> the uint32 words of fpd_adamw_t.no_decay_bits, by a direct loop: bit i & 31 of word i >> 5."""
    exempt = np.asarray(exempt, bool)
    words = np.zeros((exempt.size + 31) // 32, np.uint32)
    for i in np.flatnonzero(exempt):
        words[i >> 5] |= np.uint32(1 << (int(i) & 31))
    return words


def mask_ranges(n):
    """The exempt ranges of the mask tests: none on a 4- or 32-element boundary (n >= 80)."""
    return [(0, 1), (5, 70), (31, 33), (n - 3, n)]


def exempt_of(n, ranges):
    e = np.zeros(n, bool)
    for lo, hi in ranges:
        e[lo:hi] = True
    return e
