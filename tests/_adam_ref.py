"""What the Adam tests compare against: torch.optim.Adam on the CPU, never this library.

Shared by tests/test_step_cases_cpu.py and tests/test_step_kernels_gpu.py:

* adam_trajectory(): torch.optim.Adam (betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad) over one tensor, in float32
  or float64.  The criterion for general inputs is tests/_sgd_ref.assert_as_close_as_fp32: the kernel may be as far from
  float64 torch as twice what float32 torch is.
* restated(): the arithmetic of csrc/loss_adam.hip adam_kernel in float32 numpy, one rounding per operation (no contracted
  multiply-add): beta^t by pow() in double, step_size = lr / bias_corr1, 1 / sqrtf(bias_corr2) as a multiplier of sqrtf(v),
  eps added outside the root.  It shows that the bar of 2 is reachable by that formula; its three MUTANTS -- eps inside the
  bias-corrected root, sqrt(v + eps^2), a bias correction one step behind -- show that the bar has teeth.
* the degenerate trajectory beta1 = beta2 = 0, eps = 0: m = g, v = g*g, p -= lr * sign(g), every step exact on dyadic inputs,
  so a kernel has to reproduce parameters, m and v bit for bit on EVERY element.
"""
import numpy as np
import torch

LR = 2.5e-4
LRS = (LR, LR, LR)
BETAS = (0.9, 0.999)
EPS = 1e-8
REGIMES = ('small', 'eps', 'scales')
STARTS = ('zero', 'randn')
MUTANTS = ('eps_in_root', 'sqrt_v_eps2', 'stale_bias')
EXACT_LRS = (0.25, 0.25, 0.125)


def gradients(regime, n, steps=3, seed=0):
    """[gradient of step 1, 2, ...] as float32 CPU tensors: 'small' 0.01 randn; 'eps' 1e-8 randn (sqrt(v) of the size of eps);
    'scales' randn times a per-element scale 10^U(-10, 0) that stays the same over the steps."""
    gen = torch.Generator().manual_seed(100 + 7 * seed + REGIMES.index(regime))
    if regime == 'small':
        return [0.01 * torch.randn(n, generator=gen) for _ in range(steps)]
    if regime == 'eps':
        return [1e-8 * torch.randn(n, generator=gen) for _ in range(steps)]
    scale = (10.0 ** (-10.0 * torch.rand(n, generator=gen, dtype=torch.float64))).float()
    return [scale * torch.randn(n, generator=gen) for _ in range(steps)]


def start(kind, n, seed=0):
    if kind == 'zero':
        return torch.zeros(n)
    return torch.randn(n, generator=torch.Generator().manual_seed(900 + seed))


def adam_trajectory(p0, grads, lrs=LRS, betas=BETAS, eps=EPS, dtype=torch.float32):
    """torch.optim.Adam over one tensor: (parameters, exp_avg, exp_avg_sq) after the last step, in `dtype`."""
    p = torch.nn.Parameter(p0.detach().to(dtype).clone())
    opt = torch.optim.Adam([p], lr=lrs[0], betas=betas, eps=eps, weight_decay=0, amsgrad=False, foreach=False, fused=False)
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]['lr'] = lr
        p.grad = g.detach().to(dtype).clone()
        opt.step()
    st = opt.state[p]
    return p.detach().clone(), st['exp_avg'].detach().clone(), st['exp_avg_sq'].detach().clone()


def bias_corrections(t, betas=BETAS):
    """(1 - beta1^t, 1 - beta2^t) as the kernel forms them: the float32 betas, pow() in double, rounded to float32."""
    b1, b2 = np.float32(betas[0]), np.float32(betas[1])
    return np.float32(1.0 - float(b1) ** t), np.float32(1.0 - float(b2) ** t)


def restated(p0, grads, lrs=LRS, betas=BETAS, eps=EPS, grad_scale=1.0, mutant=None):
    """adam_kernel in float32 numpy -> (parameters, m, v) as float32 CPU tensors."""
    f = np.float32
    p = p0.detach().numpy().astype(f).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    b1, b2, e, one = f(betas[0]), f(betas[1]), f(eps), f(1.0)
    for t, (g, lr) in enumerate(zip(grads, lrs), start=1):
        bc1, bc2 = bias_corrections(t - 1 if mutant == 'stale_bias' and t > 1 else t, betas)
        step_size, inv = f(lr) / bc1, one / np.sqrt(bc2)
        g = g.detach().numpy().astype(f) * f(grad_scale)
        m = b1 * m + (one - b1) * g
        v = b2 * v + (one - b2) * g * g
        if mutant == 'eps_in_root':
            denom = np.sqrt(v + e) * inv
        elif mutant == 'sqrt_v_eps2':
            denom = np.sqrt(v + e * e) * inv
        else:
            denom = np.sqrt(v) * inv + e
        p = p - step_size * (m / denom)
        assert p.dtype == f and m.dtype == f and v.dtype == f and denom.dtype == f
    return torch.from_numpy(p), torch.from_numpy(m), torch.from_numpy(v)


def ratio(ours, r32, r64):
    """max|ours - r64| / max|r32 - r64| (what _sgd_ref.assert_as_close_as_fp32 bounds by 2), without asserting."""
    e32 = float((r32.double() - r64).abs().max())
    return float((ours.double() - r64).abs().max()) / e32 if e32 else float('inf')


def exact_inputs(n, seed=0):
    """The degenerate trajectory's inputs: parameters k/8 (|k| <= 16), gradients +-k/8 (k = 1..8, never zero), one per lr of EXACT_LRS."""
    gen = torch.Generator().manual_seed(40 + seed)
    p0 = torch.randint(-16, 17, (n,), generator=gen).float() / 8
    grads = [torch.randint(1, 9, (n,), generator=gen).float() / 8 * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)
             for _ in EXACT_LRS]
    return p0, grads


def exact_expected(p0, grads):
    """-> (parameters, m, v) after the steps of EXACT_LRS at beta1 = beta2 = 0, eps = 0, in closed form."""
    p = p0.double()
    for g, lr in zip(grads, EXACT_LRS):
        p = p - lr * torch.sign(g.double())
    return p.float(), grads[-1].clone(), grads[-1] * grads[-1]
