"""What the SGD tests compare against: torch.optim.SGD on the CPU, never this library.

Two things are shared by tests/test_sgd_cpu.py and tests/test_sgd_gpu.py:

* the dyadic trajectory: parameters k/8 (|k| <= 16), gradients k/8 (|k| <= 8), lr 0.25, 0.25, 0.125 and momentum / weight
  decay from {0, 0.5} x {0, 0.25}.  Every intermediate of three steps is exactly representable in float32, so float32 and
  float64 torch agree bit for bit (asserted in test_sgd_cpu.py) and a kernel has to reproduce the parameters exactly,
  whichever multiply-adds it contracts.
* the criterion for general inputs: the kernel may be as far from float64 torch as twice what float32 torch is.  The factor
  2 allows for another choice of contracted multiply-adds than torch's CPU kernels make; a wrong formula (missing decay,
  sign, Nesterov term, stale lr) is off by three or more orders of magnitude.
"""
import torch

# (momentum, weight_decay, nesterov)
VARIANTS = [(0.5, 0.25, False), (0.0, 0.25, False), (0.5, 0.0, False), (0.0, 0.0, False), (0.5, 0.25, True), (0.5, 0.0, True)]
LRS = (0.25, 0.25, 0.125)


def dyadic_inputs(n, seed=0):
    """(parameters, [gradient of step 1, 2, 3]) as float32 CPU tensors of n elements."""
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randint(-16, 17, (n,), generator=gen).float() / 8
    grads = [torch.randint(-8, 9, (n,), generator=gen).float() / 8 for _ in LRS]
    return p0, grads


def sgd_trajectory(p0, grads, lrs, momentum, weight_decay, nesterov, dtype=torch.float32, buf0=None):
    """torch.optim.SGD over one tensor: [(parameters, momentum buffer or None) after each step], in `dtype`.
    buf0: momentum buffer to start from (a trajectory continued across calls)."""
    p = torch.nn.Parameter(p0.detach().to(dtype).clone())
    opt = torch.optim.SGD([p], lr=lrs[0], momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=nesterov,
                          maximize=False)
    if buf0 is not None:
        opt.state[p]['momentum_buffer'] = buf0.detach().to(dtype).clone()
    out = []
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]['lr'] = lr
        p.grad = g.detach().to(dtype).clone()
        opt.step()
        b = opt.state[p].get('momentum_buffer') if momentum != 0 else None
        out.append((p.detach().clone(), None if b is None else b.detach().clone()))
    return out


def assert_as_close_as_fp32(ours, r32, r64, label):
    """max|ours - r64| <= 2 max|r32 - r64|; returns the ratio of the two maxima."""
    e = float((ours.double() - r64).abs().max())
    e32 = float((r32.double() - r64).abs().max())
    assert e <= 2 * e32, '%s: max|ours - fp64 torch| = %.3e, max|fp32 torch - fp64 torch| = %.3e (ratio %.3f, allowed 2)' % (
        label, e, e32, e / e32 if e32 else float('inf'))
    return e / e32 if e32 else 0.0
