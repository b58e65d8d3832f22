#!/usr/bin/env python
"""Times fpd_sgd (csrc/loss_adam.hip sgd_kernel, one launch) against fpd_adam (adam_kernel + its tick, two launches) over one flat
arena, in alternating batches of back-to-back calls between two device events (so both see the same machine state).

    python tools/optim_bench.py [--n 3287936 --momentum 0.9 --wd 1e-4 --nesterov --rounds 7 --calls 200] [--out FILE]

The default n is the benchmark student's parameter count (hourglass, 4 stacks x 128 features).  Prints one line per round and a
summary: median us per call of either, their ratio and the bytes either moves per element (Adam 16 read + 12 written, SGD with
momentum 12 + 8, without 8 + 4)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fpd_amd import runtime as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=3287936)
    ap.add_argument('--momentum', type=float, default=0.9)
    ap.add_argument('--wd', type=float, default=1e-4)
    ap.add_argument('--nesterov', action='store_true')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'optim_bench needs the GPU'
    dev = torch.device('cuda:0')
    n = a.n
    gen = torch.Generator().manual_seed(0)
    param = torch.randn(n, generator=gen).to(dev)
    grad = (1e-3 * torch.randn(n, generator=gen)).to(dev)
    m, v, buf = (torch.zeros(n, device=dev) for _ in range(3))
    lr = torch.full((1,), 1e-6, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    ad = R.AdamT()
    ad.n, ad.param, ad.grad, ad.m, ad.v = n, param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr()
    ad.lr, ad.beta1, ad.beta2, ad.eps, ad.bias_corr1, ad.bias_corr2, ad.grad_scale = 0.0, 0.9, 0.999, 1e-8, 1.0, 1.0, 1.0
    ad.lr_dev, ad.step_dev = lr.data_ptr(), step.data_ptr()
    sg = R.SgdT()
    sg.n, sg.param, sg.grad = n, param.data_ptr(), grad.data_ptr()
    sg.buf = buf.data_ptr() if a.momentum != 0 else None
    sg.lr, sg.momentum, sg.weight_decay, sg.grad_scale, sg.nesterov = 0.0, a.momentum, a.wd, 1.0, int(a.nesterov)
    sg.lr_dev, sg.step_dev = lr.data_ptr(), step.data_ptr()
    lib, st = R.lib(), R.current_stream()
    calls = {'fpd_adam': lambda: R.check(lib.fpd_adam(ad, st), 'fpd_adam'),
             'fpd_sgd': lambda: R.check(lib.fpd_sgd(sg, st), 'fpd_sgd')}

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k

    for fn in calls.values():                   # warm-up: code objects loaded, caches in their steady state
        timed(fn, 20)
    lines = ['# optim_bench n=%d momentum=%g wd=%g nesterov=%d: us per call, %d back-to-back calls per sample, alternating'
             % (n, a.momentum, a.wd, a.nesterov, a.calls)]
    us = {k: [] for k in calls}
    for r in range(a.rounds):
        for k, fn in calls.items():
            us[k].append(timed(fn, a.calls))
        lines.append('round %d  fpd_adam %.2f us  fpd_sgd %.2f us' % (r, us['fpd_adam'][-1], us['fpd_sgd'][-1]))
    m0, m1 = statistics.median(us['fpd_adam']), statistics.median(us['fpd_sgd'])
    b_sgd = 20 if a.momentum != 0 else 12
    lines.append('median  fpd_adam %.2f us (min %.2f max %.2f)  fpd_sgd %.2f us (min %.2f max %.2f)  ratio %.2f'
                 % (m0, min(us['fpd_adam']), max(us['fpd_adam']), m1, min(us['fpd_sgd']), max(us['fpd_sgd']), m1 / m0))
    lines.append('bytes moved per call: adam %.1f MB (%.0f GB/s), sgd %.1f MB (%.0f GB/s); library %s'
                 % (28 * n / 1e6, 28 * n / m0 / 1e3, b_sgd * n / 1e6, b_sgd * n / m1 / 1e3, R.lib_sha16()))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
