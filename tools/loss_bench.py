#!/usr/bin/env python
"""Times fpd_loss_ohkm (csrc/loss_ohkm.hip, two launches) against fpd_loss (csrc/loss_adam.hip, one launch) at one shape, on the
same buffers, in alternating batches of back-to-back calls between two device events (so both see the same machine state).

    python tools/loss_bench.py [--batch 32 --joints 16 --size 64 --stacks 4 --dtype bf16 --topk 8 --rounds 7 --calls 200] [--out FILE]

Prints one line per round and a summary: median us per call of either, their ratio, and the budget the new path was given
(twice the fpd_loss time: it reads the maps twice; plus one launch gap, reported separately as the time of an empty-handed
second launch is not measured here)."""
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
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--joints', type=int, default=16)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--stacks', type=int, default=4)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--topk', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'loss_bench needs the GPU'
    dev = torch.device('cuda:0')
    B, J, H, S = a.batch, a.joints, a.size, a.stacks
    dt, tdt = (R.BF16, torch.bfloat16) if a.dtype == 'bf16' else (R.F32, torch.float32)
    gen = torch.Generator().manual_seed(0)
    outs = [torch.randn(B, H, H, J, generator=gen).to(tdt).to(dev) for _ in range(S)]
    douts = [torch.empty_like(o) for o in outs]
    teacher = torch.randn(B, H, H, J, generator=gen).to(tdt).to(dev)
    target = torch.rand(B, J, H, H, generator=gen).to(dev)
    weight = torch.rand(B, J, generator=gen).to(dev)
    losses = torch.zeros(2, dtype=torch.float64, device=dev)
    k = R.LossOhkmT()
    for s in (k.base, ):
        s.B, s.J, s.H, s.W, s.S, s.dtype, s.target_nchw, s.alpha, s.grad_scale = B, J, H, H, S, dt, 1, 0.5, 1.0
        for i in range(S):
            s.out[i], s.dout[i] = outs[i].data_ptr(), douts[i].data_ptr()
        s.teacher, s.target, s.weight, s.losses = teacher.data_ptr(), target.data_ptr(), weight.data_ptr(), losses.data_ptr()
    k.topk_pose = k.topk_kd = a.topk
    nbytes = R.lib().fpd_loss_ohkm_scratch_bytes(k.base)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    masks = torch.zeros(S * 2 * B, dtype=torch.int32, device=dev)
    k.scratch, k.scratch_bytes, k.masks = scratch.data_ptr(), nbytes, masks.data_ptr()
    lib, st = R.lib(), R.current_stream()
    calls = {'fpd_loss': lambda: R.check(lib.fpd_loss(k.base, st), 'fpd_loss'),
             'fpd_loss_ohkm': lambda: R.check(lib.fpd_loss_ohkm(k, st), 'fpd_loss_ohkm')}

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    for fn in calls.values():                   # warm-up: code objects loaded, caches in their steady state
        timed(fn, 20)
    lines = ['# loss_bench B=%d J=%d %dx%d S=%d %s topk=%d: us per call, %d back-to-back calls per sample, alternating'
             % (B, J, H, H, S, a.dtype, a.topk, a.calls)]
    us = {n: [] for n in calls}
    for r in range(a.rounds):
        for n, fn in calls.items():
            us[n].append(timed(fn, a.calls))
        lines.append('round %d  fpd_loss %.2f us  fpd_loss_ohkm %.2f us' % (r, us['fpd_loss'][-1], us['fpd_loss_ohkm'][-1]))
    m0, m1 = statistics.median(us['fpd_loss']), statistics.median(us['fpd_loss_ohkm'])
    traffic = (S + 1) * B * H * H * J * (2 if a.dtype == 'bf16' else 4) + B * J * H * H * 4
    lines.append('median  fpd_loss %.2f us (min %.2f max %.2f)  fpd_loss_ohkm %.2f us (min %.2f max %.2f)  ratio %.2f  budget 2 x fpd_loss = %.2f us (+ one launch gap)'
                 % (m0, min(us['fpd_loss']), max(us['fpd_loss']), m1, min(us['fpd_loss_ohkm']), max(us['fpd_loss_ohkm']), m1 / m0, 2 * m0))
    lines.append('bytes read per pass over the maps %.1f MB, gradients written %.1f MB; library %s'
                 % (traffic / 1e6, S * B * H * H * J * (2 if a.dtype == 'bf16' else 4) / 1e6, R.lib_sha16()))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
