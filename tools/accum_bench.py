#!/usr/bin/env python
"""What gradient accumulation (FusedFPDStep accum=, csrc/grad_accum.hip) costs, in ONE process and ONE call.

    python tools/accum_bench.py [--pairs 6 --launches 100 --steps 40 --parts lt --accum 4] [--out profiles/accum_bench.txt]

(l) The op alone: fpd_grad_accum in each of its three modes over two flat arenas of the benchmark's hourglass student
    (3 287 936 elements) and of the HRNet-W32 student (28 536 113), beside fpd_adam at the same n.  Every call is timed on its
    own between two device events, the method of tools/clip_bench.py, so that the figures compare with that tool's; `--pairs`
    windows of `--launches` calls after one untimed window.  Both arenas stay in the 256 MB Infinity Cache where they fit
    (2 x 13 MB do, 2 x 114 MB in part).
(t) The whole step on the benchmark pair (hg4x128 bf16 student, hg8x256 bf16 teacher, batch 32, 256x256) on ONE
    FusedFPDStep(accum=k): `--pairs` interleaved pairs of `--steps` pipelined micro-batches between two device events, one
    untimed window each, with the step's window length switched between 1 (student_step then takes the path of a step built
    without accum=: the three new ranges are not run) and k.  Same streams, same arenas, same plan: nothing but the path
    differs.  Time is per micro-batch.  At k the optimizer range runs once per k micro-batches and one accumulate launch is
    paid per micro-batch, so the sign is not predicted.
The rule of the other tools decides: a difference is ESTABLISHED only if the mean difference is at least twice the largest
same-path spread and every run of one setting beats every run of the other."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')      # as bench.py: before torch loads the HIP runtime

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fpd_amd import executor as E  # noqa: E402
from fpd_amd import runtime as R  # noqa: E402
from fpd_amd import synth  # noqa: E402
from fpd_amd.lib.models import hourglass  # noqa: E402

MODES = (('FIRST', R.ACCUM_FIRST, 8), ('ADD', R.ACCUM_ADD, 12), ('FIN', R.ACCUM_FIN, 8))      # name, mode, bytes moved per element


class AD(dict):
    __getattr__ = dict.__getitem__


def hg_cfg(feats, stacks, joints=16, dtype='bf16'):
    return AD(MODEL=AD(NUM_JOINTS=joints, DTYPE=dtype, EXTRA=AD(NUM_FEATURES=feats, NUM_STACKS=stacks, NUM_BLOCKS=1)))


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def per_call_us(call, pairs, launches):
    """Mean microseconds of call() per window, each call between its own two events."""
    def window():
        evs = []
        for _ in range(launches):
            e0, e1 = events()
            e0.record()
            call()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        return float(np.mean([a.elapsed_time(b) for a, b in evs])) * 1e3
    window()
    return np.array([window() for _ in range(pairs)])


def op_alone(lines, name, n, pairs, launches):
    lib, st, dev = R.lib(), R.current_stream(), torch.device('cuda:0')
    g, acc = torch.randn(n, device=dev) * 1e-3, torch.zeros(n, device=dev)
    scale = torch.full((1,), 0.25, device=dev)
    a = R.GradAccumT()
    a.n, a.grad, a.acc, a.scale_dev = n, g.data_ptr(), acc.data_ptr(), scale.data_ptr()
    blocks, vec = R.C.c_int32(), R.C.c_int64()
    a.mode = R.ACCUM_ADD
    R.check(lib.fpd_grad_accum_geometry(a, blocks, vec), 'fpd_grad_accum_geometry')
    lines.append('%-10s n = %d (2 x %.1f MB): grid %d x 256, %d trip(s) over the %d-element vector part'
                 % (name, n, 4 * n / 1e6, blocks.value, -(-(vec.value // 4) // (blocks.value * 256)), vec.value))
    res = {}
    for label, mode, moved in MODES:
        a.mode = mode
        acc.zero_()
        us = per_call_us(lambda: R.check(lib.fpd_grad_accum(a, st), 'fpd_grad_accum'), pairs, launches)
        res[label] = us
        lines.append('%-10s fpd_grad_accum, %-6s %8.2f us per call (min %.2f max %.2f over %d windows of %d calls): %d B/element moved, %.2f TB/s'
                     % ('', label + ':', us.mean(), us.min(), us.max(), pairs, launches, moved, moved * n / us.mean() / 1e6))
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(acc).all())
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    lr_dev, step_dev = torch.full((1,), 1e-3, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    d = R.AdamT()
    d.n, d.param, d.grad, d.m, d.v, d.param_lp = n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None
    d.lr, d.beta1, d.beta2, d.eps, d.bias_corr1, d.bias_corr2, d.grad_scale = 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, 1.0
    d.lr_dev, d.step_dev = lr_dev.data_ptr(), step_dev.data_ptr()
    us = per_call_us(lambda: R.check(lib.fpd_adam(d, st), 'fpd_adam'), pairs, launches)
    lines.append('%-10s fpd_adam beside it:     %8.2f us per call (min %.2f max %.2f): 28 B/element moved, %.2f TB/s'
                 % ('', us.mean(), us.min(), us.max(), 28 * n / us.mean() / 1e6))
    return {k: float(v.mean()) for k, v in res.items()}


def build_pair(x, tg, tw, k):
    dev = torch.device('cuda:0')
    B, H, W = 32, 256, 256
    torch.manual_seed(1)
    s = hourglass.get_pose_net(hg_cfg(128, 4), is_train=True).to(dev)
    torch.manual_seed(2)
    t = hourglass.get_pose_net(hg_cfg(256, 8), is_train=False).to(dev)
    cal = E.GraphInstance(t.device_state(), t.cfg_hg, B, H, W, train=True).finalize()
    cal.image().copy_(x)
    cal.run('prep'); cal.run('fwd')
    cal.calibrate_running_stats()
    del cal
    step = E.FusedFPDStep(s.device_state(), s.cfg_hg, t.device_state(), t.cfg_hg, B, H, W, alpha=0.5, lr=2.5e-4, accum=k)
    step.set_batch(x, tg, tw)
    step.run_pipelined(k)
    return s, t, step


def window(step, steps):
    e0, e1 = events()
    e0.record()
    step.run_pipelined(steps)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def toggled_step(lines, pairs, steps, k, op_us):
    assert steps % k == 0, '--steps must be a multiple of --accum: every timed window then holds whole windows only'
    x, tg, tw = synth.make_batch(1000, 32, 16, (256, 256), (64, 64))
    s, t, step = build_pair(x, tg, tw, k)
    runs = {1: [], k: []}
    for length in runs:                       # run_pipelined ends with flush(): no window is open when the length changes
        step.accum = length
        window(step, steps)
    before = (step.updates, int(step.step_dev))
    for _ in range(pairs):
        for length in runs:
            step.accum = length
            runs[length].append(window(step, steps))
    step.accum = k
    after = (step.updates, int(step.step_dev))
    want = pairs * (steps + steps // k)
    assert after[0] - before[0] == after[1] - before[1] == want, (before, after, want)
    p, c = np.array(runs[1]), np.array(runs[k])
    for label, v in (('k = 1', p), ('k = %d' % k, c)):
        lines.append('%-8s mean %8.4f  min %8.4f  max %8.4f ms per micro-batch (%d windows of %d pipelined micro-batches)'
                     % (label, v.mean(), v.min(), v.max(), pairs, steps))
    diff = c.mean() - p.mean()
    spread = max(p.max() - p.min(), c.max() - c.min())
    every = bool(p.max() < c.min() or c.max() < p.min())
    lines.append('whole step: mean difference (k = %d - k = 1) %+.4f ms per micro-batch (%+.2f %%); largest same-path spread %.4f ms; ratio %.2f '
                 '(bar: 2); every run of one side beyond every run of the other: %s'
                 % (k, diff, 100 * diff / p.mean(), spread, abs(diff) / max(spread, 1e-12), every))
    lines.append('verdict by the bar set beforehand: a difference is %s' % ('ESTABLISHED' if abs(diff) >= 2 * spread and every else 'NOT ESTABLISHED'))
    if op_us is not None:
        lines.append('the op alone (same n) took %.2f us (FIRST), %.2f (ADD), %.2f (FIN)' % (op_us['FIRST'], op_us['ADD'], op_us['FIN']))
    lines.append('updates in the timed windows %d (= %d windows x (%d + %d)); loss of the last micro-batch %.6f; launches per micro-batch %r'
                 % (after[0] - before[0], pairs, steps, steps // k, step.losses()[2], step.launches_per_step()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--parts', default='lt')
    ap.add_argument('--accum', type=int, default=4, help='part t: micro-batches per update')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'accum_bench needs the GPU'
    lines = ['# accum_bench: pairs %d, launches %d, steps %d, accum %d; library %s; %s'
             % (a.pairs, a.launches, a.steps, a.accum, R.lib_sha16(), torch.cuda.get_device_name(0))]
    hg_us = None
    if 'l' in a.parts:
        lines.append('## (l) the op alone, every call between its own events')
        hg_us = op_alone(lines, 'hg4x128', 3287936, a.pairs, a.launches)
        op_alone(lines, 'HRNet-W32', 28536113, a.pairs, max(20, a.launches // 2))
        torch.cuda.empty_cache()
        lines.append('')
    if 't' in a.parts:
        lines.append('## (t) the whole step, benchmark pair: one step, its window length switched between 1 and %d' % a.accum)
        toggled_step(lines, a.pairs, a.steps, a.accum, hg_us)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
