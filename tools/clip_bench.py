#!/usr/bin/env python
"""What global gradient-norm clipping (utils.GradClipper, csrc/grad_clip.hip) costs, in ONE process and ONE call.

    python tools/clip_bench.py [--pairs 6 --launches 100 --steps 40 --parts lt --max-norm 1e-3] [--out profiles/clip_bench.txt]

(l) The op alone: fpd_grad_clip (sum of squares, finalise, scale) over a flat arena of the benchmark's hourglass student
    (3 287 936 elements) and of the HRNet-W32 student (28 536 113), in two states -- clipping (max_norm at half the norm: the
    scale launch reads and writes the arena) and not clipping (max_norm = inf: every thread of the scale launch leaves at
    once) -- beside fpd_adam at the same n.  A clipped arena would not clip a second time, so every call is timed on its own
    between two device events, with the arena refilled by a device copy in front of it, outside the timed span; the same
    method serves all three so that they compare.  `--pairs` windows of `--launches` calls after one untimed window.  The
    copy leaves the arena in the 256 MB Infinity Cache where it fits (13 MB does, 114 MB in part).
(t) The whole step on the benchmark pair (hg4x128 bf16 student, hg8x256 bf16 teacher, batch 32, 256x256) on ONE
    FusedFPDStep(clip=): the optimizer range is replayed with and without its first op (without it the range is the plan of
    before, op for op), `--pairs` interleaved pairs of `--steps` pipelined steps between two device events, one untimed
    window each.  Same streams, same arenas: nothing but the op differs.  `--max-norm` is the clipper's (the default clips).
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
from fpd_amd.lib.utils.utils import GradClipper  # noqa: E402


class AD(dict):
    __getattr__ = dict.__getitem__


def hg_cfg(feats, stacks, joints=16, dtype='bf16'):
    return AD(MODEL=AD(NUM_JOINTS=joints, DTYPE=dtype, EXTRA=AD(NUM_FEATURES=feats, NUM_STACKS=stacks, NUM_BLOCKS=1)))


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def per_call_us(call, refill, pairs, launches):
    """Mean microseconds of call() per window, each call between its own two events with refill() in front of it, untimed."""
    def window():
        evs = []
        for _ in range(launches):
            refill()
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
    g0 = torch.randn(n, device=dev) * 1e-3
    g = g0.clone()
    norm0 = float(g0.double().norm())
    nbytes = lib.fpd_grad_clip_scratch_bytes(n)
    partial = torch.zeros(nbytes // 8, dtype=torch.float64, device=dev)
    out, counters = torch.zeros(2, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
    a = R.GradClipT()
    a.n, a.grad, a.partial, a.partial_bytes, a.out, a.counters = n, g.data_ptr(), partial.data_ptr(), nbytes, out.data_ptr(), counters.data_ptr()
    blocks, vec = R.C.c_int32(), R.C.c_int64()
    a.max_norm = 1.0
    R.check(lib.fpd_grad_clip_geometry(a, blocks, vec), 'fpd_grad_clip_geometry')
    lines.append('%-10s n = %d (%.1f MB): grid %d x 256, %d trip(s) over the %d-element vector part, %d partials'
                 % (name, n, 4 * n / 1e6, blocks.value, -(-(vec.value // 4) // (blocks.value * 256)), vec.value, blocks.value))
    res = {}
    for label, max_norm, moved in (('clipping', 0.5 * norm0, 12), ('not clipping', float('inf'), 4)):
        a.max_norm = max_norm
        counters.zero_()
        us = per_call_us(lambda: R.check(lib.fpd_grad_clip(a, st), 'fpd_grad_clip'), lambda: g.copy_(g0), pairs, launches)
        c = counters.tolist()
        assert c[0] == (pairs + 1) * launches and c[1] == (c[0] if label == 'clipping' else 0) and c[2] == 0, c
        res[label] = us
        lines.append('%-10s fpd_grad_clip, %-12s %8.2f us per call (min %.2f max %.2f over %d windows of %d calls): %d B/element moved, %.2f TB/s'
                     % ('', label + ':', us.mean(), us.min(), us.max(), pairs, launches, moved, moved * n / us.mean() / 1e6))
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    lr_dev, step_dev = torch.full((1,), 1e-3, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    d = R.AdamT()
    d.n, d.param, d.grad, d.m, d.v, d.param_lp = n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None
    d.lr, d.beta1, d.beta2, d.eps, d.bias_corr1, d.bias_corr2, d.grad_scale = 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, 1.0
    d.lr_dev, d.step_dev = lr_dev.data_ptr(), step_dev.data_ptr()
    us = per_call_us(lambda: R.check(lib.fpd_adam(d, st), 'fpd_adam'), lambda: g.copy_(g0), pairs, launches)
    lines.append('%-10s fpd_adam beside it:        %8.2f us per call (min %.2f max %.2f): 28 B/element moved, %.2f TB/s'
                 % ('', us.mean(), us.min(), us.max(), 28 * n / us.mean() / 1e6))
    return float(res['clipping'].mean())


def build_pair(x, tg, tw, max_norm):
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
    clip = GradClipper(s, max_norm)
    step = E.FusedFPDStep(s.device_state(), s.cfg_hg, t.device_state(), t.cfg_hg, B, H, W, alpha=0.5, lr=2.5e-4, clip=clip)
    step.set_batch(x, tg, tw)
    step.run_pipelined(3)
    return s, t, clip, step


def window(step, steps):
    e0, e1 = events()
    e0.record()
    step.run_pipelined(steps)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def toggled_step(lines, pairs, steps, op_us, max_norm):
    x, tg, tw = synth.make_batch(1000, 32, 16, (256, 256), (64, 64))
    s, t, clip, step = build_pair(x, tg, tw, max_norm)
    b, e = step.student.rng['adam']
    assert e - b == 2 and step.student.plan.op_type(b) == R.OP_GRAD_CLIP
    ranges = {'plain': (b + 1, e), 'clip': (b, e)}
    runs = {k: [] for k in ranges}
    for k, r in ranges.items():
        step.student.rng['adam'] = r
        window(step, steps)
    before = clip.stats()
    for _ in range(pairs):
        for k, r in ranges.items():
            step.student.rng['adam'] = r
            runs[k].append(window(step, steps))
    step.student.rng['adam'] = (b, e)
    after = clip.stats()
    p, c = np.array(runs['plain']), np.array(runs['clip'])
    for k, v in (('without clip=', p), ('with clip=', c)):
        lines.append('%-14s mean %8.4f  min %8.4f  max %8.4f ms per step (%d windows of %d pipelined steps)' % (k, v.mean(), v.min(), v.max(), pairs, steps))
    diff = c.mean() - p.mean()
    spread = max(p.max() - p.min(), c.max() - c.min())
    every = bool(p.max() < c.min() or c.max() < p.min())
    lines.append('whole step: mean difference (clip - plain) %+.4f ms (%+.2f %%); largest same-path spread %.4f ms; ratio %.2f (bar: 2); every run of '
                 'one side beyond every run of the other: %s' % (diff, 100 * diff / p.mean(), spread, abs(diff) / max(spread, 1e-12), every))
    lines.append('verdict by the bar set beforehand: a difference is %s' % ('ESTABLISHED' if abs(diff) >= 2 * spread and every else 'NOT ESTABLISHED'))
    if op_us is not None:
        lines.append('the op alone (clipping, same n) took %.2f us' % op_us)
    lines.append('max_norm %g: calls in the timed windows %d (= %d windows x %d steps), clipped %d, non-finite %d; last norm %.6g, coef %.6g; launches per step %r'
                 % (max_norm, after['calls'] - before['calls'], pairs, steps, after['clipped'] - before['clipped'],
                    after['nonfinite'] - before['nonfinite'], clip.norm(), clip.coef(), step.launches_per_step()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--parts', default='lt')
    ap.add_argument('--max-norm', type=float, default=1e-3, help='part t: the clipper\'s max_norm (inf: measure only)')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'clip_bench needs the GPU'
    lines = ['# clip_bench: pairs %d, launches %d, steps %d; library %s; %s' % (a.pairs, a.launches, a.steps, R.lib_sha16(), torch.cuda.get_device_name(0))]
    hg_us = None
    if 'l' in a.parts:
        lines.append('## (l) the op alone, every call between its own events, the arena refilled in front of it')
        hg_us = op_alone(lines, 'hg4x128', 3287936, a.pairs, a.launches)
        op_alone(lines, 'HRNet-W32', 28536113, a.pairs, max(20, a.launches // 2))
        torch.cuda.empty_cache()
        lines.append('')
    if 't' in a.parts:
        lines.append('## (t) the whole step, benchmark pair: one step, its optimizer range with and without the op')
        toggled_step(lines, a.pairs, a.steps, hg_us, a.max_norm)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
