#!/usr/bin/env python
"""What the weight average (utils.ModelEma, csrc/ema.hip) costs, in ONE process and ONE call.

    python tools/ema_bench.py [--pairs 6 --launches 300 --steps 40 --parts lts --order ema,plain] [--out profiles/ema_bench.txt]

(l) The launch alone: fpd_ema (the streaming kernel + the counter's tick) over the parameter and running-statistics arenas of
    the benchmark's hourglass student (hg4x128) and of the HRNet-W32 student, `--pairs` windows of `--launches` back-to-back
    calls each between two device events, after one untimed window.  Reported: microseconds per call and the achieved bytes/s
    against the bytes the kernel must move (source and average read, average written: 12 bytes per element).  The hourglass
    arenas (about 40 MB) stay in the 256 MB Infinity Cache between back-to-back calls, so that figure is a cache-resident one;
    the HRNet arenas (about 340 MB) do not fit and stream from HBM.
(t) The whole step on the benchmark pair (hg4x128 bf16 student, hg8x256 bf16 teacher, batch 32, 256x256) with and without
    the average, on ONE FusedFPDStep(ema=): the optimizer range is replayed with and without its last op (without it the range
    is the plan of before, op for op), `--pairs` interleaved pairs of `--steps` pipelined steps between two device events,
    one untimed window each.  Same streams, same arenas: nothing but the op differs.
(s) The same comparison between TWO steps built in one process, one with ema= and one without, in the order `--order`
    gives.  Each step owns its lane streams, and the hardware queue a stream lands on depends on how many were created
    before it: this part shows what the build order alone does to a step, which (t) is free of.
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
from fpd_amd.lib.config import _wrap  # noqa: E402
from fpd_amd.lib.models import hourglass, pose_hrnet  # noqa: E402
from fpd_amd.lib.utils.utils import ModelEma  # noqa: E402


class AD(dict):
    __getattr__ = dict.__getitem__


def hg_cfg(feats, stacks, joints=16, dtype='bf16'):
    return AD(MODEL=AD(NUM_JOINTS=joints, DTYPE=dtype, EXTRA=AD(NUM_FEATURES=feats, NUM_STACKS=stacks, NUM_BLOCKS=1)))


def w32_cfg():
    st = lambda n, m: dict(NUM_MODULES=m, NUM_BRANCHES=n, BLOCK='BASIC', NUM_BLOCKS=[4] * n, NUM_CHANNELS=[32, 64, 128, 256][:n], FUSE_METHOD='SUM')
    extra = {'FINAL_CONV_KERNEL': 1, 'PRETRAINED_LAYERS': ['*'], 'STAGE2': st(2, 1), 'STAGE3': st(3, 4), 'STAGE4': st(4, 3)}
    return _wrap({'MODEL': {'NAME': 'pose_hrnet', 'NUM_JOINTS': 17, 'INIT_WEIGHTS': False, 'PRETRAINED': '', 'DTYPE': 'bf16', 'EXTRA': extra}})


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def launch_alone(lines, name, model, pairs, launches):
    ema = ModelEma(model)
    a = ema.ema_args()
    lib, st = R.lib(), R.current_stream()
    blocks, vec = R.C.c_int32(), (R.C.c_int64 * R.EMA_MAX_SEG)()
    R.check(lib.fpd_ema_geometry(a, blocks, vec), 'fpd_ema_geometry')
    n = a.seg[0].n + a.seg[1].n
    need = 12 * n + 16 * a.copy_n

    def window():
        e0, e1 = events()
        e0.record()
        for _ in range(launches):
            R.check(lib.fpd_ema(a, st), 'fpd_ema')
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches
    window()
    us = np.array([window() for _ in range(pairs)])
    trips = -(-max(vec[0], vec[1]) // 4 // (blocks.value * 256))
    lines.append('%-14s param %d + running statistics %d elements, %d copied integers; grid %d x 256, %d trip(s) over the vectors; %.1f MB to move'
                 % (name, a.seg[0].n, a.seg[1].n, a.copy_n, blocks.value, trips, need / 1e6))
    lines.append('%-14s fpd_ema (kernel + tick) %.2f us per call (min %.2f max %.2f over %d windows of %d calls): %.2f TB/s of the 12 B/element'
                 % ('', us.mean(), us.min(), us.max(), pairs, launches, need / us.mean() / 1e6))
    return float(us.mean()), float(us.max() - us.min())


def build_pair(kind, x, tg, tw):
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
    ema = ModelEma(s) if kind == 'ema' else None
    step = E.FusedFPDStep(s.device_state(), s.cfg_hg, t.device_state(), t.cfg_hg, B, H, W, alpha=0.5, lr=2.5e-4, ema=ema)
    step.set_batch(x, tg, tw)
    step.run_pipelined(3)
    return s, t, ema, step


def window(step, steps):
    e0, e1 = events()
    e0.record()
    step.run_pipelined(steps)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def report(lines, runs, pairs, steps, launch_us):
    a, b = np.array(runs['plain']), np.array(runs['ema'])
    for k, v in (('without ema=', a), ('with ema=', b)):
        lines.append('%-14s mean %8.4f  min %8.4f  max %8.4f ms per step (%d windows of %d pipelined steps)' % (k, v.mean(), v.min(), v.max(), pairs, steps))
    diff = b.mean() - a.mean()
    spread = max(a.max() - a.min(), b.max() - b.min())
    every = bool(a.max() < b.min() or b.max() < a.min())
    lines.append('whole step: mean difference (ema - plain) %+.4f ms (%+.2f %%); largest same-path spread %.4f ms; ratio %.2f (bar: 2); every run of '
                 'one side beyond every run of the other: %s' % (diff, 100 * diff / a.mean(), spread, abs(diff) / max(spread, 1e-12), every))
    lines.append('verdict by the bar set beforehand: a difference is %s' % ('ESTABLISHED' if abs(diff) >= 2 * spread and every else 'NOT ESTABLISHED'))
    if launch_us is not None:
        over = diff * 1e3 - launch_us
        lines.append('the launch alone took %.2f us: the step grew by %+.2f us more than that; the spread is %.2f us -> %s'
                     % (launch_us, over, spread * 1e3, 'INVESTIGATE: more than the launch and the spread explain' if over > spread * 1e3 else
                        'nothing beyond the launch itself shows'))


def toggled_step(lines, pairs, steps, launch_us):
    x, tg, tw = synth.make_batch(1000, 32, 16, (256, 256), (64, 64))
    s, t, ema, step = build_pair('ema', x, tg, tw)
    b, e = step.student.rng['adam']
    assert e - b == 2 and step.student.plan.op_type(e - 1) == R.OP_EMA
    ranges = {'plain': (b, e - 1), 'ema': (b, e)}
    runs = {k: [] for k in ranges}
    for k, r in ranges.items():
        step.student.rng['adam'] = r
        window(step, steps)
    before = ema.updates
    for _ in range(pairs):
        for k, r in ranges.items():
            step.student.rng['adam'] = r
            runs[k].append(window(step, steps))
    step.student.rng['adam'] = (b, e)
    report(lines, runs, pairs, steps, launch_us)
    lines.append('updates counted by the average in the timed windows: %d (= %d windows x %d steps); launches per step %r'
                 % (ema.updates - before, pairs, steps, step.launches_per_step()))


def two_steps(lines, pairs, steps, launch_us, order):
    x, tg, tw = synth.make_batch(1000, 32, 16, (256, 256), (64, 64))
    built = {kind: build_pair(kind, x, tg, tw) for kind in order}
    torch.cuda.synchronize()
    runs = {kind: [] for kind in ('plain', 'ema')}
    for kind in runs:
        window(built[kind][3], steps)
    for _ in range(pairs):
        for kind in runs:
            runs[kind].append(window(built[kind][3], steps))
    lines.append('built in the order: %s' % ', '.join(order))
    report(lines, runs, pairs, steps, launch_us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--launches', type=int, default=300)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--parts', default='lts')
    ap.add_argument('--order', default='ema,plain', help="part s: which of the two steps is built first")
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'ema_bench needs the GPU'
    dev = torch.device('cuda:0')
    lines = ['# ema_bench: pairs %d, launches %d, steps %d; library %s; %s' % (a.pairs, a.launches, a.steps, R.lib_sha16(), torch.cuda.get_device_name(0))]
    hg_us = None
    if 'l' in a.parts:
        lines.append('## (l) the launch alone')
        hg_us, _ = launch_alone(lines, 'hg4x128', hourglass.get_pose_net(hg_cfg(128, 4), is_train=True).to(dev), a.pairs, a.launches)
        launch_alone(lines, 'HRNet-W32', pose_hrnet.get_pose_net(w32_cfg(), is_train=True).to(dev), a.pairs, max(20, a.launches // 5))
        torch.cuda.empty_cache()
        lines.append('')
    if 't' in a.parts:
        lines.append('## (t) the whole step, benchmark pair: one step, its optimizer range with and without the op')
        toggled_step(lines, a.pairs, a.steps, hg_us)
        torch.cuda.empty_cache()
        lines.append('')
    if 's' in a.parts:
        lines.append('## (s) the whole step, benchmark pair: two steps in one process')
        two_steps(lines, a.pairs, a.steps, hg_us, a.order.split(','))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
