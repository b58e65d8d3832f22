#!/usr/bin/env python
"""What the AdamW launch (utils.FusedAdamW, csrc/adamw.hip) costs, in ONE process and ONE call.

    python tools/adamw_bench.py [--pairs 6 --launches 100 --steps 40 --parts lt] [--out profiles/adamw_bench.txt]

(l) The op alone: fpd_adamw over flat arenas of the benchmark's hourglass student (3 287 936 elements) and of the HRNet-W32
    student (28 536 113) in four modes -- plain (no decay, no mask, no AMSGrad), decay, decay with the exemption mask (every
    third run of 1..64 elements exempt), AMSGrad -- with fpd_adam, the existing kernel, beside it at the same n.  Every call is
    timed on its own between two device events, the method of tools/accum_bench.py; `--pairs` interleaved rounds (every mode
    gets one window of `--launches` calls per round) after one untimed round.  The plain mode is judged against fpd_adam: it
    moves the same 28 bytes per element through 16-byte vectors where fpd_adam moves 4-byte elements, so it is expected not
    to be slower; FusedAdam is not rerouted either way.
(t) The whole step on the benchmark pair (hg4x128 bf16 student, hg8x256 bf16 teacher, batch 32, 256x256) on ONE FusedFPDStep
    built with a FusedAdamW (decay + mask): behind its plan one FPD_OP_ADAM is recorded over the same arenas, moments and
    schedule scalars, and the optimizer range is switched between the two one-op ranges -- FusedAdam's op and FusedAdamW's --
    in `--pairs` interleaved pairs of `--steps` pipelined steps between two device events, one untimed window each.  Same
    streams, same arenas, same plan: nothing but the op differs.  One instance, because two FusedFPDStep built side by side in
    one process are not a same-path comparison: the second one built runs slower whichever optimizer it holds.
    The two one-op ranges are also timed alone on the step's own arenas, every call between its own events.
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
from fpd_amd.lib.utils.utils import FusedAdamW  # noqa: E402

# name, weight_decay, mask, AMSGrad, bytes moved per element
MODES = (('plain', 0.0, False, False, 28.0), ('decay', 0.01, False, False, 28.0), ('decay+mask', 0.01, True, False, 28.125),
         ('amsgrad', 0.0, False, True, 36.0))


class AD(dict):
    __getattr__ = dict.__getitem__


def hg_cfg(feats, stacks, joints=16, dtype='bf16'):
    return AD(MODEL=AD(NUM_JOINTS=joints, DTYPE=dtype, EXTRA=AD(NUM_FEATURES=feats, NUM_STACKS=stacks, NUM_BLOCKS=1)))


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def window_us(call, launches):
    """Mean microseconds of call() over one window, each call between its own two events."""
    evs = []
    for _ in range(launches):
        e0, e1 = events()
        e0.record()
        call()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return float(np.mean([a.elapsed_time(b) for a, b in evs])) * 1e3


def verdict(lines, label, a_name, a, b_name, b):
    """b against a (the yardstick): the difference of the means against the largest same-path spread, bar 2."""
    diff = b.mean() - a.mean()
    spread = max(a.max() - a.min(), b.max() - b.min())
    every = bool(a.max() < b.min() or b.max() < a.min())
    est = abs(diff) >= 2 * spread and every
    lines.append('%s: mean difference (%s - %s) %+.4f (%+.2f %%); largest same-path spread %.4f; ratio %.2f (bar: 2); every run of one side '
                 'beyond every run of the other: %s' % (label, b_name, a_name, diff, 100 * diff / a.mean(), spread, abs(diff) / max(spread, 1e-12), every))
    lines.append('verdict by the bar set beforehand: a difference is %s%s'
                 % ('ESTABLISHED' if est else 'NOT ESTABLISHED', (' (%s is %s)' % (b_name, 'slower' if diff > 0 else 'faster')) if est else ''))
    return est, diff


def op_alone(lines, name, n, pairs, launches):
    lib, st, dev = R.lib(), R.current_stream(), torch.device('cuda:0')
    g = torch.randn(n, device=dev) * 1e-3
    p, m, v, x = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    lr_dev, step_dev = torch.full((1,), 1e-3, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    bits = np.zeros((n + 31) // 32 * 32, np.uint8)
    rng, i, k = np.random.RandomState(0), 0, 0
    while i < n:                                # runs of 1..64 elements, every third one exempt: boundaries inside vectors and words
        w = int(rng.randint(1, 65))
        if k % 3 == 0:
            bits[i:i + w] = 1
        i, k = i + w, k + 1
    mask = torch.from_numpy(np.packbits(bits, bitorder='little').view(np.int32).copy()).to(dev)

    def adamw_args(wd, with_mask, ams):
        a = R.AdamWT()
        a.n, a.param, a.grad, a.m, a.v, a.param_lp = n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None
        a.lr, a.beta1, a.beta2, a.eps, a.bias_corr1, a.bias_corr2, a.grad_scale = 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, 1.0
        a.lr_dev, a.step_dev = lr_dev.data_ptr(), step_dev.data_ptr()
        a.weight_decay, a.vmax, a.no_decay_bits = wd, (x.data_ptr() if ams else None), (mask.data_ptr() if with_mask else None)
        return a
    d = R.AdamT()
    d.n, d.param, d.grad, d.m, d.v, d.param_lp = n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None
    d.lr, d.beta1, d.beta2, d.eps, d.bias_corr1, d.bias_corr2, d.grad_scale = 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, 1.0
    d.lr_dev, d.step_dev = lr_dev.data_ptr(), step_dev.data_ptr()
    calls = [('fpd_adam', 28.0, lambda: R.check(lib.fpd_adam(d, st), 'fpd_adam'))]
    for label, wd, with_mask, ams, moved in MODES:
        a = adamw_args(wd, with_mask, ams)
        calls.append(('fpd_adamw ' + label, moved, (lambda a=a: R.check(lib.fpd_adamw(a, st), 'fpd_adamw'))))
    blocks, vec = R.C.c_int32(), R.C.c_int64()
    R.check(lib.fpd_adamw_geometry(adamw_args(0.0, False, False), blocks, vec), 'fpd_adamw_geometry')
    lines.append('%-10s n = %d (arenas of %.1f MB): fpd_adamw grid %d x 256, %d trip(s) over the %d-element vector part; fpd_adam grid %d x 256, '
                 '%d trip(s) over single elements' % (name, n, 4 * n / 1e6, blocks.value, -(-(vec.value // 4) // (blocks.value * 256)), vec.value,
                                                     min(4096, -(-n // 256)), -(-n // (min(4096, -(-n // 256)) * 256))))
    res = {c[0]: [] for c in calls}
    for r in range(pairs + 1):                  # interleaved rounds, the first one untimed
        for label, _, call in calls:
            us = window_us(call, launches)
            if r:
                res[label].append(us)
    assert all(bool(torch.isfinite(t).all()) for t in (p, m, v, x))
    res = {k: np.array(u) for k, u in res.items()}
    for label, moved, _ in calls:
        us = res[label]
        lines.append('%-10s %-22s %8.2f us per call (min %.2f max %.2f over %d windows of %d calls): %g B/element moved, %.2f TB/s'
                     % ('', label + ':', us.mean(), us.min(), us.max(), pairs, launches, moved, moved * n / us.mean() / 1e6))
    est, diff = verdict(lines, '%s, plain fpd_adamw against fpd_adam, us per call' % name, 'fpd_adam', res['fpd_adam'], 'fpd_adamw plain',
                        res['fpd_adamw plain'])
    if est and diff > 0:
        lines.append('the plain mode is established SLOWER than fpd_adam at this n; FusedAdam keeps fpd_adam either way')
    return res


def build_pair(x, tg, tw):
    """ONE FusedFPDStep with a FusedAdamW (decay + mask), and behind its plan one FPD_OP_ADAM over the same arenas, moments and
    schedule scalars: the optimizer range is switched between the two one-op ranges, nothing else differs."""
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
    opt = FusedAdamW(s, lr=2.5e-4, weight_decay=0.01, no_decay_norm_bias=True)
    step = E.FusedFPDStep(s.device_state(), s.cfg_hg, t.device_state(), t.cfg_hg, B, H, W, alpha=0.5, lr=2.5e-4, adam=opt)
    w = step._adamw_args
    d = R.AdamT()
    for name, _ in R.AdamT._fields_:
        setattr(d, name, getattr(w, name))
    plan = step.student.plan
    b = len(plan)
    plan.add(R.OP_ADAM, d)
    ranges = {'FusedAdam': (b, len(plan)), 'FusedAdamW': step.student.rng['adam']}
    step.set_batch(x, tg, tw)
    step.run_pipelined(2)
    return s, t, step, opt, ranges


def window(step, steps):
    e0, e1 = events()
    e0.record()
    step.run_pipelined(steps)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def toggled_step(lines, pairs, nsteps):
    x, tg, tw = synth.make_batch(1000, 32, 16, (256, 256), (64, 64))
    s, t, step, opt, ranges = build_pair(x, tg, tw)
    runs = {k: [] for k in ranges}
    for k in ranges:                          # run_pipelined ends with flush(): nothing is pending when the range changes
        step.student.rng['adam'] = ranges[k]
        window(step, nsteps)
    before = int(opt.step_dev)
    for _ in range(pairs):
        for k in ranges:
            step.student.rng['adam'] = ranges[k]
            runs[k].append(window(step, nsteps))
    step.student.rng['adam'] = ranges['FusedAdamW']
    assert int(opt.step_dev) - before == 2 * pairs * nsteps, (before, int(opt.step_dev))
    runs = {k: np.array(v) for k, v in runs.items()}
    for k, v in runs.items():
        b, e = ranges[k]
        lines.append('%-10s mean %8.4f  min %8.4f  max %8.4f ms per step (%d windows of %d pipelined steps); optimizer range: op types %r'
                     % (k, v.mean(), v.min(), v.max(), pairs, nsteps, [step.student.plan.op_type(i) for i in range(b, e)]))
    verdict(lines, 'whole step, ms per step', 'FusedAdam', runs['FusedAdam'], 'FusedAdamW (decay + mask)', runs['FusedAdamW'])
    lines.append('updates in the timed windows %d; loss of the last step %.6f; launches per step %r'
                 % (int(opt.step_dev) - before, step.losses()[2], step.launches_per_step()))
    # the two ranges alone on the step's own arenas (the gradient of the last step, with its exact zeros), every call between its own events
    alone = {k: [] for k in ranges}
    for r in range(pairs + 1):
        for k in ranges:
            b, e = ranges[k]
            us = window_us(lambda: step.student.plan.run(b, e, None), 50)
            if r:
                alone[k].append(us)
    for k, v in alone.items():
        v = np.array(v)
        lines.append('%-10s range alone on the step\'s arenas: %8.2f us per call (min %.2f max %.2f over %d windows of 50 calls)'
                     % (k, v.mean(), v.min(), v.max(), pairs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--parts', default='lt')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'adamw_bench needs the GPU'
    lines = ['# adamw_bench: pairs %d, launches %d, steps %d; library %s; %s'
             % (a.pairs, a.launches, a.steps, R.lib_sha16(), torch.cuda.get_device_name(0))]
    if 'l' in a.parts:
        lines.append('## (l) the op alone, every call between its own events, interleaved rounds')
        op_alone(lines, 'hg4x128', 3287936, a.pairs, a.launches)
        torch.cuda.empty_cache()
        op_alone(lines, 'HRNet-W32', 28536113, a.pairs, max(20, a.launches // 2))
        torch.cuda.empty_cache()
        lines.append('')
    if 't' in a.parts:
        lines.append('## (t) the whole step, benchmark pair: the optimizer switched between FusedAdam and FusedAdamW (decay + mask)')
        toggled_step(lines, a.pairs, a.steps)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
