#!/usr/bin/env python
"""What the DARK decode costs: the launch alone against fpd_final_preds, and one whole validation with TEST.DARK on
against off, in ONE process and ONE call.

    python tools/dark_bench.py [--samples 2048 --batch 32 --pairs 6 --ksize 11] [--out profiles/dark_bench.txt]

The launch: fpd_dark_refine (NHWC, as the validation step calls it, and NCHW, as get_final_preds does) and
fpd_final_preds with the quarter-pixel shift at 32x16x64x64 on Gaussian peaks with noise, `--reps` windows of `--launches`
back-to-back launches each between two device events, after a warm-up of one window.

The validation: tools/validate_bench.py's setting (synthetic_aug validation scenes, the hg4x128 bf16 student, flip test
on), core.function.validate with TEST.DARK on against off, one untimed run each, then `--pairs` interleaved pairs, every
run a host clock around the call, which ends with the results on the host.  That tool's rule decides: a difference is
ESTABLISHED only if the mean difference is at least twice the largest same-path spread and every run of one setting beats
every run of the other."""
import argparse
import logging
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fpd_amd import runtime as R  # noqa: E402
from fpd_amd.lib import models  # noqa: E402,F401
from fpd_amd.lib.config import _defaults  # noqa: E402
from fpd_amd.lib.core import function as F  # noqa: E402
from fpd_amd.lib.core.inference import dark_taps_device  # noqa: E402
from fpd_amd.lib.core.loss import JointsMSELoss  # noqa: E402
from fpd_amd.lib.dataset.device_dataset import synthetic_aug  # noqa: E402


def peak_maps(n, j, h, w, seed=0):
    """[n,j,h,w] float32: one Gaussian peak of sigma 2 per map at a sub-pixel position away from the border, plus noise."""
    g = torch.Generator().manual_seed(seed)
    mx = 2.5 + torch.rand(n, j, 1, 1, generator=g, dtype=torch.float64) * (w - 6)
    my = 2.5 + torch.rand(n, j, 1, 1, generator=g, dtype=torch.float64) * (h - 6)
    amp = 0.3 + 0.7 * torch.rand(n, j, 1, 1, generator=g, dtype=torch.float64)
    y = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1)
    x = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w)
    m = amp * torch.exp(-((x - mx) ** 2 + (y - my) ** 2) / 8.0) + 0.01 * torch.randn(n, j, h, w, generator=g, dtype=torch.float64)
    return m.float()


def time_launches(call, launches, reps):
    """ms per launch over `reps` windows of `launches` launches between two device events; one untimed window first."""
    out = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        e1.synchronize()
        if r:
            out.append(e0.elapsed_time(e1) / launches)
    return np.array(out)


def launch_alone(a, lines):
    n, j, h, w = 32, 16, 64, 64
    lib, st = R.lib(), R.current_stream()
    nchw = peak_maps(n, j, h, w).cuda()
    nhwc = nchw.permute(0, 2, 3, 1).contiguous()
    taps = dark_taps_device(a.ksize, nchw.device)
    coords = torch.empty((n, j, 2), dtype=torch.float32, device='cuda')
    maxvals = torch.empty((n, j), dtype=torch.float32, device='cuda')
    refined = torch.zeros((n, j), dtype=torch.int32, device='cuda')
    res = {}
    for name, hm, layout in (('fpd_dark_refine NHWC', nhwc, R.DARK_NHWC), ('fpd_dark_refine NCHW', nchw, R.DARK_NCHW)):
        d = R.DarkT()
        d.N, d.J, d.H, d.W, d.layout, d.ksize = n, j, h, w, layout, a.ksize
        d.hm, d.taps, d.coords, d.maxvals, d.refined = hm.data_ptr(), taps.data_ptr(), coords.data_ptr(), maxvals.data_ptr(), refined.data_ptr()
        res[name] = time_launches(lambda d=d: R.check(lib.fpd_dark_refine(d, st), 'fpd_dark_refine'), a.launches, a.reps)
        assert int(refined.sum()) == n * j, 'the benchmark maps are meant to be refined, every one'
    f = R.FinalPredsT()
    f.N, f.J, f.H, f.W, f.post_process = n, j, h, w, 1
    f.hm, f.coords, f.maxvals = nchw.data_ptr(), coords.data_ptr(), maxvals.data_ptr()
    res['fpd_final_preds NCHW'] = time_launches(lambda: R.check(lib.fpd_final_preds(f, st), 'fpd_final_preds'), a.launches, a.reps)
    lines.append('The launch alone at %dx%dx%dx%d, k = %d (every map refined): %d windows of %d back-to-back launches between device '
                 'events, one untimed window first; microseconds per launch.' % (n, j, h, w, a.ksize, a.reps, a.launches))
    for name, v in res.items():
        lines.append('%-22s median %8.2f  min %8.2f  max %8.2f us' % (name, np.median(v) * 1e3, v.min() * 1e3, v.max() * 1e3))
    lines.append('')
    return {k: float(np.median(v)) for k, v in res.items()}


def whole_validation(a, lines):
    cfgs = {}
    for name, dark in (('dark off', False), ('dark on', True)):
        cfg = _defaults()
        cfg.DATASET.DATASET, cfg.DATASET.NUM_VALID_SAMPLES, cfg.TEST.BATCH_SIZE_PER_GPU = 'synthetic_aug', a.samples, a.batch
        cfg.MODEL.DTYPE, cfg.MODEL.EXTRA.NUM_FEATURES, cfg.MODEL.EXTRA.NUM_STACKS = 'bf16', 128, 4
        cfg.TEST.FLIP_TEST = cfg.TEST.SHIFT_HEATMAP = cfg.TEST.POST_PROCESS = True
        cfg.TEST.DARK, cfg.TEST.BLUR_KERNEL = dark, a.ksize
        cfgs[name] = cfg
    torch.manual_seed(1)
    cfg0 = cfgs['dark off']
    model = models.hourglass.get_pose_net(cfg0, is_train=False).cuda().eval()
    crit = JointsMSELoss(True).cuda()
    _, loader, db = synthetic_aug(cfg0, 'cuda', train=False)
    out_dir = tempfile.mkdtemp()
    times = {k: [] for k in cfgs}
    last = {}
    lines.append('One validation of %d synthetic_aug samples, batch %d (%d batches, two forwards each: flip test on), hg4x128 bf16 '
                 'student, core.function.validate with TEST.DARK off against on (k = %d), one process, one call: one untimed run '
                 'each, then %d interleaved pairs.' % (a.samples, a.batch, len(loader), a.ksize, a.pairs))
    lines.append('')

    def run(name, tag):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        F.validate(cfgs[name], loader, db, model, crit, out_dir, out_dir)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        last[name] = F.validate.last
        lines.append('%-9s %8.1f ms  %7.3f ms/batch  %8.1f samples/s  %s' % (name, dt * 1e3, dt * 1e3 / len(loader), a.samples / dt, tag))
        print(lines[-1], flush=True)
        return dt
    for name in cfgs:
        run(name, 'untimed')
    for k in range(a.pairs):
        for name in cfgs:
            times[name].append(run(name, 'pair%d' % (k + 1)))
    lines.append('')
    ms = {k: np.array(v) * 1e3 for k, v in times.items()}
    for k, v in ms.items():
        lines.append('%-9s mean %8.1f  min %8.1f  max %8.1f ms' % (k, v.mean(), v.min(), v.max()))
    diff = ms['dark on'].mean() - ms['dark off'].mean()
    spread = max(v.max() - v.min() for v in ms.values())
    every = bool(ms['dark off'].max() < ms['dark on'].min())
    lines.append('mean difference (on - off) %.1f ms (%.2f %% of a validation, %.1f us per batch); largest same-path spread of the '
                 'call %.1f ms; ratio %.2f (bar: 2)' % (diff, 100 * diff / ms['dark off'].mean(), diff * 1e3 / len(loader), spread,
                                                          diff / max(spread, 1e-9)))
    lines.append('every run without DARK faster than every run with it: %s' % every)
    lines.append('verdict by the bar set beforehand (mean difference >= 2 x largest same-path spread, and every run of one setting '
                 'beats every run of the other): a cost of DARK is %s' % ('ESTABLISHED' if diff >= 2 * spread and every else 'NOT ESTABLISHED'))
    x, y = last['dark on'], last['dark off']
    moved = np.abs(x['all_preds'][:, :, 0:2].astype(np.float64) - y['all_preds'][:, :, 0:2]).max(-1)
    lines.append('max values and boxes of the two settings bit-equal: %s; coordinate difference in image pixels: median %.3f, '
                 'largest %.1f (the student is untrained: its maps are noise, and on a map without a Gaussian peak the Newton '
                 'step is as unbounded as in the published decode)'
                 % (x['all_preds'][:, :, 2].tobytes() == y['all_preds'][:, :, 2].tobytes() and x['all_boxes'].tobytes() == y['all_boxes'].tobytes(),
                    float(np.median(moved)), float(moved.max())))
    return diff, spread, len(loader)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=2048)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--ksize', type=int, default=11)
    ap.add_argument('--launches', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dark_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'dark_bench needs the GPU'
    logging.basicConfig(level=logging.WARNING)
    lines = []
    launch_alone(a, lines)
    print('\n'.join(lines), flush=True)
    mark = len(lines)
    whole_validation(a, lines)
    print('\n'.join(lines[mark:][-6:]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
