#!/usr/bin/env python
"""What DEBUG.DEBUG costs the training loop: epochs of core.function.fpd_train on the benchmark pair (hg4x128 <- hg8x256,
batch 32, bf16, DATASET synthetic_aug) in ONE process and ONE call, alternating

    off     DEBUG.DEBUG false
    async   all four SAVE_* flags at PRINT_FREQ 100, canvases handed to the AsyncImageWriter (the loops' default)
    sync    the same with the writer forced synchronous (download, encode and write inside the loop)

    python tools/vis_bench.py [--iters 200 --repeats 5 --print-freq 100] [--out profiles/vis_bench.txt]

One untimed epoch of each, then `repeats` interleaved rounds; every epoch is a host clock around the call, which returns with
the device idle and the files written.  Also reported: the device time of one debug iteration's launches (device events,
behind a plug of queued matmuls so that the interval holds kernel time), the bytes it downloads, and the host time of one
JPEG encode per canvas.  The asynchronous writer counts as ESTABLISHED against the synchronous one only if the mean
difference exceeds twice the largest same-path spread of the call (the rule of profiles/validate_bench.txt)."""
import argparse
import itertools
import logging
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fpd_amd.lib import models  # noqa: E402,F401
from fpd_amd.lib.config import _defaults  # noqa: E402
from fpd_amd.lib.core import function as F  # noqa: E402
from fpd_amd.lib.core.loss import JointsMSELoss  # noqa: E402
from fpd_amd.lib.dataset.device_dataset import synthetic_aug  # noqa: E402
from fpd_amd.lib.utils import vis  # noqa: E402
from fpd_amd.lib.utils.utils import FusedAdam  # noqa: E402


class Epoch(object):
    """`iters` batches: the loader's own (short) epochs one after another."""

    def __init__(self, loader, iters):
        self.loader, self.iters = loader, iters

    def __iter__(self):
        return itertools.islice(itertools.chain.from_iterable(iter(self.loader) for _ in itertools.count()), self.iters)

    def __len__(self):
        return self.iters


def config(debug, print_freq, batch):
    cfg = _defaults()
    cfg.DATASET.DATASET, cfg.DATASET.NUM_SCENES, cfg.DATASET.NUM_VALID_SAMPLES = 'synthetic_aug', 2 * batch, batch
    cfg.TRAIN.BATCH_SIZE_PER_GPU, cfg.PRINT_FREQ = batch, print_freq
    cfg.MODEL.DTYPE, cfg.MODEL.EXTRA.NUM_FEATURES, cfg.MODEL.EXTRA.NUM_STACKS = 'bf16', 128, 4
    d = cfg.DEBUG
    d.DEBUG = d.SAVE_BATCH_IMAGES_GT = d.SAVE_BATCH_IMAGES_PRED = d.SAVE_HEATMAPS_GT = d.SAVE_HEATMAPS_PRED = bool(debug)
    return cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--print-freq', type=int, default=100)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vis_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'vis_bench needs the GPU'
    logging.basicConfig(level=logging.WARNING)
    cfgs = {'off': config(False, a.print_freq, a.batch), 'async': config(True, a.print_freq, a.batch), 'sync': config(True, a.print_freq, a.batch)}
    tcfg = config(False, a.print_freq, a.batch)
    tcfg.MODEL.EXTRA.NUM_FEATURES, tcfg.MODEL.EXTRA.NUM_STACKS = 256, 8
    torch.manual_seed(1)
    student = models.hourglass.get_pose_net(cfgs['off'], is_train=True).cuda()
    torch.manual_seed(2)
    teacher = models.hourglass.get_pose_net(tcfg, is_train=False).cuda()
    crit = JointsMSELoss(True).cuda()
    opt = FusedAdam(student, lr=2.5e-4)
    loader, _, _ = synthetic_aug(cfgs['off'], 'cuda')
    epoch = Epoch(loader, a.iters)
    out_dir = tempfile.mkdtemp()
    debug_iters = len(range(0, a.iters, a.print_freq))
    lines = ['Epochs of %d iterations of core.function.fpd_train, hg4x128 <- hg8x256, batch %d, bf16, synthetic_aug, PRINT_FREQ %d '
             '(%d debug iterations per epoch, four canvases each), one process, one call: one untimed epoch of each path, then %d '
             'interleaved rounds.' % (a.iters, a.batch, a.print_freq, debug_iters, a.repeats), '']

    def run(name, tag):
        F.DEBUG_WRITER_ASYNC = name != 'sync'
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        F.fpd_train(cfgs[name], epoch, student, teacher, crit, crit, opt, 0, out_dir, out_dir, None)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lines.append('%-6s %9.1f ms  %7.3f ms/iteration  %8.1f images/s  %s' % (name, dt * 1e3, dt * 1e3 / a.iters, a.iters * a.batch / dt, tag))
        print(lines[-1], flush=True)
        return dt
    times = {k: [] for k in cfgs}
    try:
        for name in cfgs:
            run(name, 'untimed')
        for k in range(a.repeats):
            for name in cfgs:
                times[name].append(run(name, 'round%d' % (k + 1)))
    finally:
        F.DEBUG_WRITER_ASYNC = True
    lines.append('')
    ms = {k: np.array(v) * 1e3 for k, v in times.items()}
    for k, v in ms.items():
        lines.append('%-6s mean %9.1f  min %9.1f  max %9.1f ms   %8.1f images/s' % (k, v.mean(), v.min(), v.max(), a.iters * a.batch / (v.mean() * 1e-3)))
    spread = max(v.max() - v.min() for v in ms.values())
    for x, y in (('async', 'off'), ('sync', 'off'), ('sync', 'async')):
        diff = ms[x].mean() - ms[y].mean()
        lines.append('%s - %s: mean difference %.1f ms per epoch (%.2f %%), %.2f ms per debug iteration; largest same-path spread of the call '
                     '%.1f ms; ratio %.2f (bar: 2)' % (x, y, diff, 100 * diff / ms[y].mean(), diff / debug_iters, spread, abs(diff) / max(spread, 1e-9)))
    gain = ms['sync'].mean() - ms['async'].mean()
    lines.append('asynchronous writer against the synchronous one, by the bar set beforehand (mean difference > 2 x largest same-path '
                 'spread): %s' % ('ESTABLISHED' if gain > 2 * spread else 'NOT ESTABLISHED'))

    # one debug iteration taken apart, on a batch of the loader and the student's own last map
    inp, target, _, meta = next(iter(loader))
    step = F.fused_step_for(student, teacher, opt, inp.shape, float(cfgs['off'].KD.ALPHA), 1, (True, True))
    output = step.student.output_view(-1).permute(0, 3, 1, 2)
    plug = torch.randn(4096, 4096, device='cuda')

    def render():
        mm = vis.image_minmax(inp)
        preds = vis.max_preds(output)[0]
        return [vis.render_image_with_joints(inp, meta['joints'], meta['joints_vis'], minmax=mm),
                vis.render_image_with_joints(inp, preds, meta['joints_vis'], coord_scale=4.0, minmax=mm),
                vis.render_heatmaps(inp, target, minmax=mm), vis.render_heatmaps(inp, output, minmax=mm, preds=preds)]
    render()
    dev_ms = []
    for _ in range(7):
        torch.cuda.synchronize()
        for _ in range(16):
            plug @ plug
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        canvases = render()
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    host = [c.cpu().numpy() for c in canvases]
    enc = []
    for c in host:
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            vis.write_jpeg(os.path.join(out_dir, 'enc.jpg'), c)
            t.append((time.perf_counter() - t0) * 1e3)
        enc.append(statistics.median(t))
    lines.append('')
    lines.append('one debug iteration: device time of its launches (min/max, max_preds of the output, two joint grids, two heat-map '
                 'grids) median %.3f ms (min %.3f, max %.3f over 7); canvases %s = %d bytes downloaded'
                 % (statistics.median(dev_ms), min(dev_ms), max(dev_ms), ', '.join('x'.join(str(v) for v in c.shape) for c in host),
                    sum(c.size for c in host)))
    lines.append('host time of one JPEG encode + write (PIL, quality 95), median of 5: %s ms; all four %.1f ms'
                 % (', '.join('%.1f' % v for v in enc), sum(enc)))
    print('\n'.join(lines[-9:]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
