#!/usr/bin/env python
"""Times one whole validation of the benchmark student through core.function.validate (the fused step: enqueued work only,
device-resident results) against core.function._validate_per_batch (the per-batch body it replaces: host affine loop,
layout round trips, four host synchronisations per batch), in ONE process and ONE call.

    python tools/validate_bench.py [--samples 2048 --batch 32 --pairs 6] [--out profiles/validate_bench.txt]

DATASET 'synthetic_aug' validation scenes, the hg4x128 bf16 student of bench.py, TEST.FLIP_TEST / SHIFT_HEATMAP /
POST_PROCESS on.  One untimed run of each path, then `pairs` interleaved pairs; every run is a host clock around the call,
which ends with the results on the host.  The rule of profiles/bneck_upadd_ab.txt decides: the gain is ESTABLISHED only if
the mean difference is at least twice the largest same-path spread and every fused run beats every per-batch run.  Both
paths' result arrays are compared to the bit at the end."""
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

from fpd_amd.lib import models  # noqa: E402,F401
from fpd_amd.lib.config import _defaults  # noqa: E402
from fpd_amd.lib.core import function as F  # noqa: E402
from fpd_amd.lib.core.loss import JointsMSELoss  # noqa: E402
from fpd_amd.lib.dataset.device_dataset import synthetic_aug  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=2048)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'validate_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'validate_bench needs the GPU'
    logging.basicConfig(level=logging.WARNING)
    cfg = _defaults()
    cfg.DATASET.DATASET, cfg.DATASET.NUM_VALID_SAMPLES, cfg.TEST.BATCH_SIZE_PER_GPU = 'synthetic_aug', a.samples, a.batch
    cfg.MODEL.DTYPE, cfg.MODEL.EXTRA.NUM_FEATURES, cfg.MODEL.EXTRA.NUM_STACKS = 'bf16', 128, 4
    cfg.TEST.FLIP_TEST = cfg.TEST.SHIFT_HEATMAP = cfg.TEST.POST_PROCESS = True
    torch.manual_seed(1)
    model = models.hourglass.get_pose_net(cfg, is_train=False).cuda().eval()
    crit = JointsMSELoss(True).cuda()
    _, loader, db = synthetic_aug(cfg, 'cuda', train=False)
    out_dir = tempfile.mkdtemp()
    paths = {'per-batch': F._validate_per_batch, 'fused': F.validate}
    times = {k: [] for k in paths}
    lines = ['One validation of %d synthetic_aug samples, batch %d (%d batches, two forwards each: flip test on), hg4x128 bf16 '
             'student, one process, one call: core.function._validate_per_batch against core.function.validate, one untimed '
             'run each, then %d interleaved pairs.' % (a.samples, a.batch, len(loader), a.pairs), '']

    def run(name, tag):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        paths[name](cfg, loader, db, model, crit, out_dir, out_dir)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lines.append('%-9s %8.1f ms  %7.3f ms/batch  %8.1f samples/s  %s' % (name, dt * 1e3, dt * 1e3 / len(loader), a.samples / dt, tag))
        print(lines[-1], flush=True)
        return dt
    for name in paths:
        run(name, 'untimed')
    for k in range(a.pairs):
        for name in paths:
            times[name].append(run(name, 'pair%d' % (k + 1)))
    lines.append('')
    ms = {k: np.array(v) * 1e3 for k, v in times.items()}
    for k, v in ms.items():
        lines.append('%-9s mean %8.1f  min %8.1f  max %8.1f ms' % (k, v.mean(), v.min(), v.max()))
    diff = ms['per-batch'].mean() - ms['fused'].mean()
    spread = max(v.max() - v.min() for v in ms.values())
    every = bool(ms['fused'].max() < ms['per-batch'].min())
    lines.append('mean difference %.1f ms (%.1f %%, %.2fx); largest same-path spread of the call %.1f ms; ratio %.2f (bar: 2)'
                 % (diff, 100 * diff / ms['per-batch'].mean(), ms['per-batch'].mean() / ms['fused'].mean(), spread, diff / max(spread, 1e-9)))
    lines.append('every fused run faster than every per-batch run: %s' % every)
    lines.append('verdict by the bar set beforehand (mean difference >= 2 x largest same-path spread, and every fused run '
                 'beats every per-batch run): %s' % ('ESTABLISHED' if diff >= 2 * spread and every else 'NOT ESTABLISHED'))
    x, y = F.validate.last, F._validate_per_batch.last
    same = x['all_preds'].tobytes() == y['all_preds'].tobytes() and x['all_boxes'].tobytes() == y['all_boxes'].tobytes()
    lines.append('result arrays of the two paths bit-equal: %s; loss %.9g / %.9g, accuracy %.9g / %.9g' % (same, x['loss'], y['loss'], x['acc'], y['acc']))
    print('\n'.join(lines[-6:]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
