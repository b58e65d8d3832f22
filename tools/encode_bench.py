#!/usr/bin/env python
"""What DARK's unbiased target encoding costs and what it buys, in ONE process and ONE call.

    python tools/encode_bench.py [--pairs 6 --launches 2000 --batches 50 --iters 30 --parts abct] [--out profiles/encode_bench.txt]

(a) The launch alone: fpd_render_targets_unbiased against fpd_render_targets_w (the biased launch of the loader) at
    32x16x64x64, sigma 2, on the same seeded joints: `--pairs` interleaved pairs of windows of `--launches` back-to-back
    launches each between two device events, after one untimed window each.
(b) One DeviceAugmentLoader training batch (three launches), MODEL.TARGET_TYPE gaussian against gaussian_unbiased: host
    clock around `--batches` batches being enqueued, and device events around each batch's launches behind a plug of
    matmuls, in interleaved pairs.
(c) Training throughput: core.function.fpd_train over the synthetic_aug loader with the benchmark pair (hg4x128 bf16
    student, hg8x256 bf16 teacher, batch 32, 256x256), `--iters` iterations per run, interleaved pairs, one untimed run each.
The rule of the other tools decides: a difference is ESTABLISHED only if the mean difference is at least twice the largest
same-path spread and every run of one setting beats every run of the other.

Then the encode-to-decode accuracy table at 64x48 from the device kernels: targets rendered by fpd_render_targets
(biased) or fpd_render_targets_unbiased, decoded by the arg-max, the quarter-pixel shift or fpd_dark_refine; distance to
the true sub-pixel centre in heat-map pixels."""
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

from fpd_amd import executor as E  # noqa: E402
from fpd_amd import runtime as R  # noqa: E402
from fpd_amd import synth  # noqa: E402
from fpd_amd.lib import models  # noqa: E402,F401
from fpd_amd.lib.config import _defaults  # noqa: E402
from fpd_amd.lib.core import function as F  # noqa: E402
from fpd_amd.lib.core.inference import final_preds_device  # noqa: E402
from fpd_amd.lib.core.loss import JointsMSELoss  # noqa: E402
from fpd_amd.lib.dataset import DeviceAugmentLoader, DeviceJointsDB, DevicePipeline  # noqa: E402
from fpd_amd.lib.dataset.device_pipeline import gaussian_patch  # noqa: E402
from fpd_amd.lib.utils.utils import FusedAdam  # noqa: E402

TYPES = ('gaussian', 'gaussian_unbiased')


def verdict(lines, what, unit, runs):
    """Mean difference against the largest same-path spread, and whether every run of one side beats every run of the other."""
    a, b = (np.array(runs[t]) for t in TYPES)
    for t, v in zip(TYPES, (a, b)):
        lines.append('%-18s mean %10.3f  min %10.3f  max %10.3f %s' % (t, v.mean(), v.min(), v.max(), unit))
    diff = b.mean() - a.mean()
    spread = max(a.max() - a.min(), b.max() - b.min())
    every = bool(a.max() < b.min() or b.max() < a.min())
    lines.append('%s: mean difference (unbiased - gaussian) %+.3f %s (%+.2f %%); largest same-path spread %.3f %s; ratio %.2f (bar: 2); '
                 'every run of one side beyond every run of the other: %s' % (what, diff, unit, 100 * diff / a.mean(), spread, unit,
                                                                             abs(diff) / max(spread, 1e-12), every))
    lines.append('verdict by the bar set beforehand: a difference is %s' % ('ESTABLISHED' if abs(diff) >= 2 * spread and every else 'NOT ESTABLISHED'))
    lines.append('')


def window(call, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def launch_alone(a, lines):
    b, j, h, w, sigma = 32, 16, 64, 64, 2
    lib, st = R.lib(), R.current_stream()
    g = torch.Generator().manual_seed(0)
    joints = torch.zeros((b, j, 3), dtype=torch.float64)
    joints[..., 0:2] = torch.rand(b, j, 2, generator=g, dtype=torch.float64) * 4 * w
    joints = joints.cuda()
    vis = (torch.rand(b, j, generator=g) < 0.85).float().cuda()
    patch = torch.from_numpy(np.ascontiguousarray(gaussian_patch(sigma), np.float32)).cuda()
    target = torch.empty((b, j, h, w), dtype=torch.float32, device='cuda')
    weight = torch.empty((b, j, 1), dtype=torch.float32, device='cuda')
    t = R.TargetsWT()
    t.t.B, t.t.J, t.t.H, t.t.W, t.t.patch, t.t.stride_x, t.t.stride_y = b, j, h, w, patch.shape[0], 4.0, 4.0
    t.t.joints, t.t.vis, t.t.g, t.t.target, t.t.weight = joints.data_ptr(), vis.data_ptr(), patch.data_ptr(), target.data_ptr(), weight.data_ptr()
    u = R.TargetsUnbiasedT()
    u.B, u.J, u.H, u.W, u.sigma, u.stride_x, u.stride_y = b, j, h, w, sigma, 4.0, 4.0
    u.joints, u.vis, u.target, u.weight = joints.data_ptr(), vis.data_ptr(), target.data_ptr(), weight.data_ptr()
    calls = {'gaussian': lambda: R.check(lib.fpd_render_targets_w(t, st), 'fpd_render_targets_w'),
             'gaussian_unbiased': lambda: R.check(lib.fpd_render_targets_unbiased(u, st), 'fpd_render_targets_unbiased')}
    runs = {k: [] for k in TYPES}
    for k in TYPES:
        window(calls[k], a.launches)
    for _ in range(a.pairs):
        for k in TYPES:
            runs[k].append(window(calls[k], a.launches))
    lines.append('(a) The launch alone at %dx%dx%dx%d, sigma %d (%d of %d joints visible), library %s: fpd_render_targets_w (gaussian) '
                 'against fpd_render_targets_unbiased, %d interleaved pairs of windows of %d back-to-back launches between device events, '
                 'one untimed window each; microseconds per launch.'
                 % (b, j, h, w, sigma, int(vis.sum()), b * j, os.path.basename(R.LIB_PATH), a.pairs, a.launches))
    verdict(lines, 'launch', 'us', runs)


def loader_batch(a, lines):
    dev = torch.device('cuda:0')
    sc = synth.make_scenes(7, 64, 16, size=(256, 384), aspect_ratio=1.0)
    db = DeviceJointsDB(device=dev, **sc)
    loaders = {}
    for tt in TYPES:
        cfg = _defaults()
        cfg.DATASET.PROB_HALF_BODY, cfg.MODEL.TARGET_TYPE = 0.3, tt
        loaders[tt] = DeviceAugmentLoader(db, cfg, 32, True, shuffle=True, drop_last=True, seed=0)
    rng = np.random.Generator(np.random.PCG64(1))
    plug = torch.randn(4096, 4096, device=dev)

    def host_ms(loader):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.batches):
            loader.batch(rng.integers(0, 64, 32).astype(np.int32), rng)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3 / a.batches

    def device_ms(loader):
        torch.cuda.synchronize()
        for _ in range(24):
            plug @ plug
        ev = []
        for _ in range(a.batches):
            rows = loader.stage(rng.integers(0, 64, 32).astype(np.int32), rng).to(dev, non_blocking=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loader.launch(rows, 32)
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))
    host, devt = {k: [] for k in TYPES}, {k: [] for k in TYPES}
    for tt in TYPES:
        host_ms(loaders[tt]); device_ms(loaders[tt])
    for _ in range(a.pairs):
        for tt in TYPES:
            host[tt].append(host_ms(loaders[tt]))
            devt[tt].append(device_ms(loaders[tt]))
    lines.append('(b) One DeviceAugmentLoader training batch (32 crops of 256x256 from 64 scenes, 16 joints, three launches): %d interleaved '
                 'pairs; host = clock around %d batches being enqueued, device = median over %d batches of the events around the three '
                 'launches behind a plug of matmuls; milliseconds per batch.' % (a.pairs, a.batches, a.batches))
    verdict(lines, 'host', 'ms', host)
    verdict(lines, 'device', 'ms', devt)


def training(a, lines):
    cfgd = os.path.join(ROOT, 'experiments', 'fpd_synthetic')
    cfg = _defaults()
    cfg.merge_from_file(os.path.join(cfgd, 'hg4x128_student.yaml'))
    tcfg = cfg.clone()                                         # as tools/fpd_train.py: the teacher's file over the student's config
    tcfg.merge_from_file(os.path.join(cfgd, 'hg8x256_teacher.yaml'))
    cfg.PRINT_FREQ = a.iters                                   # one drain per run: the loop's only host synchronisation
    bs = cfg.TRAIN.BATCH_SIZE_PER_GPU
    torch.manual_seed(1)
    student = models.hourglass.get_pose_net(cfg, is_train=True).cuda()
    torch.manual_seed(2)
    teacher = models.hourglass.get_pose_net(tcfg, is_train=False).cuda()
    opt = FusedAdam(student, lr=cfg.TRAIN.LR)
    crit = JointsMSELoss(True).cuda()
    w, h = cfg.MODEL.IMAGE_SIZE
    n_scenes = 64
    db = DeviceJointsDB(device='cuda', **synth.make_scenes(17, n_scenes, cfg.MODEL.NUM_JOINTS, size=(w, w + w // 2), aspect_ratio=1.0))
    rng = np.random.Generator(np.random.PCG64(3))

    class Batches(object):
        """`--iters` training batches of random scenes per epoch through one DeviceAugmentLoader."""
        def __init__(self, loader):
            self.loader = loader

        def __len__(self):
            return a.iters

        def __iter__(self):
            for _ in range(a.iters):
                yield self.loader.batch(rng.integers(0, n_scenes, bs).astype(np.int32), rng)
    loaders = {}
    for tt in TYPES:
        c = cfg.clone()
        c.MODEL.TARGET_TYPE = tt
        loaders[tt] = Batches(DeviceAugmentLoader(db, c, bs, True, shuffle=True, drop_last=True, seed=0))
    # the random teacher gets sane eval-mode BN statistics once, as in tools/fpd_train.py
    x0 = next(iter(loaders['gaussian']))[0]
    cal = E.GraphInstance(teacher.device_state(), teacher.cfg_hg, x0.shape[0], x0.shape[2], x0.shape[3], train=True).finalize()
    cal.image().copy_(x0)
    cal.run('prep')
    cal.run('fwd')
    cal.calibrate_running_stats()
    del cal
    out = tempfile.mkdtemp()

    def run(tt):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        F.fpd_train(cfg, loaders[tt], student, teacher, crit, crit, opt, 0, out, out, None)
        torch.cuda.synchronize()
        return len(loaders[tt]) * bs / (time.perf_counter() - t0)
    runs = {k: [] for k in TYPES}
    for tt in TYPES:
        run(tt)
    for _ in range(a.pairs):
        for tt in TYPES:
            runs[tt].append(run(tt))
            print('%-18s %9.1f images/s' % (tt, runs[tt][-1]), flush=True)
    lines.append('(c) core.function.fpd_train over the device-augmenting loader, the benchmark pair (hg4x128 bf16 student, hg8x256 bf16 '
                 'teacher, batch %d, %dx%d), %d iterations per run, one untimed run each, then %d interleaved pairs; images/s.'
                 % (bs, h, w, a.iters, a.pairs))
    verdict(lines, 'throughput', 'images/s', runs)


def accuracy(a, lines):
    w, h, sigma, k, n, j = 48, 64, 2, 11, 25, 16
    rng = np.random.RandomState(20261020)
    cen = np.stack([rng.uniform(4, w - 5, (n, j)), rng.uniform(4, h - 5, (n, j))], -1)
    joints = torch.from_numpy(np.concatenate([cen * 4.0, np.zeros((n, j, 1))], -1)).cuda()
    vis = torch.ones((n, j), dtype=torch.float32, device='cuda')
    lines.append('Encode to decode at %dx%d (h x w), sigma %d, k %d, %d seeded sub-pixel centres in [4, W-5] x [4, H-5], everything on the '
                 'device: distance to the true centre in heat-map pixels, median / max.' % (h, w, sigma, k, n * j))
    lines.append('%-36s %-22s %-22s %-22s' % ('targets', 'arg-max', 'quarter-pixel shift', 'DARK'))
    for name, tt in (('biased (fpd_render_targets)', 'gaussian'), ('unbiased (fpd_render_targets_unbiased)', 'gaussian_unbiased')):
        maps = DevicePipeline((4 * w, 4 * h), (w, h), sigma, 'cuda', target_type=tt).generate_target(joints, vis)[0]
        cells = []
        for post, dark in ((False, 0), (True, 0), (False, k)):
            coords = final_preds_device(maps, None, post, dark=dark)[0].cpu().numpy()
            d = np.linalg.norm(coords.astype(np.float64) - cen, axis=-1)
            cells.append('%.3e / %.3e' % (np.median(d), d.max()))
        lines.append('%-36s %-22s %-22s %-22s' % ((name,) + tuple(cells)))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--launches', type=int, default=2000)
    ap.add_argument('--batches', type=int, default=50)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--parts', default='abct', help='which of (a), (b), (c) and the accuracy table (t) to run')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'encode_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'encode_bench needs the GPU'
    logging.basicConfig(level=logging.WARNING)
    lines = []
    for step in [f for k, f in zip('abct', (launch_alone, loader_batch, training, accuracy)) if k in a.parts]:
        mark = len(lines)
        step(a, lines)
        print('\n'.join(lines[mark:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
