#!/usr/bin/env python
"""Times the rescoring + OKS NMS step of COCODataset.evaluate at the scale of val2017 with detection boxes -- 5 000 pictures,
about 100 000 people, clustered the way the tests' people are (tests/_coco_ref.clustered_people) -- on the device
(csrc/oks_nms.hip, one launch for all pictures) and as the numpy restatement of the tests (tests/_coco_ref.nms_pictures:
a Python loop over pictures, vectorised over the people of one) on the same machine:

    python tools/oks_nms_bench.py [--pictures 5000 --mean-people 20 --seed 0 --reps 5 --time-limit 600] [--out FILE]

  device launch      device events around the one launch (median of --reps launches after one warm-up launch)
  device end to end  host clock around lib.nms.nms.oks_nms_device: upload of the people, launch, download (median of --reps)
  host restatement   host clock around tests/_coco_ref.nms_pictures, once per mode
The two paths must agree on every score and keep list, or the tool fails.  At most 16 host threads; the whole run stands
under --time-limit seconds (SIGALRM)."""
import argparse
import os
import signal
import statistics
import sys
import time

for _v in ('OMP_NUM_THREADS', 'MKL_NUM_THREADS', 'OPENBLAS_NUM_THREADS'):
    os.environ[_v] = str(min(16, int(os.environ.get(_v) or 16)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fpd_amd.lib.nms.nms import oks_nms_device  # noqa: E402
from tests import _coco_ref as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pictures', type=int, default=5000)
    ap.add_argument('--mean-people', type=int, default=20)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--time-limit', type=int, default=600)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit('oks_nms_bench: time limit of %d s reached' % a.time_limit))
    signal.alarm(a.time_limit)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    assert torch.cuda.is_available(), 'oks_nms_bench needs the GPU'
    rng = np.random.default_rng(a.seed)
    sizes = rng.integers(1, 2 * a.mean_people, a.pictures)
    parts = [C.clustered_people(rng, int(p)) for p in sizes]
    kpts, area, box = (np.concatenate([c[k] for c in parts]) for k in range(3))
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    thresh, vis = 0.9, 0.2
    lines = ['oks_nms_bench: %d pictures, %d people (1..%d per picture), 17 joints, OKS_THRE %.1f, IN_VIS_THRE %.1f; %d reps'
             % (a.pictures, len(kpts), sizes.max(), thresh, vis, a.reps)]
    oks_nms_device(kpts[:64], area[:64], box[:64], [0, 64], thresh, in_vis_thre=vis)           # library load, first launch
    for soft in (False, True):
        launch_ms, wall_ms = [], []

        def timer(launch):
            launch()                                                                            # warm-up
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch()
                e1.record()
                e1.synchronize()
                launch_ms.append(e0.elapsed_time(e1))
        got = oks_nms_device(kpts, area, box, offsets, thresh, soft=soft, in_vis_thre=vis, timer=timer)
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = oks_nms_device(kpts, area, box, offsets, thresh, soft=soft, in_vis_thre=vis)
            wall_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want = C.nms_pictures(kpts, area, box, offsets, vis, thresh, soft)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(g, w) for g, w in zip(got, want))
        dev, wall = statistics.median(launch_ms), statistics.median(wall_ms)
        lines.append('%s: kept %d of %d | device launch %.3f ms (min %.3f max %.3f) | device end to end (upload + launch + download) '
                     '%.3f ms (min %.3f max %.3f) | host restatement %.1f ms | host / device end to end %.1fx | results %s'
                     % ('soft' if soft else 'hard', int(want[2].sum()), len(kpts), dev, min(launch_ms), max(launch_ms), wall,
                        min(wall_ms), max(wall_ms), host_ms, host_ms / wall, 'identical' if same else 'DIFFER'))
        print(lines[-1], flush=True)
        if not same:
            sys.exit('oks_nms_bench: the device and the host restatement disagree')
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
