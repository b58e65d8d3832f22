#!/usr/bin/env python
"""Times the keypoint AP table of COCODataset.evaluate at the scale of val2017 -- 5 000 pictures, gts and post-NMS detections
per picture drawn the way the tests draw them (tests/_coco_eval_cases.random_picture) -- on the device (csrc/coco_eval.hip:
fpd_coco_match + fpd_coco_accumulate) and on the host (lib/dataset/coco_eval.evaluate_keypoints) on the same machine:

    python tools/coco_eval_bench.py [--pictures 5000 --max-gts 4 --max-dts 24 --seed 0 --reps 5 --time-limit 900] [--out FILE]

  device launches    device events around each of the two launches (median of --reps after one warm-up launch each)
  device end to end  host clock around coco_eval.evaluate_arrays_device: grouping and cut on the host, upload, both launches,
                     the device sort, download of the tables, the ten means (median of --reps); the gts are packed once per
                     dataset (coco_eval.pack_ground_truth), timed apart
  host               host clock around evaluate_keypoints over the same dicts, once
The ten statistics of the two paths must be equal, or the tool fails.  At most 16 host threads; the whole run stands under
--time-limit seconds (SIGALRM).  Writes --out (default profiles/coco_eval_bench.txt)."""
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

from fpd_amd.lib.dataset import coco_eval as E  # noqa: E402
from tests import _coco_eval_cases as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pictures', type=int, default=5000)
    ap.add_argument('--max-gts', type=int, default=4)
    ap.add_argument('--max-dts', type=int, default=24)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--time-limit', type=int, default=900)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coco_eval_bench.txt'))
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit('coco_eval_bench: time limit of %d s reached' % a.time_limit))
    signal.alarm(a.time_limit)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    assert torch.cuda.is_available(), 'coco_eval_bench needs the GPU'
    rng = np.random.default_rng(a.seed)
    gts, dts, image_ids = [], [], list(range(1, a.pictures + 1))
    for img in image_ids:
        g, d = K.random_picture(rng, img, int(rng.integers(0, a.max_gts + 1)), int(rng.integers(0, a.max_dts + 1)))
        gts.extend(g)
        dts.extend(d)
    dts = [dts[i] for i in rng.permutation(len(dts))]
    dt_ids = np.array([d['image_id'] for d in dts], np.int64)
    dt_kpts = np.array([d['keypoints'] for d in dts], np.float64)
    dt_scores = np.array([d['score'] for d in dts], np.float64)
    t0 = time.perf_counter()
    packed = E.pack_ground_truth(gts, image_ids, 1)
    pack_ms = (time.perf_counter() - t0) * 1e3
    kept = int(E.group_detections(packed['image_ids'], dt_ids, dt_scores)[1][-1])
    lines = ['coco_eval_bench: %d pictures, %d gts, %d detections (%d after the cut to %d per picture), 17 joints; %d reps'
             % (a.pictures, len(gts), len(dts), kept, E.MAX_DETS, a.reps)]
    E.evaluate_arrays_device(packed, dt_ids[:64], dt_kpts[:64], dt_scores[:64])                    # library load, first launches
    launch_ms = {'match': [], 'accumulate': []}

    def timer(name):
        def run(launch):
            launch()                                                                                # warm-up
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch()
                e1.record()
                e1.synchronize()
                launch_ms[name].append(e0.elapsed_time(e1))
        return run
    got = E.evaluate_arrays_device(packed, dt_ids, dt_kpts, dt_scores, timer={k: timer(k) for k in launch_ms})
    wall_ms = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = E.evaluate_arrays_device(packed, dt_ids, dt_kpts, dt_scores)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    want = E.evaluate_keypoints(gts, dts, image_ids, [1])
    host_ms = (time.perf_counter() - t0) * 1e3
    same = got.tolist() == want.tolist()
    med = statistics.median
    wall = med(wall_ms)
    lines.append('device launches: fpd_coco_match %.3f ms (min %.3f max %.3f) | fpd_coco_accumulate %.3f ms (min %.3f max %.3f)'
                 % (med(launch_ms['match']), min(launch_ms['match']), max(launch_ms['match']), med(launch_ms['accumulate']),
                    min(launch_ms['accumulate']), max(launch_ms['accumulate'])))
    lines.append('device end to end (grouping + upload + launches + sort + download + means) %.3f ms (min %.3f max %.3f) | packing the '
                 'gts, once per dataset %.1f ms | host evaluate_keypoints %.1f ms | host / device end to end %.1fx | statistics %s'
                 % (wall, min(wall_ms), max(wall_ms), pack_ms, host_ms, host_ms / wall, 'identical' if same else 'DIFFER'))
    lines.append('statistics: ' + ' '.join('%s %.6f' % (n, v) for n, v in zip(E.STAT_NAMES, want)))
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if not same:
        sys.exit('coco_eval_bench: the device and the host disagree: %s against %s' % (got.tolist(), want.tolist()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
