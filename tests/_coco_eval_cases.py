"""Pictures for the device AP table (csrc/coco_eval.hip; tests/test_coco_eval_cpu.py, tests/test_coco_eval_gpu.py,
tools/coco_eval_bench.py): a generated set of annotation / result dicts that holds every situation the matching can meet,
the dict-based grouping of coco_eval.evaluate_keypoints restated so that its per-picture results can be compared one by one,
and the builders of the hand-derived scenes of tests/test_coco_cpu.py.

The expected values always come from the host functions of lib/dataset/coco_eval.py (picture_oks, match_picture, accumulate,
evaluate_keypoints), never from the device path.

Why the people of a picture are either near each other or 10^6 px apart: the device's exp and its summation order differ from
numpy's in the last bits, so a comparison of the matching may only flip where two OKS values, or a value and a threshold, are
closer than that.  People jittered about one pose have OKS values spread over (0.01, 1); people 10^6 px away have OKS exactly 0
(the exp underflows); what must not occur are tiny non-zero values such as 1e-80 and 1e-90 side by side."""
import functools

import numpy as np

SEED = 20
J = 17
FAST_G = 64                     # csrc/coco_eval.hip COCO_FAST_G: up to this many gts the taken flags are a register bit mask
BIG_G = 200                     # the picture that takes the general path
ALWAYS_ON = (5, 6, 11, 12, 13, 14)      # joints every annotated gt has: the OKS never rests on one small-sigma joint alone


def gt_dict(img, kpts, area, bbox=None, iscrowd=0):
    k = np.asarray(kpts, np.float64).reshape(J, 3)
    if bbox is None:
        x0, y0 = k[:, 0].min(), k[:, 1].min()
        bbox = [float(x0), float(y0), float(k[:, 0].max() - x0), float(k[:, 1].max() - y0)]
    return {'image_id': img, 'category_id': 1, 'keypoints': k.reshape(-1).tolist(), 'num_keypoints': int((k[:, 2] > 0).sum()),
            'area': float(area), 'bbox': [float(v) for v in bbox], 'iscrowd': int(iscrowd)}


def dt_dict(img, kpts, score):
    k = np.zeros((J, 3))
    k[:, 0:2] = np.asarray(kpts, np.float64).reshape(J, -1)[:, 0:2]
    k[:, 2] = 0.9
    return {'image_id': img, 'category_id': 1, 'keypoints': k.reshape(-1).tolist(), 'score': float(score)}


def _visibility(rng):
    v = rng.choice([0.0, 1.0, 2.0], J, p=[0.3, 0.2, 0.5])
    v[list(ALWAYS_ON)] = 2
    return v


AREAS = (700.0, 1000.0, 3000.0, 9000.0, 20000.0)          # a picture's people have 0.5 .. 2 times one of these: both edges of 'medium' are crossed


def random_picture(rng, img, n_gt, n_dt, crowd=0.1, blank=0.1, far=0.15):
    """n_gt people jittered about one pose (some crowds, some without an annotated joint, some 10^6 px away) and n_dt
    detections jittered about them (some 2 * 10^6 px away), scores with two decimals (ties within and across pictures)."""
    ext = float([25.0, 70.0, 200.0][int(rng.integers(0, 3))])
    base = 300.0 + rng.uniform(0, ext, (J, 2))
    unit = float(AREAS[int(rng.integers(0, len(AREAS)))])
    step = np.sqrt(unit) * 0.05                                     # the jitter that costs a mid-sigma joint about exp(-1/4)
    gts, poses = [], []
    for _ in range(n_gt):
        area = unit * rng.uniform(0.5, 2.0)
        xy = base + rng.standard_normal((J, 2)) * rng.uniform(0, 3) * step
        if rng.uniform() < far:
            xy = xy + 1e6
        k = np.concatenate([xy, _visibility(rng)[:, None]], 1)
        bbox = None
        if rng.uniform() < blank:                                   # no annotated joint: its box doubled about itself is the pose's extent
            k[:, 2] = 0
            x0, y0, w, h = xy[:, 0].min(), xy[:, 1].min(), np.ptp(xy[:, 0]), np.ptp(xy[:, 1])
            bbox = [x0 + w / 3, y0 + h / 3, w / 3, h / 3]
        gts.append(gt_dict(img, k, area, bbox, iscrowd=int(rng.uniform() < crowd)))
        poses.append(xy)
    dts = []
    for _ in range(n_dt):
        xy = poses[int(rng.integers(0, len(poses)))] if poses else base
        xy = xy + rng.standard_normal((J, 2)) * rng.uniform(0.05, 2.5) * step
        if rng.uniform() < far:
            xy = xy + 2e6
        dts.append(dt_dict(img, xy, np.round(rng.uniform(0.1, 1.0), 2)))
    return gts, dts


def eye_gt(image_id, x, y, area=2500.0, iscrowd=0, annotated=True):
    """tests/test_coco_cpu.py: a person whose only annotated joint is the left eye at (x, y); annotated False: no joint at
    all and a 10 x 10 box at (x, y)."""
    k = np.zeros((J, 3))
    if annotated:
        k[1] = (x, y, 2)
    return {'image_id': image_id, 'category_id': 1, 'keypoints': k.reshape(-1).tolist(), 'num_keypoints': int(annotated),
            'area': area, 'bbox': [x, y, 10.0, 10.0], 'iscrowd': iscrowd}


def eye_dt(image_id, x, y, score, extent=(40.0, 50.0)):
    """tests/test_coco_cpu.py: a detection whose left eye is at (x, y); its other joints span a box of `extent`."""
    k = np.zeros((J, 3))
    k[:, 0], k[:, 1] = x, y
    k[0, 0:2] = (x + extent[0], y + extent[1])
    k[:, 2] = 0.9
    return {'image_id': image_id, 'category_id': 1, 'keypoints': k.reshape(-1).tolist(), 'score': score}


def hand_scenes():
    """The scenes of tests/test_coco_cpu.py's keypoint AP section -> {name: (gts, dts)}."""
    rng = np.random.default_rng(3)
    exact = ([], [])
    for n, (img, score) in enumerate(((7, 0.9), (7, 0.6), (9, 0.75))):
        k = np.zeros((J, 3))
        k[:, 0:2] = rng.uniform(0, 60, (J, 2)) + 200 * n
        k[:, 2] = 2
        exact[0].append({'image_id': img, 'category_id': 1, 'keypoints': k.reshape(-1).tolist(), 'num_keypoints': J, 'area': 2500.0,
                         'bbox': [200.0 * n, 200.0 * n, 60.0, 60.0], 'iscrowd': 0})
        exact[1].append({'image_id': img, 'category_id': 1, 'keypoints': k.reshape(-1).tolist(), 'score': score})
    two = [eye_gt(1, 100, 100), eye_gt(1, 300, 100)]
    return {
        'exact': exact,
        'far_in_front': (two, [eye_dt(1, 600, 100, 0.9), eye_dt(1, 100, 100, 0.4)]),
        'outside_the_range': (two, [eye_dt(1, 600, 100, 0.9, extent=(100.0, 100.0)), eye_dt(1, 100, 100, 0.4)]),
        'crowd_and_unannotated': ([eye_gt(1, 100, 100), eye_gt(1, 200, 100), eye_gt(1, 300, 100, iscrowd=1), eye_gt(1, 400, 100, annotated=False)],
                                  [eye_dt(1, 100, 100, 0.9), eye_dt(1, 200, 100, 0.85), eye_dt(1, 300, 100, 0.8), eye_dt(1, 300, 100, 0.7),
                                   eye_dt(1, 395, 95, 0.6, extent=(20.0, 20.0))]),
        'taken': (two, [eye_dt(1, 100, 100, 0.9), eye_dt(1, 100, 100, 0.8), eye_dt(1, 300, 100, 0.7)]),
        'scan_stops': ([eye_gt(1, 100, 100), eye_gt(1, 101, 102, iscrowd=1)], [eye_dt(1, 101, 102, 0.9)]),
        'best_fit': ([eye_gt(1, 100, 100, area=9000.0), eye_gt(1, 101, 102, area=1600.0)], [eye_dt(1, 101, 102, 0.9), eye_dt(1, 100, 100, 0.8)]),
        'cut_21': ([eye_gt(1, 100 * k, 50) for k in range(21)], [eye_dt(1, 100 * k, 50, 0.95 - 0.01 * k) for k in range(21)]),
        'large_and_empty': ([eye_gt(1, 100, 100, area=10000.0), eye_gt(2, 100, 100)], [eye_dt(1, 100, 100, 0.9)]),
    }


# the pictures of the generated set that are built on purpose; every other id is a random picture
PIC = {'gts_only': 101, 'dts_only': 102, 'empty': 103, 'twenty': 104, 'twenty_five': 105, 'one_dt': 106, 'crowd': 107,
       'blank': 108, 'twins': 109, 'edges': 110, 'scan_stops': 111, 'best_fit': 112, 'big': 113}


def _retarget(people, img):
    return [dict(p, image_id=img) for p in people]


@functools.lru_cache(maxsize=None)
def case_set(seed=SEED):
    """-> (gts, dts, image_ids): 13 pictures built on purpose (PIC) and 27 random ones.  The results are shuffled: neither
    grouped by picture nor sorted by score, so the grouping and the stable order of equal scores are exercised."""
    rng = np.random.default_rng(seed)
    gts, dts = [], []

    def add(pair):
        gts.extend(pair[0])
        dts.extend(pair[1])
    add(random_picture(rng, PIC['gts_only'], 4, 0))
    add(random_picture(rng, PIC['dts_only'], 0, 5))
    add(random_picture(rng, PIC['twenty'], 6, 20, far=0))
    add(random_picture(rng, PIC['twenty_five'], 8, 25, far=0))
    add(random_picture(rng, PIC['one_dt'], 3, 1, far=0, blank=0, crowd=0))
    # a crowd among ordinary people, four detections on the crowd itself
    g, d = random_picture(rng, PIC['crowd'], 3, 2, far=0, blank=0, crowd=0)
    k = np.asarray(g[0]['keypoints']).reshape(J, 3).copy()
    k[:, 0:2] += 1e6
    g.append(gt_dict(PIC['crowd'], k, 5000.0, iscrowd=1))
    for s in (0.91, 0.73, 0.73, 0.35):
        d.append(dt_dict(PIC['crowd'], k[:, 0:2] + rng.standard_normal((J, 2)) * 0.8, s))
    add((g, d))
    # a gt without an annotated joint: detections inside its doubled box (OKS 1) and sticking out of it
    xy = 300.0 + rng.uniform(0, 90, (J, 2))
    x0, y0, w, h = xy[:, 0].min(), xy[:, 1].min(), np.ptp(xy[:, 0]), np.ptp(xy[:, 1])
    centre = np.array([x0 + w / 2, y0 + h / 2])
    blank = gt_dict(PIC['blank'], np.concatenate([xy, np.zeros((J, 1))], 1), 3000.0, [x0 + w / 3, y0 + h / 3, w / 3, h / 3])
    add(([blank], [dt_dict(PIC['blank'], centre + (xy - centre) * 0.5, 0.8), dt_dict(PIC['blank'], xy + rng.standard_normal((J, 2)) * 4, 0.6),
                   dt_dict(PIC['blank'], xy + rng.standard_normal((J, 2)) * 9, 0.5)]))
    # two byte-identical gts and two detections near them
    g, d = random_picture(rng, PIC['twins'], 1, 2, far=0, blank=0, crowd=0)
    add((g + [dict(g[0])], d))
    # areas exactly on the edges of the medium range
    g, d = random_picture(rng, PIC['edges'], 2, 3, far=0, blank=0, crowd=0)
    g[0]['area'], g[1]['area'] = float(32 ** 2), float(96 ** 2)
    add((g, d))
    scenes = hand_scenes()
    add((_retarget(scenes['scan_stops'][0], PIC['scan_stops']), _retarget(scenes['scan_stops'][1], PIC['scan_stops'])))
    add((_retarget(scenes['best_fit'][0], PIC['best_fit']), _retarget(scenes['best_fit'][1], PIC['best_fit'])))
    add(random_picture(rng, PIC['big'], BIG_G, 20, far=0.05))
    for n in range(27):
        add(random_picture(rng, 200 + n, int(rng.integers(0, 9)), int(rng.integers(0, 14))))
    dts = [dts[i] for i in rng.permutation(len(dts))]
    image_ids = sorted(set(PIC.values()) | set(range(200, 227)))
    return gts, dts, image_ids


def host_pictures(gts, dts, image_ids, cat=1):
    """evaluate_keypoints' grouping, restated -> per picture of the sorted ids (gts, dts cut to the 20 best, picture_oks,
    [match_picture per area range])."""
    from fpd_amd.lib.dataset import coco_eval as E
    by_gt, by_dt = {}, {}
    for g in gts:
        g = dict(g, _ignore=bool(g.get('iscrowd', 0)) or g['num_keypoints'] == 0)
        by_gt.setdefault((g['image_id'], g['category_id']), []).append(g)
    for pos, d in enumerate(dts):
        d = dict(d, _area=E.detection_area(d['keypoints']), id=pos + 1)
        by_dt.setdefault((d['image_id'], d['category_id']), []).append(d)
    out = []
    for img in sorted(set(image_ids)):
        g = by_gt.get((img, cat), [])
        d = by_dt.get((img, cat), [])
        d = [d[i] for i in np.argsort([-x['score'] for x in d], kind='mergesort')[:E.MAX_DETS]]
        oks = E.picture_oks(g, d)
        out.append((g, d, oks, [E.match_picture(g, d, oks, rng) for rng in E.AREA_RANGES]))
    return out


@functools.lru_cache(maxsize=None)
def host_case_set(seed=SEED):
    gts, dts, image_ids = case_set(seed)
    return host_pictures(gts, dts, image_ids)


def margins(pictures):
    """(smallest |oks - t| over the ten thresholds, OKS exactly 1 aside; smallest gap between two different OKS values of one
    detection's row) over the host_pictures() given."""
    from fpd_amd.lib.dataset import coco_eval as E
    thr_gap = row_gap = np.inf
    for _, _, oks, _ in pictures:
        if oks.size == 0:
            continue
        v = oks[oks != 1.0]
        if v.size:
            thr_gap = min(thr_gap, float(np.abs(v[:, None] - E.OKS_THRS[None, :]).min()))
        for row in oks:
            u = np.unique(row)
            if u.size > 1:
                row_gap = min(row_gap, float(np.diff(u).min()))
    return thr_gap, row_gap


def flag_tables(pictures):
    """The host's flags laid out as the device writes them -> (matched [3,10,D], dt_ignored [3,10,D] uint8, gt_counted [3,n_img],
    scores [D], dt_area [D]); pictures in order, the detections of a picture best first."""
    from fpd_amd.lib.dataset import coco_eval as E
    na, nt = len(E.AREA_RANGES), len(E.OKS_THRS)
    d_total = sum(len(p[1]) for p in pictures)
    matched, ignored = np.zeros((na, nt, d_total), np.uint8), np.zeros((na, nt, d_total), np.uint8)
    counted = np.zeros((na, len(pictures)), np.int32)
    at = 0
    for i, (g, d, _, res) in enumerate(pictures):
        for r in range(na):
            if res[r] is None:
                continue
            matched[r, :, at:at + len(d)], ignored[r, :, at:at + len(d)] = res[r][0], res[r][1]
            counted[r, i] = int(np.count_nonzero(~res[r][2]))
        at += len(d)
    scores = np.array([x['score'] for p in pictures for x in p[1]], np.float64)
    area = np.array([x['_area'] for p in pictures for x in p[1]], np.float64)
    return matched, ignored, counted, scores, area


def device_inputs(gts, dts, image_ids, device='cuda'):
    """What evaluate_arrays_device uploads, for the tests that drive match_device themselves -> (dict of device tensors, packed
    gt, rows, dt_offsets)."""
    from fpd_amd.lib.dataset import coco_eval as E
    packed = E.pack_ground_truth(gts, image_ids, 1)
    scores = np.array([d['score'] for d in dts], np.float64)
    kpts = np.array([d['keypoints'] for d in dts], np.float64).reshape(len(dts), J, 3)
    rows, dt_offsets = E.group_detections(packed['image_ids'], [d['image_id'] for d in dts], scores)
    pairs = np.diff(dt_offsets).astype(np.int64) * np.diff(packed['gt_offsets']).astype(np.int64)
    oks_offsets = np.concatenate([[0], np.cumsum(pairs)]).astype(np.int64)
    t = E.upload({'gt_kpts': packed["gt_kpts"].reshape(len(packed["gt_area"]), J, 3), 'gt_area': packed['gt_area'], 'gt_bbox': packed['gt_bbox'],
                  'dt_kpts': kpts[rows], 'scores': scores[rows], 'sigmas': E.SIGMAS, 'rec_thrs': E.REC_THRS, 'oks_offsets': oks_offsets,
                  'gt_offsets': packed['gt_offsets'], 'dt_offsets': dt_offsets, 'gt_flags': packed['gt_flags']}, device)
    t['oks_total'] = int(oks_offsets[-1])
    return t, packed, rows, dt_offsets
