"""COCO keypoint AP / AR on the host (numpy), written from the published algorithm -- pycocotools is not available here, so
this table is NOT pinned to it by a test; tests/test_coco_cpu.py holds it to hand-derived cases.

    evaluate_keypoints(gts, dts, image_ids, cat_ids) -> the ten statistics
        AP, AP.5, AP.75, AP(M), AP(L), AR, AR.5, AR.75, AR(M), AR(L)

gts: annotation dicts of the ground-truth file (image_id, category_id, keypoints [3J], num_keypoints, area, bbox, iscrowd);
dts: result dicts (image_id, category_id, keypoints [3J], score) in the order of the results file.  Runs once per
validation; the per-picture matching is a Python loop over 10 thresholds x at most 20 detections x the picture's people."""
import numpy as np

SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
OKS_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = 20
AREA_RANGES = ((0 ** 2, 1e5 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))          # all, medium, large
STAT_NAMES = ('AP', 'Ap .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)')
EPS = np.spacing(1)


def detection_area(keypoints):
    """The extent of a detection's keypoints, (xmax - xmin) * (ymax - ymin)."""
    k = np.asarray(keypoints, np.float64)
    x, y = k[0::3], k[1::3]
    return float((x.max() - x.min()) * (y.max() - y.min()))


def picture_oks(gts, dts, sigmas=SIGMAS):
    """[len(dts), len(gts)]: a gt with annotated joints compares those joints; one without compares every joint by its
    distance outside the gt box doubled about itself."""
    out = np.zeros((len(dts), len(gts)))
    var = (np.asarray(sigmas, np.float64) * 2) ** 2
    for gi, gt in enumerate(gts):
        g = np.asarray(gt['keypoints'], np.float64)
        xg, yg, vg = g[0::3], g[1::3], g[2::3]
        on = vg > 0
        bx, by, bw, bh = gt['bbox']
        x0, x1, y0, y1 = bx - bw, bx + bw * 2, by - bh, by + bh * 2
        for di, dt in enumerate(dts):
            d = np.asarray(dt['keypoints'], np.float64)
            xd, yd = d[0::3], d[1::3]
            if on.any():
                dx, dy = xd - xg, yd - yg
            else:
                dx = np.maximum(0, x0 - xd) + np.maximum(0, xd - x1)
                dy = np.maximum(0, y0 - yd) + np.maximum(0, yd - y1)
            e = (dx ** 2 + dy ** 2) / var / (gt['area'] + EPS) / 2
            if on.any():
                e = e[on]
            out[di, gi] = np.sum(np.exp(-e)) / e.shape[0]
    return out


def match_picture(gts, dts, oks, area_range):
    """One picture, one area range.  dts: in descending score, at most MAX_DETS; oks [len(dts), len(gts)].
    -> (matched [T,D] bool, dt_ignored [T,D] bool, gt_ignored [G] bool, scores [D]) or None without gts and dts."""
    if not gts and not dts:
        return None
    lo, hi = area_range
    ignored = np.array([bool(g['_ignore']) or g['area'] < lo or g['area'] > hi for g in gts], bool)
    order = np.argsort(ignored, kind='mergesort')                   # the gts that count first
    ignored = ignored[order]
    crowd = np.array([bool(gts[k].get('iscrowd', 0)) for k in order], bool)
    oks = oks[:, order] if len(gts) and len(dts) else oks
    nt, nd, ng = len(OKS_THRS), len(dts), len(gts)
    gt_taken = np.zeros((nt, ng), bool)
    matched = np.zeros((nt, nd), bool)
    dt_ignored = np.zeros((nt, nd), bool)
    for ti, t in enumerate(OKS_THRS):
        for di in range(nd):
            best, m = min(t, 1 - 1e-10), -1
            for gi in range(ng):
                if gt_taken[ti, gi] and not crowd[gi]:
                    continue                                        # this gt is taken at this threshold
                if m > -1 and not ignored[m] and ignored[gi]:
                    break                                           # a counting match is in hand; only ignored gts follow
                if oks[di, gi] < best:
                    continue
                best, m = oks[di, gi], gi
            if m == -1:
                continue
            matched[ti, di] = True
            dt_ignored[ti, di] = ignored[m]
            gt_taken[ti, m] = True
    outside = np.array([d['_area'] < lo or d['_area'] > hi for d in dts], bool).reshape(1, nd)
    dt_ignored |= ~matched & np.repeat(outside, nt, 0)
    return matched, dt_ignored, ignored, np.array([d['score'] for d in dts], np.float64)


def accumulate(per_picture):
    """per_picture: the match_picture results of one category and one area range, in picture order
    -> (precision [T,R], recall [T]); -1 where there is no gt that counts."""
    nt, nr = len(OKS_THRS), len(REC_THRS)
    precision, recall = -np.ones((nt, nr)), -np.ones(nt)
    res = [r for r in per_picture if r is not None]
    if not res:
        return precision, recall
    scores = np.concatenate([r[3] for r in res])
    inds = np.argsort(-scores, kind='mergesort')
    matched = np.concatenate([r[0] for r in res], axis=1)[:, inds]
    dt_ig = np.concatenate([r[1] for r in res], axis=1)[:, inds]
    npig = int(np.count_nonzero(~np.concatenate([r[2] for r in res])))
    if npig == 0:
        return precision, recall
    tp_sum = np.cumsum(matched & ~dt_ig, axis=1).astype(np.float64)
    fp_sum = np.cumsum(~matched & ~dt_ig, axis=1).astype(np.float64)
    for ti in range(nt):
        tp, fp = tp_sum[ti], fp_sum[ti]
        nd = len(tp)
        rc = tp / npig
        pr = tp / (fp + tp + EPS)
        recall[ti] = rc[-1] if nd else 0
        for i in range(nd - 1, 0, -1):                              # non-increasing from the right
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        at = np.searchsorted(rc, REC_THRS, side='left')
        q = np.zeros(nr)
        inside = at < nd
        q[inside] = pr[at[inside]]
        precision[ti] = q
    return precision, recall


def _mean(v):
    v = v[v > -1]
    return float(np.mean(v)) if v.size else -1.0


def evaluate_keypoints(gts, dts, image_ids, cat_ids, sigmas=SIGMAS):
    """-> np.float64 [10] in the order of STAT_NAMES."""
    image_ids = sorted(set(image_ids))
    by_gt, by_dt = {}, {}
    for g in gts:
        g = dict(g, _ignore=bool(g.get('iscrowd', 0)) or g['num_keypoints'] == 0)
        by_gt.setdefault((g['image_id'], g['category_id']), []).append(g)
    for pos, d in enumerate(dts):
        d = dict(d, _area=detection_area(d['keypoints']), id=pos + 1)
        by_dt.setdefault((d['image_id'], d['category_id']), []).append(d)
    nt, nr, nk, na = len(OKS_THRS), len(REC_THRS), len(cat_ids), len(AREA_RANGES)
    precision, recall = -np.ones((nt, nr, nk, na)), -np.ones((nt, nk, na))
    for ki, cat in enumerate(cat_ids):
        per_area = [[] for _ in AREA_RANGES]
        for img in image_ids:
            g = by_gt.get((img, cat), [])
            d = by_dt.get((img, cat), [])
            d = [d[i] for i in np.argsort([-x['score'] for x in d], kind='mergesort')[:MAX_DETS]]
            oks = picture_oks(g, d, sigmas)
            for ai, rng in enumerate(AREA_RANGES):
                per_area[ai].append(match_picture(g, d, oks, rng))
        for ai in range(na):
            precision[:, :, ki, ai], recall[:, ki, ai] = accumulate(per_area[ai])
    t50, t75 = int(np.argmin(np.abs(OKS_THRS - 0.5))), int(np.argmin(np.abs(OKS_THRS - 0.75)))
    return np.array([_mean(precision[:, :, :, 0]), _mean(precision[t50, :, :, 0]), _mean(precision[t75, :, :, 0]),
                     _mean(precision[:, :, :, 1]), _mean(precision[:, :, :, 2]),
                     _mean(recall[:, :, 0]), _mean(recall[t50, :, 0]), _mean(recall[t75, :, 0]),
                     _mean(recall[:, :, 1]), _mean(recall[:, :, 2])], np.float64)


# ---- the same table on the device (csrc/coco_eval.hip: fpd_coco_match, fpd_coco_accumulate) ----------------------------------
# The functions above are the yardstick; the ones below restate them for the device and are held to them flag by flag
# (tests/test_coco_eval_gpu.py).  The host sorts and cuts with whole-array numpy calls; nothing below loops over pictures or
# detections except pack_ground_truth's one pass over the annotation dicts.

def _R():
    from ... import runtime
    return runtime


def _check_offsets(offsets, total, what):
    o = np.asarray(offsets, np.int64).reshape(-1)
    if o.size < 1 or o[0] != 0 or o[-1] != total or (np.diff(o) < 0).any() or total >= 2 ** 31:
        raise _R().FpdError('coco_eval: %s offsets must rise from 0 to %d' % (what, total))


def pack_ground_truth(gts, image_ids, cat_id):
    """The annotation dicts of category `cat_id` on the pictures `image_ids` as arrays, pictures in ascending id, the gts of
    a picture contiguous and in file order -> dict: image_ids [n_img] int64, gt_kpts [G,J,3], gt_area [G], gt_bbox [G,4]
    (float64), gt_flags [G] uint8 (bit 0: crowd or num_keypoints == 0, bit 1: crowd), gt_offsets [n_img+1] int32."""
    ids = sorted(set(image_ids))
    slot = {v: i for i, v in enumerate(ids)}
    pic, kpts, area, bbox, flags = [], [], [], [], []
    for g in gts:
        s = slot.get(g['image_id'])
        if s is None or g['category_id'] != cat_id:
            continue
        crowd = bool(g.get('iscrowd', 0))
        pic.append(s)
        kpts.append(g['keypoints'])
        area.append(g['area'])
        bbox.append(g['bbox'])
        flags.append(int(crowd or g['num_keypoints'] == 0) | int(crowd) << 1)
    n = len(pic)
    pic = np.asarray(pic, np.int64)
    order = np.argsort(pic, kind='stable')
    counts = np.bincount(pic, minlength=len(ids))
    return {'image_ids': np.asarray(ids, np.int64), 'cat_id': cat_id,
            'gt_kpts': np.ascontiguousarray(np.asarray(kpts, np.float64).reshape(n, -1 if n else 0, 3)[order]),
            'gt_area': np.asarray(area, np.float64).reshape(n)[order], 'gt_bbox': np.asarray(bbox, np.float64).reshape(n, 4)[order],
            'gt_flags': np.asarray(flags, np.uint8).reshape(n)[order],
            'gt_offsets': np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)}


def group_detections(image_ids, dt_image_ids, dt_scores):
    """The grouping of evaluate_keypoints over arrays: the detections (rows in results-file order) of each picture of the
    sorted `image_ids`, best score first, equal scores in file order, cut to the MAX_DETS best
    -> (rows [D] into the detections, pictures in ascending id; dt_offsets [n_img+1] int32)."""
    ids = np.asarray(image_ids, np.int64).reshape(-1)
    dt_ids = np.asarray(dt_image_ids, np.int64).reshape(-1)
    scores = np.asarray(dt_scores, np.float64).reshape(-1)
    if dt_ids.size != scores.size:
        raise _R().FpdError('coco_eval: %d detection picture ids, %d scores' % (dt_ids.size, scores.size))
    n_img = ids.size
    pic = np.searchsorted(ids, dt_ids)
    rows = np.flatnonzero(ids[np.minimum(pic, n_img - 1)] == dt_ids) if n_img else np.zeros(0, np.int64)
    rows = rows[np.lexsort((-scores[rows], pic[rows]))]              # by picture, then by falling score; stable
    p = pic[rows]
    counts = np.bincount(p, minlength=n_img)
    rank = np.arange(p.size) - (np.cumsum(counts) - counts)[p]
    rows = rows[rank < MAX_DETS]
    return rows, np.concatenate([[0], np.cumsum(np.minimum(counts, MAX_DETS))]).astype(np.int32)


def upload(arrays, device='cuda'):
    """One host-to-device copy for a dict of numpy arrays -> dict of device tensors (views of one buffer, 16-byte aligned)."""
    import torch
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    at, size = {}, 0
    for k, v in arrays.items():
        at[k] = size
        size += (v.nbytes + 15) // 16 * 16
    host = np.zeros(max(size, 16), np.uint8)
    for k, v in arrays.items():
        host[at[k]:at[k] + v.nbytes] = v.reshape(-1).view(np.uint8)
    buf = torch.from_numpy(host).to(torch.device(device))
    return {k: buf[at[k]:at[k] + v.nbytes].view(getattr(torch, v.dtype.name)).view(v.shape) for k, v in arrays.items()}


def match_device(t, grid=0, out=None, timer=None):
    """fpd_coco_match over device tensors `t`: gt_kpts [G,J,3], gt_area, gt_bbox, gt_flags, dt_kpts [D,J,3], gt_offsets,
    dt_offsets (int32), oks_offsets (int64, the last entry the size of the OKS buffer), sigmas [J]
    -> dict of device tensors oks, matched [3,10,D], dt_ignored [3,10,D] (uint8), gt_counted [3,n_img], dt_area [D], status
    [n_img] (include/fpd_amd.h fpd_coco_match_t); `out`: tensors to write into instead of fresh ones."""
    import torch
    R = _R()
    dev = t['sigmas'].device
    n_img, j = t['gt_offsets'].numel() - 1, t['sigmas'].numel()
    g_total, d_total = t['gt_area'].numel(), t['dt_kpts'].shape[0]
    oks_total = int(t['oks_total'])
    na, nt = len(AREA_RANGES), len(OKS_THRS)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    o = dict(out or {})
    for k, shape, dtype in (('oks', (oks_total,), torch.float64), ('scratch', (1 + na * nt, g_total), torch.uint8),
                            ('matched', (na, nt, d_total), torch.uint8), ('dt_ignored', (na, nt, d_total), torch.uint8),
                            ('gt_counted', (na, n_img), torch.int32), ('dt_area', (d_total,), torch.float64),
                            ('status', (n_img,), torch.int32)):
        if k not in o:
            o[k] = new(shape, dtype)
    a = R.CocoMatchT()
    a.n_img, a.J, a.G_total, a.D_total, a.grid, a.oks_total = n_img, j, g_total, d_total, int(grid), oks_total
    for r, (lo, hi) in enumerate(AREA_RANGES):
        a.area_lo[r], a.area_hi[r] = float(lo), float(hi)
    for k, thr in enumerate(OKS_THRS):
        a.oks_thrs[k] = float(thr)
    for k in ('gt_kpts', 'gt_area', 'gt_bbox', 'gt_flags', 'dt_kpts', 'gt_offsets', 'dt_offsets', 'oks_offsets', 'sigmas'):
        setattr(a, k, t[k].data_ptr())
    for k in ('oks', 'scratch', 'matched', 'dt_ignored', 'gt_counted', 'dt_area', 'status'):
        setattr(a, k, o[k].data_ptr())

    def launch():
        with torch.cuda.device(dev):
            R.check(R.lib().fpd_coco_match(a, R.current_stream()), 'fpd_coco_match')
    (timer or (lambda f: f()))(launch)
    return o


def accumulate_device(matched, dt_ignored, order, npig, rec_thrs, timer=None):
    """fpd_coco_accumulate over device tensors: the flags [3,10,D] (uint8), order [D] int32 (rank -> detection), npig [3] int32,
    rec_thrs [R] float64 -> device tensors (precision [10,R,3], recall [10,3], status [30])."""
    import torch
    R = _R()
    dev = matched.device
    na, nt, d_total = matched.shape
    precision = torch.empty((nt, rec_thrs.numel(), na), dtype=torch.float64, device=dev)
    recall = torch.empty((nt, na), dtype=torch.float64, device=dev)
    status = torch.empty(na * nt, dtype=torch.int32, device=dev)
    tp = torch.empty((na, nt, d_total), dtype=torch.int32, device=dev)
    env = torch.empty((na, nt, d_total), dtype=torch.float64, device=dev)
    a = R.CocoAccumT()
    a.D_total, a.n_rec = d_total, rec_thrs.numel()
    a.matched, a.dt_ignored, a.order, a.npig, a.rec_thrs = (matched.data_ptr(), dt_ignored.data_ptr(), order.data_ptr(),
                                                            npig.data_ptr(), rec_thrs.data_ptr())
    a.tp, a.env, a.precision, a.recall, a.status = tp.data_ptr(), env.data_ptr(), precision.data_ptr(), recall.data_ptr(), status.data_ptr()

    def launch():
        with torch.cuda.device(dev):
            R.check(R.lib().fpd_coco_accumulate(a, R.current_stream()), 'fpd_coco_accumulate')
    (timer or (lambda f: f()))(launch)
    return precision, recall, status


def _ten_stats(precision, recall):
    """precision [T,R,K,A], recall [T,K,A] -> the ten statistics, with evaluate_keypoints' own expressions."""
    t50, t75 = int(np.argmin(np.abs(OKS_THRS - 0.5))), int(np.argmin(np.abs(OKS_THRS - 0.75)))
    return np.array([_mean(precision[:, :, :, 0]), _mean(precision[t50, :, :, 0]), _mean(precision[t75, :, :, 0]),
                     _mean(precision[:, :, :, 1]), _mean(precision[:, :, :, 2]),
                     _mean(recall[:, :, 0]), _mean(recall[t50, :, 0]), _mean(recall[t75, :, 0]),
                     _mean(recall[:, :, 1]), _mean(recall[:, :, 2])], np.float64)


def evaluate_arrays_device(packed_gt, dt_image_ids, dt_kpts, dt_scores, device='cuda', grid=0, return_tables=False, sigmas=SIGMAS,
                           timer=None):
    """The ten statistics of evaluate_keypoints from arrays: packed_gt of pack_ground_truth, and the detections in the order
    of the results file (dt_image_ids [N], dt_kpts [N,3J] or [N,J,3], dt_scores [N]).  The grouping and the cut to the 20
    best per picture (numpy, whole arrays), one upload, fpd_coco_match, npig by one device reduction, torch.sort,
    fpd_coco_accumulate, one download of the two tables, the means.  return_tables: also precision [10,101,1,3] and recall
    [10,1,3].  timer: {'match': f, 'accumulate': f}, each given its launch as a thunk (tools/coco_eval_bench.py)."""
    R = _R()
    sig = np.ascontiguousarray(sigmas, np.float64).reshape(-1)
    j = sig.size
    gt_kpts = packed_gt['gt_kpts']
    g_total = gt_kpts.shape[0]
    if g_total and gt_kpts.shape[1] != j:
        raise R.FpdError('coco_eval: %d sigmas for gts of %d joints' % (j, gt_kpts.shape[1]))
    if not 1 <= j <= 64:
        raise R.FpdError('coco_eval: %d joints outside 1..64' % j)
    gt_offsets = np.asarray(packed_gt['gt_offsets'])
    _check_offsets(gt_offsets, g_total, 'gt')
    n_img = gt_offsets.size - 1
    if n_img != len(packed_gt['image_ids']):
        raise R.FpdError('coco_eval: %d pictures, %d gt offsets' % (len(packed_gt['image_ids']), gt_offsets.size))
    scores = np.asarray(dt_scores, np.float64).reshape(-1)
    kpts = np.asarray(dt_kpts, np.float64)
    if kpts.size != scores.size * j * 3:
        raise R.FpdError('coco_eval: detections of shape %s for %d scores and %d joints' % (kpts.shape, scores.size, j))
    rows, dt_offsets = group_detections(packed_gt['image_ids'], dt_image_ids, scores)
    nt, nr, na = len(OKS_THRS), len(REC_THRS), len(AREA_RANGES)
    if n_img == 0:
        precision, recall = -np.ones((nt, nr, 1, na)), -np.ones((nt, 1, na))
        return (_ten_stats(precision, recall), precision, recall) if return_tables else _ten_stats(precision, recall)
    import torch
    pairs = np.diff(dt_offsets).astype(np.int64) * np.diff(gt_offsets).astype(np.int64)
    oks_offsets = np.concatenate([[0], np.cumsum(pairs)]).astype(np.int64)
    t = upload({'gt_kpts': gt_kpts.reshape(g_total, j, 3), 'gt_area': packed_gt['gt_area'], 'gt_bbox': packed_gt['gt_bbox'],
                'dt_kpts': kpts.reshape(scores.size, j, 3)[rows], 'scores': scores[rows], 'sigmas': sig, 'rec_thrs': REC_THRS,
                'oks_offsets': oks_offsets, 'gt_offsets': gt_offsets.astype(np.int32), 'dt_offsets': dt_offsets,
                'gt_flags': packed_gt['gt_flags']}, device)
    t['oks_total'] = int(oks_offsets[-1])
    timer = timer or {}
    m = match_device(t, grid=grid, timer=timer.get('match'))
    npig = m['gt_counted'].sum(dim=1, dtype=torch.int32)
    order = torch.sort(t['scores'], stable=True, descending=True).indices.to(torch.int32)
    precision, recall, status = accumulate_device(m['matched'], m['dt_ignored'], order, npig, t['rec_thrs'], timer=timer.get('accumulate'))
    back = torch.cat([precision.reshape(-1), recall.reshape(-1), m['status'].min().reshape(1).double(),
                      status.min().reshape(1).double()]).cpu().numpy()
    if back[-2] < 0 or back[-1] < 0:
        raise R.FpdError('coco_eval: the kernel refused %s' % ('an offset table' if back[-2] < 0 else 'the order'))
    precision = back[:nt * nr * na].reshape(nt, nr, 1, na)
    recall = back[nt * nr * na:nt * nr * na + nt * na].reshape(nt, 1, na)
    stats = _ten_stats(precision, recall)
    return (stats, precision, recall) if return_tables else stats


def evaluate_keypoints_device(gts, dts, image_ids, cat_ids, sigmas=SIGMAS, device='cuda'):
    """evaluate_keypoints on the device; one category."""
    if len(cat_ids) != 1:
        raise _R().FpdError('coco_eval: the device path evaluates exactly one category, got %d' % len(cat_ids))
    cat = cat_ids[0]
    packed = pack_ground_truth(gts, image_ids, cat)
    dts = [d for d in dts if d['category_id'] == cat]
    j = np.asarray(sigmas).size
    return evaluate_arrays_device(packed, np.array([d['image_id'] for d in dts], np.int64),
                                  np.array([d['keypoints'] for d in dts], np.float64).reshape(len(dts), j * 3),
                                  np.array([d['score'] for d in dts], np.float64), device=device, sigmas=sigmas)
