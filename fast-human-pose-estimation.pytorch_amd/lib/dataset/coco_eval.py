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
