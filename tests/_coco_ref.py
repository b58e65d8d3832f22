"""Rescoring and OKS NMS of COCO's evaluate restated in numpy, vectorised over the people of one picture (what
csrc/oks_nms.hip computes; held to the reference's own `oks_nms` / `soft_oks_nms` by tests/test_coco_cpu.py through the
cases of tests/golden/coco_ref.npz), plus the generator of clustered people the tests and tools/oks_nms_bench.py share.

The number formats are the kernel's: x, y differences, their squares and the sum of the two squares in float32; everything
after that in float64 with the divisions in the order  / (2 sigma)^2 / ((a_g + a_d) / 2 + 2^-52) / 2.  Equal scores: the
lower index first (a stable sort of the negated scores)."""
import numpy as np

SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
SOFT_MAX_DETS = 20
EPS = 2.0 ** -52


def rescore(kpts, box_score, in_vis_thre):
    """kpts [P,J,3] float32, box_score [P] float64 -> [P] float64: the mean of the maxvals above the threshold, summed in
    joint order in float32, times the box score in float64; 0 for a person without such a joint."""
    kpts = np.asarray(kpts, np.float32)
    m = kpts[:, :, 2]
    on = m > np.float32(in_vis_thre)
    total = np.zeros(len(kpts), np.float32)
    for j in range(kpts.shape[1]):                      # joint order matters in float32
        total = np.where(on[:, j], total + m[:, j], total).astype(np.float32)
    count = on.sum(1)
    mean = np.where(count > 0, total / np.maximum(count, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    return mean.astype(np.float64) * np.asarray(box_score, np.float64)


def oks(kpts, area, g, sigmas=SIGMAS):
    """OKS of person g with every person of the picture (g itself: 1) -> [P] float64."""
    kpts = np.asarray(kpts, np.float32)
    dx = kpts[:, :, 0] - kpts[g, :, 0]
    dy = kpts[:, :, 1] - kpts[g, :, 1]
    d2 = (dx * dx + dy * dy).astype(np.float32)
    area = np.asarray(area, np.float64)
    e = d2.astype(np.float64) / ((np.asarray(sigmas, np.float64) * 2) ** 2)[None, :] / ((area[g] + area) / 2 + EPS)[:, None] / 2
    return np.exp(-e).sum(1) / kpts.shape[1]


def _best(work, present):
    idx = np.flatnonzero(present)
    return int(idx[np.argsort(-work[idx], kind='stable')[0]])


def hard_nms(kpts, area, score, thresh, sigmas=SIGMAS):
    """-> list of picks: the best person present, then everyone present with oks > thresh leaves."""
    present = np.ones(len(score), bool)
    keep = []
    while present.any():
        g = _best(np.asarray(score, np.float64), present)
        keep.append(g)
        present &= ~(oks(kpts, area, g, sigmas) > thresh)
        present[g] = False
    return keep


def soft_nms(kpts, area, score, thresh, sigmas=SIGMAS, trace=None):
    """-> list of at most 20 picks; after each the working scores of the rest decay by exp(-oks^2 / thresh).
    trace: a list that receives the working scores of the people not yet picked at every pick (the fixture's margins)."""
    work = np.array(score, np.float64)
    present = np.ones(len(work), bool)
    keep = []
    while present.any() and len(keep) < SOFT_MAX_DETS:
        if trace is not None:
            trace.append(work[present].copy())
        g = _best(work, present)
        keep.append(g)
        present[g] = False
        o = oks(kpts, area, g, sigmas)
        work = np.where(present, work * np.exp(-o ** 2 / thresh), work)
    return keep


def nms_pictures(kpts, area, box_score, offsets, in_vis_thre, oks_thre, soft):
    """Rescoring + NMS of every picture -> (score [P], keep [P] int32 padded with -1 per picture, n_keep [n_img])."""
    score = rescore(kpts, box_score, in_vis_thre)
    keep = np.full(len(score), -1, np.int32)
    n_keep = np.zeros(len(offsets) - 1, np.int32)
    for i in range(len(offsets) - 1):
        a, b = int(offsets[i]), int(offsets[i + 1])
        k = (soft_nms if soft else hard_nms)(kpts[a:b], area[a:b], score[a:b], oks_thre)
        keep[a:a + len(k)] = k
        n_keep[i] = len(k)
    return score, keep, n_keep


def margins(kpts, area, score, thresh):
    """(smallest |oks - thresh| over the comparisons of the hard NMS, smallest relative gap between two scores, smallest
    relative gap between two soft working scores that compete at a pick)."""
    oks_gap, present = np.inf, np.ones(len(score), bool)
    while present.any():
        g = _best(score, present)
        present[g] = False
        o = oks(kpts, area, g)
        if present.any():
            oks_gap = min(oks_gap, float(np.abs(o[present] - thresh).min()))
        present &= ~(o > thresh)

    def rel_gap(v):
        v = np.sort(np.asarray(v, np.float64))
        return float(((v[1:] - v[:-1]) / np.maximum(np.abs(v[1:]), 1e-300)).min()) if len(v) > 1 else np.inf
    trace = []
    soft_nms(kpts, area, score, thresh, trace=trace)
    return oks_gap, rel_gap(score), min([rel_gap(w) for w in trace] + [np.inf])


def clustered_people(rng, p, j=17):
    """p people around p // 4 (at least 1) base poses: jitter of 0.5 .. 6 px per person, areas 4e4 .. 1.2e5, maxvals and box
    scores in (0.05, 1) -> (kpts [p,j,3] float32, area [p] float64, box_score [p] float64)."""
    n_base = max(p // 4, 1)
    base = rng.uniform(20, 620, (n_base, 1, 2)) + rng.uniform(-90, 90, (n_base, j, 2))
    which = rng.integers(0, n_base, p)
    jitter = rng.uniform(0.5, 6.0, (p, 1, 1))
    kpts = np.zeros((p, j, 3), np.float32)
    kpts[:, :, 0:2] = base[which] + rng.standard_normal((p, j, 2)) * jitter
    kpts[:, :, 2] = rng.uniform(0.05, 1.0, (p, j))
    return kpts, rng.uniform(4e4, 1.2e5, p), rng.uniform(0.05, 1.0, p)
