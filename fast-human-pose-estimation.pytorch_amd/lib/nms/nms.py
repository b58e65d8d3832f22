"""`nms.nms` of the reference (/root/reference/lib/nms/nms.py:75-177) with its names, signatures and return types, run on
the device: every function here uploads its people, issues ONE launch of csrc/oks_nms.hip (fpd_oks_nms) and downloads.

    oks_iou(g, d, a_g, a_d)          float64 [len(d)]: the OKS of `g` with every row of `d`
    oks_nms(kpts_db, thresh)         list of indices kept by the hard greedy NMS
    soft_oks_nms(kpts_db, thresh)    np.intp array: the at most 20 picks of the soft NMS
    oks_nms_device(...)              what COCODataset.evaluate calls: rescoring + NMS of every picture in one launch

Equal scores are picked lower index first (numpy's argsort leaves the order of ties unspecified).  `in_vis_thre` of the
three reference functions selects joints by a Python expression (`list(a) and list(b)`) that nothing in the reference ever
reaches -- coco.py never passes it -- so it is not restated: passing one raises.  Box `nms`, `cpu_nms` and `gpu_nms` are
not built; nothing in the reference calls them."""
import numpy as np

from ... import runtime as R

SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


def _sigmas(sigmas, j):
    s = np.ascontiguousarray(sigmas if isinstance(sigmas, np.ndarray) else SIGMAS, np.float64).reshape(-1)
    if s.size != j:
        raise R.FpdError('oks: %d sigmas for %d joints' % (s.size, j))
    return s


def oks_nms_device(kpts, area, box_score, offsets, oks_thre, soft=False, in_vis_thre=0.0, sigmas=None, rescore=True,
                   grid=0, want_oks=False, device='cuda', timer=None):
    """kpts [P,J,3] (x, y, maxval), area [P], box_score [P], offsets [n_img+1] (the people of a picture are contiguous)
    -> (score [P] float64, keep [P] int32, n_keep [n_img] int32[, oks_first [P] float64]) as numpy arrays; see
    include/fpd_amd.h fpd_oks_nms_t.  One upload, one launch, one download, no host work per picture.
    timer: a callable given the launch as a thunk (tools/oks_nms_bench.py times the launch alone with it)."""
    import torch
    kpts = np.ascontiguousarray(kpts, np.float32)
    if kpts.ndim != 3 or kpts.shape[2] != 3:
        raise R.FpdError('oks_nms: kpts must be [P,J,3], got %s' % (kpts.shape,))
    p, j = kpts.shape[0], kpts.shape[1]
    area = np.ascontiguousarray(area, np.float64).reshape(-1)
    box_score = np.ascontiguousarray(box_score, np.float64).reshape(-1)
    offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
    if area.size != p or box_score.size != p:
        raise R.FpdError('oks_nms: %d people, %d areas, %d scores' % (p, area.size, box_score.size))
    if offsets.size < 1 or offsets[0] != 0 or offsets[-1] != p or (np.diff(offsets) < 0).any() or p >= 2 ** 31:
        raise R.FpdError('oks_nms: offsets must rise from 0 to the number of people (%d)' % p)
    n_img = offsets.size - 1
    sig = _sigmas(sigmas, j)
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    d_kpts, d_area, d_box, d_off, d_sig = up(kpts), up(area), up(box_score), up(offsets.astype(np.int32)), up(sig)
    score = torch.empty(p, dtype=torch.float64, device=dev)
    work = torch.empty(p, dtype=torch.float64, device=dev)
    keep = torch.empty(p, dtype=torch.int32, device=dev)
    n_keep = torch.empty(n_img, dtype=torch.int32, device=dev)
    oks = torch.empty(p, dtype=torch.float64, device=dev) if want_oks else None
    a = R.OksNmsT()
    a.P_total, a.n_img, a.J, a.soft, a.rescore, a.grid = p, n_img, j, int(bool(soft)), int(bool(rescore)), int(grid)
    a.in_vis_thre, a.oks_thre = float(in_vis_thre), float(oks_thre)
    a.kpts, a.area, a.box_score, a.offsets, a.sigmas = (d_kpts.data_ptr(), d_area.data_ptr(), d_box.data_ptr(),
                                                        d_off.data_ptr(), d_sig.data_ptr())
    a.score, a.work, a.keep, a.n_keep = score.data_ptr(), work.data_ptr(), keep.data_ptr(), n_keep.data_ptr()
    if oks is not None:
        a.oks_first = oks.data_ptr()

    def launch():
        with torch.cuda.device(dev):
            R.check(R.lib().fpd_oks_nms(a, R.current_stream()), 'fpd_oks_nms')
    if timer is not None:
        timer(launch)
    else:
        launch()
    out = (score.cpu().numpy(), keep.cpu().numpy(), n_keep.cpu().numpy())
    if (out[2] < 0).any():
        raise R.FpdError('fpd_oks_nms: the kernel refused the offsets of picture %d' % int(np.flatnonzero(out[2] < 0)[0]))
    return out + ((oks.cpu().numpy(),) if oks is not None else ())


def _no_vis_thre(name, in_vis_thre):
    if in_vis_thre is not None:
        raise R.FpdError('%s: in_vis_thre is not supported (the reference never passes it)' % name)


def _db_arrays(kpts_db):
    scores = np.array([kpts_db[i]['score'] for i in range(len(kpts_db))], np.float64)
    kpts = np.array([np.asarray(kpts_db[i]['keypoints']).reshape(-1, 3) for i in range(len(kpts_db))])
    areas = np.array([kpts_db[i]['area'] for i in range(len(kpts_db))], np.float64)
    return scores, kpts, areas


def oks_iou(g, d, a_g, a_d, sigmas=None, in_vis_thre=None):
    """nms.py:75-94: g [3J] and d [n,3J] flattened (x, y, v) triplets -> float64 [n].  One picture of 1 + n people in which
    g is the first pick (the only score of 2) and, with a threshold of -1, removes everyone else: one round of the greedy loop,
    whose per-person OKS output holds the answer."""
    _no_vis_thre('oks_iou', in_vis_thre)
    g, d = np.asarray(g).reshape(-1, 3), np.asarray(d)
    n = d.shape[0]
    if n == 0:
        return np.zeros((0,))
    kpts = np.concatenate([g[None], d.reshape(n, -1, 3)]).astype(np.float32)
    area = np.concatenate([[a_g], np.asarray(a_d, np.float64).reshape(-1)])
    box = np.concatenate([[2.0], np.ones(n)])
    out = oks_nms_device(kpts, area, box, [0, n + 1], -1.0, sigmas=sigmas, rescore=False, want_oks=True)
    return out[3][1:].copy()


def oks_nms(kpts_db, thresh, sigmas=None, in_vis_thre=None):
    """nms.py:97-124 -> list of the kept indices, best first."""
    _no_vis_thre('oks_nms', in_vis_thre)
    if len(kpts_db) == 0:
        return []
    scores, kpts, areas = _db_arrays(kpts_db)
    _, keep, n_keep = oks_nms_device(kpts, areas, scores, [0, len(scores)], thresh, sigmas=sigmas, rescore=False)
    return [int(k) for k in keep[:n_keep[0]]]


def soft_oks_nms(kpts_db, thresh, sigmas=None, in_vis_thre=None):
    """nms.py:138-177 -> np.intp array of the at most 20 picks ([] for no people, like the reference)."""
    _no_vis_thre('soft_oks_nms', in_vis_thre)
    if len(kpts_db) == 0:
        return []
    scores, kpts, areas = _db_arrays(kpts_db)
    _, keep, n_keep = oks_nms_device(kpts, areas, scores, [0, len(scores)], thresh, soft=True, sigmas=sigmas, rescore=False)
    return keep[:n_keep[0]].astype(np.intp)
