#!/usr/bin/env python
"""Golden vectors of the COCO dataset class and of the OKS NMS, produced by the REFERENCE's own `COCODataset._get_db`,
`.evaluate`, `oks_nms`, `soft_oks_nms` and `oks_iou` (/root/reference/lib/dataset/coco.py, lib/nms/nms.py, imported by
file path; build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_coco.py

The reference code runs as it is.  What it needs and this container lacks is stubbed: `np.float` (removed from numpy),
`json_tricks` (`load` / `dump` are the standard library's here, numpy scalars written as plain numbers), cv2 and torchvision
(imported, never called on this path), empty `nms.cpu_nms` / `nms.gpu_nms` (Cython / CUDA extensions nothing calls), and
`pycocotools.coco` / `pycocotools.cocoeval`.  The `COCO` stand-in is the few lines over `json` below; that it hands out
image ids, annotations and categories in FILE ORDER is OUR ASSUMPTION about pycocotools (its dictionaries are filled in
file order), which nothing here can check.  `_do_python_keypoint_eval` is replaced by a no-op that returns zeros: the AP
table is not part of this fixture.  The pickle cache of the record list goes to a temporary DATASET.CACHE_ROOT.

Contents (inputs stored as in_*):
  (a) db/<case>/...      every field of `db` for train2017, val2017 with ground-truth boxes, val2017 with the detection file
  (b) res/<hard|soft>/...  the results list the reference's `evaluate` wrote for in_preds / in_boxes / in_paths
  (c) nms/<P>/...        for P in 1, 2, 3, 17, 65, 130, 257 clustered people (tests/_coco_ref.clustered_people): inputs, the
                         rescored values, the keep lists of oks_nms / soft_oks_nms and the OKS of everyone with the top person

PRECONDITIONS, asserted; SEED is advanced until they hold and the seed found is printed:
  - no OKS that a decision compares lies within 1e-6 of the threshold (hard NMS: every pick against everyone present);
  - no two scores of a picture are equal, and no two soft working scores that compete at a pick are closer than 1e-9 relative;
  - in every case with P >= 17 at least a fifth of the people are kept and at least a fifth suppressed.
An existing coco_ref.npz is compared array by array before it is replaced."""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
REF = '/root/reference/lib'

from tests import _coco_ref as C  # noqa: E402
from tests import _coco_tree as T  # noqa: E402

SEED = 0
THRESH, IN_VIS_THRE = 0.9, 0.2


class COCO:
    """The five calls coco.py makes, in file order (see the module docstring)."""

    def __init__(self, path=None):
        with open(path) as f:
            self.dataset = json.load(f)
        self.imgs = {im['id']: im for im in self.dataset.get('images', [])}
        self.anns = {a['id']: a for a in self.dataset.get('annotations', [])}
        self.cats = {c['id']: c for c in self.dataset.get('categories', [])}

    def getCatIds(self):
        return list(self.cats)

    def loadCats(self, ids):
        return [self.cats[i] for i in ids]

    def getImgIds(self):
        return list(self.imgs)

    def loadImgs(self, i):
        return [self.imgs[i]]

    def getAnnIds(self, imgIds, iscrowd=None):
        return [a['id'] for a in self.anns.values() if a['image_id'] == imgIds and (iscrowd is None or a['iscrowd'] == iscrowd)]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]


def _plain(o):
    if isinstance(o, np.generic):
        return o.item()
    if isinstance(o, np.ndarray):
        return o.tolist()
    raise TypeError(type(o))


def reference_modules():
    np.float = float
    jt = types.ModuleType('json_tricks')
    jt.load = json.load
    jt.dump = lambda obj, f, **kw: json.dump(obj, f, default=_plain, **kw)
    sys.modules['json_tricks'] = jt
    for name in ('cv2', 'torchvision', 'torchvision.transforms', 'pycocotools', 'pycocotools.coco', 'pycocotools.cocoeval',
                 'nms.cpu_nms', 'nms.gpu_nms'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['pycocotools.coco'].COCO = COCO
    sys.modules['pycocotools.cocoeval'].COCOeval = None
    sys.modules['nms.cpu_nms'].cpu_nms = sys.modules['nms.gpu_nms'].gpu_nms = None
    for pkg_name in ('dataset', 'nms'):
        pkg = types.ModuleType(pkg_name)
        pkg.__path__ = [os.path.join(REF, pkg_name)]
        sys.modules[pkg_name] = pkg
    sys.path.insert(0, REF)
    mods = {}
    for name in ('nms.nms', 'dataset.coco'):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *name.split('.')) + '.py')
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[name]
        spec.loader.exec_module(mods[name])
    ds = mods['dataset.coco'].COCODataset
    ds._do_python_keypoint_eval = lambda self, res_file, res_folder: [(n, 0.0) for n in
                                                                      ('AP', 'Ap .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)')]
    return ds, mods['nms.nms']


def make_tree_inputs(seed):
    """12 annotations over the 5 pictures, and 14 detection boxes."""
    rng = np.random.default_rng(seed)
    ann_image = np.array([0, 0, 1, 1, 1, 2, 2, 3, 3, 4, 4, 4])
    n = len(ann_image)
    hw = np.array([T.IMAGE_SHAPES[k] for k in ann_image], np.float64)
    wh = np.round(hw[:, ::-1] * rng.uniform(0.3, 0.6, (n, 2)), 2)
    xy = np.round((hw[:, ::-1] - wh) * rng.uniform(0.05, 0.9, (n, 2)), 2)
    bbox = np.concatenate([xy, wh], 1)
    kp = np.zeros((n, 17, 3), np.int64)
    kp[:, :, 0:2] = np.round(xy[:, None, :] + wh[:, None, :] * rng.uniform(0.05, 0.95, (n, 17, 2)))
    kp[:, :, 2] = rng.integers(0, 3, (n, 17))
    kp[kp[:, :, 2] == 0] = 0
    area = np.round(wh[:, 0] * wh[:, 1] * 0.6, 2)
    iscrowd = np.zeros(n, np.int64)
    iscrowd[3] = 1                                                   # a crowd annotation
    area[5] = 0.0                                                    # a zero-area box
    bbox[7, 0:2] = (-6.5, hw[7, 0] - bbox[7, 3] + 9.25)              # reaches outside the picture (left and bottom)
    kp[9] = 0                                                        # a person without keypoints
    bbox[10] = np.round(bbox[10])                                    # integer-valued box numbers
    g = {'in_ann_image': ann_image, 'in_ann_bbox': bbox, 'in_ann_area': area, 'in_ann_iscrowd': iscrowd,
         'in_ann_keypoints': kp.reshape(n, 51)}
    det_image = np.array([0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 4, 4])
    m = len(det_image)
    dhw = np.array([T.IMAGE_SHAPES[k] for k in det_image], np.float64)
    dwh = np.round(dhw[:, ::-1] * rng.uniform(0.3, 0.6, (m, 2)), 2)
    dxy = np.round((dhw[:, ::-1] - dwh) * rng.uniform(0.0, 1.0, (m, 2)), 2)
    score = np.round(rng.uniform(0.15, 0.99, m), 4)
    cat = np.ones(m, np.int64)
    cat[4] = 3                                                       # not a person
    score[9] = 0.05                                                  # below IMAGE_THRE = 0.1
    g.update({'in_det_image': det_image, 'in_det_category': cat, 'in_det_bbox': np.concatenate([dxy, dwh], 1), 'in_det_score': score})
    return g


def make_eval_inputs(seed, db, root):
    """preds / all_boxes / paths of an `evaluate` call over the detection-box db: every box three times (the second and
    third as jittered copies), so that pictures hold close and distant people."""
    rng = np.random.default_rng(seed + 77)
    rows = np.repeat(np.arange(len(db)), 3)
    rng.shuffle(rows)
    n = len(rows)
    center = np.stack([db[r]['center'] for r in rows]).astype(np.float64)
    scale = np.stack([db[r]['scale'] for r in rows]).astype(np.float64)
    base = {r: center[list(rows).index(r)][None, :] + rng.uniform(-30, 30, (17, 2)) for r in set(rows.tolist())}
    preds = np.zeros((n, 17, 3), np.float32)
    preds[:, :, 0:2] = np.stack([base[r] for r in rows.tolist()]) + rng.standard_normal((n, 17, 2)) * rng.uniform(0.3, 5.0, (n, 1, 1))
    preds[:, :, 2] = rng.uniform(0.05, 1.0, (n, 17))
    boxes = np.zeros((n, 6))
    boxes[:, 0:2], boxes[:, 2:4] = center, scale
    boxes[:, 4] = np.prod(scale * 200, 1)
    boxes[:, 5] = np.array([db[r]['score'] for r in rows]) * rng.uniform(0.8, 1.0, n)
    paths = np.array([os.path.relpath(db[r]['image'], root) for r in rows])
    return preds, boxes, paths


def picture_groups(paths):
    ids = [int(p[-16:-4]) for p in paths]
    order = list(dict.fromkeys(ids))
    return [[i for i, v in enumerate(ids) if v == pic] for pic in order]


def nms_case(seed, p):
    return C.clustered_people(np.random.default_rng([seed, p]), p)


def acceptable(seed):
    for p in T.NMS_SIZES:
        kpts, area, box = nms_case(seed, p)
        score = C.rescore(kpts, box, IN_VIS_THRE)
        og, sg, wg = C.margins(kpts, area, score, THRESH)
        kept = len(C.hard_nms(kpts, area, score, THRESH))
        if og < 1e-6 or sg <= 0 or wg < 1e-9 or (p >= 17 and not (kept * 5 >= p and (p - kept) * 5 >= p)):
            return False
    return True


def main():
    seed = SEED
    while not acceptable(seed):
        seed += 1
    if seed != SEED:
        print('set SEED = %d in tests/golden/make_golden_coco.py and run again' % seed)
        sys.exit(1)
    COCODataset, nms = reference_modules()
    g = make_tree_inputs(seed)
    res = dict(g)
    with tempfile.TemporaryDirectory() as tmp:
        root = T.write_tree(os.path.join(tmp, 'coco'), g, images=False)
        cases = (('train', 'train2017', True, {}), ('val_gt', 'val2017', False, {'USE_GT_BBOX': True}),
                 ('val_det', 'val2017', False, {'USE_GT_BBOX': False}))
        for k, (name, image_set, is_train, test) in enumerate(cases):
            cfg = T.make_cfg(root, test=test, CACHE_ROOT=os.path.join(tmp, 'cache%d' % k))
            ds = COCODataset(cfg, root, image_set, is_train)
            for key, v in T.db_arrays(ds.db, root).items():
                res['db/%s/%s' % (name, key)] = v
            print('%s: %d records' % (name, len(ds.db)))
        assert len(res['db/train/image']) == 9 and len(res['db/val_det/image']) == 12           # 12 - crowd - zero area - no keypoints / 14 - 2
        preds, boxes, paths = make_eval_inputs(seed, ds.db, root)
        for idx in picture_groups(paths):
            score = C.rescore(preds[idx], boxes[idx, 5], IN_VIS_THRE)
            og, sg, wg = C.margins(preds[idx], boxes[idx, 4], score, THRESH)
            assert og >= 1e-6 and sg > 0 and wg >= 1e-9, ('evaluate inputs', og, sg, wg)
        res.update({'in_preds': preds, 'in_boxes': boxes, 'in_paths': paths})
        for mode, soft in (('hard', False), ('soft', True)):
            cfg = T.make_cfg(root, test={'USE_GT_BBOX': False, 'SOFT_NMS': soft}, CACHE_ROOT=os.path.join(tmp, 'cache2'))
            ds = COCODataset(cfg, root, 'val2017', False)
            out = os.path.join(tmp, 'out_' + mode)
            ds.evaluate(cfg, preds.copy(), out, boxes.copy(), [os.path.join(root, p) for p in paths])
            with open(os.path.join(out, 'results', 'keypoints_val2017_results_0.json')) as f:
                results = json.load(f)
            for key, v in T.results_arrays(results).items():
                res['res/%s/%s' % (mode, key)] = v
            print('%s: %d of %d people written' % (mode, len(results), len(preds)))
        assert len(res['res/hard/score']) < len(res['res/soft/score']) <= len(preds)
    for p in T.NMS_SIZES:
        kpts, area, box = nms_case(seed, p)
        score = C.rescore(kpts, box, IN_VIS_THRE)
        db = [{'keypoints': kpts[i], 'area': area[i], 'score': score[i]} for i in range(p)]
        hard = np.array(nms.oks_nms(db, THRESH), np.int64)
        soft = np.array(nms.soft_oks_nms(db, THRESH), np.int64)
        top = int(np.argmax(score))
        flat = kpts.reshape(p, -1)
        oks_top = nms.oks_iou(flat[top], flat, area[top], area)
        og, sg, wg = C.margins(kpts, area, score, THRESH)
        print('P %3d: kept %3d (%.0f %%), soft %2d; margins oks %.2e score %.2e soft %.2e' % (
            p, len(hard), 100.0 * len(hard) / p, len(soft), og, sg, wg))
        res.update({'nms/%d/kpts' % p: kpts, 'nms/%d/area' % p: area, 'nms/%d/box_score' % p: box, 'nms/%d/score' % p: score,
                    'nms/%d/hard' % p: hard, 'nms/%d/soft' % p: soft, 'nms/%d/oks_top' % p: oks_top})
    res['nms/thresh'], res['nms/in_vis_thre'] = np.float64(THRESH), np.float64(IN_VIS_THRE)
    if os.path.exists(T.GOLDEN):
        old = T.load_golden()
        same = sorted(old) == sorted(res) and all(
            old[k].dtype == np.asarray(res[k]).dtype and np.array_equal(old[k], res[k]) for k in res)
        print('existing coco_ref.npz: %s' % ('every array identical' if same else 'DIFFERS'))
    np.savez_compressed(T.GOLDEN, **res)
    print('wrote coco_ref.npz: %d arrays, %.1f KB' % (len(res), os.path.getsize(T.GOLDEN) / 1e3))


if __name__ == '__main__':
    main()
