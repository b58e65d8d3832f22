#!/usr/bin/env python
"""Golden vectors of the MPII dataset class, produced by the REFERENCE's own `MPIIDataset._get_db` and `.evaluate`
(/root/reference/lib/dataset/mpii.py:56-194, imported by file path; build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mpii.py

The reference class runs as it is.  What it needs and this container lacks is stubbed: `np.float` (removed from numpy),
`json_tricks` (its `load` is the standard library's here), cv2 and torchvision (imported, never called on this path), and
the `dataset` package is registered empty so that its __init__ does not pull in coco.py (pycocotools).  The pickle cache
of the record list goes to a temporary DATASET.CACHE_ROOT.

Inputs (stored as in_*): 12 people over 5 images, one of them with the centre placeholder [-1, -1], mixed joints_vis, the
four arrays of gt_valid.mat, and predictions = annotation + noise of up to one head-size threshold, so that joints fall on
both sides of PCKh's 0.5.  PRECONDITION: no scaled error of an annotated joint lies within 1e-6 of any of the 51
thresholds (tests/_mpii_tree.threshold_margin), so the <= of the sweep cannot flip with the last bits of a norm; SEED is
advanced until that holds and the seed found is printed.

Outputs: every field of `db` for the valid and test sets (image paths relative to the root), the keys and values of
name_value, the indicator, and `preds` read back from pred.mat.  An existing mpii_ref.npz is compared array by array
before it is replaced."""
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

from tests import _mpii_tree as T  # noqa: E402

SEED = 0
PEOPLE = (0, 1, 0, 2, 3, 2, 4, 0, 4, 1, 2, 4)          # the image of each person
PLACEHOLDER = 5                                        # the person whose centre is [-1, -1]


def make_inputs(seed):
    rng = np.random.default_rng(seed)
    n = len(PEOPLE)
    hw = np.array([T.IMAGE_SHAPES[k] for k in PEOPLE], np.float64)
    center = np.round(hw[:, ::-1] * rng.uniform(0.35, 0.65, (n, 2)))
    scale = np.round(rng.uniform(0.3, 0.55, n), 3)
    joints = np.round(center[:, None, :] + rng.standard_normal((n, 16, 2)) * scale[:, None, None] * 40, 3)
    vis = (rng.random((n, 16)) < 0.8).astype(np.int64)
    vis[3, :10] = 0                                    # a person with 6 annotated joints at the most
    center[PLACEHOLDER] = -1
    corner = joints[:, 9, :] - rng.uniform(8, 20, (n, 2))
    head = np.stack([corner, corner + rng.uniform(18, 40, (n, 2))])                  # [2 corners, N, xy]
    g = {'in_image': np.array(['im%d.npy' % k for k in PEOPLE]), 'in_center': center, 'in_scale': scale, 'in_joints': joints,
         'in_joints_vis': vis, 'in_jnt_missing': (1 - vis.T).astype(np.uint8),
         'in_pos_gt_src': np.ascontiguousarray(joints.transpose(1, 2, 0)),
         'in_headboxes_src': np.ascontiguousarray(head.transpose(0, 2, 1))}
    size = np.linalg.norm(head[1] - head[0], axis=1) * 0.6                            # [N]
    angle, radius = rng.uniform(0, 2 * np.pi, (n, 16)), rng.uniform(0, 1, (n, 16)) * size[:, None]
    preds = np.zeros((n, 16, 3), np.float32)
    preds[:, :, 0:2] = joints - 1 + radius[..., None] * np.stack([np.cos(angle), np.sin(angle)], -1)
    preds[:, :, 2] = rng.uniform(0.1, 1, (n, 16))
    g['in_preds'] = preds
    return g


def acceptable(g):
    e, visible = T.scaled_errors(g)
    both = (e[visible] < 0.5).sum() > 10 and (e[visible] > 0.5).sum() > 10
    return T.threshold_margin(g) >= 1e-6 and visible.any(axis=1).all() and both


def reference_class():
    np.float = float
    jt = types.ModuleType('json_tricks')
    jt.load = json.load
    sys.modules['json_tricks'] = jt
    for name in ('cv2', 'torchvision', 'torchvision.transforms'):
        sys.modules.setdefault(name, types.ModuleType(name))
    pkg = types.ModuleType('dataset')
    pkg.__path__ = [os.path.join(REF, 'dataset')]
    sys.modules['dataset'] = pkg
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location('dataset.mpii', os.path.join(REF, 'dataset', 'mpii.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MPIIDataset


def main():
    seed = SEED
    while not acceptable(make_inputs(seed)):
        seed += 1
    if seed != SEED:
        print('set SEED = %d in tests/golden/make_golden_mpii.py and run again' % seed)
        sys.exit(1)
    g = make_inputs(seed)
    e, visible = T.scaled_errors(g)
    print('seed %d: threshold margin %.3g; %d annotated joints within 0.5, %d beyond' % (
        seed, T.threshold_margin(g), (e[visible] <= 0.5).sum(), (e[visible] > 0.5).sum()))
    MPIIDataset = reference_class()
    res = dict(g)
    with tempfile.TemporaryDirectory() as tmp:
        root = T.write_tree(os.path.join(tmp, 'mpii'), g, gt=True, images=False)
        cfg = T.make_cfg(root, CACHE_ROOT=os.path.join(tmp, 'cache'))
        for image_set in ('valid', 'test'):
            ds = MPIIDataset(cfg, root, image_set, False)
            assert len(ds.db) == len(PEOPLE)
            for k in ('center', 'scale', 'joints_3d', 'joints_3d_vis'):
                res['%s/%s' % (image_set, k)] = np.stack([rec[k] for rec in ds.db])
                assert res['%s/%s' % (image_set, k)].dtype == np.float64
            res[image_set + '/image'] = np.array([os.path.relpath(rec['image'], root) for rec in ds.db])
            res[image_set + '/filename'] = np.array([rec['filename'] for rec in ds.db])
            res[image_set + '/imgnum'] = np.array([rec['imgnum'] for rec in ds.db])
            if image_set == 'valid':
                out = os.path.join(tmp, 'out')
                os.makedirs(out)
                name_value, indicator = ds.evaluate(cfg, g['in_preds'], out)
                from scipy.io import loadmat
                res['pred_mat'] = loadmat(os.path.join(out, 'pred.mat'))['preds']
        res['name_value_keys'] = np.array(list(name_value.keys()))
        res['name_value_values'] = np.array([float(v) for v in name_value.values()], np.float64)
        res['indicator'] = np.float64(indicator)
    print(dict(zip(res['name_value_keys'].tolist(), res['name_value_values'].tolist())))
    if os.path.exists(T.GOLDEN):
        old = T.load_golden()
        same = sorted(old) == sorted(res) and all(
            old[k].dtype == np.asarray(res[k]).dtype and np.array_equal(old[k], res[k]) for k in res)
        print('existing mpii_ref.npz: %s' % ('every array identical' if same else 'DIFFERS'))
    np.savez_compressed(T.GOLDEN, **res)
    print('wrote mpii_ref.npz: %d arrays, %.1f KB' % (len(res), os.path.getsize(T.GOLDEN) / 1e3))


if __name__ == '__main__':
    main()
