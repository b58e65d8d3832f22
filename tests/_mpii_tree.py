"""A temporary MPII directory written from the inputs stored in tests/golden/mpii_ref.npz (made by
tests/golden/make_golden_mpii.py, which runs the reference's own MPIIDataset on the tree this module writes):

    annot/train.json, valid.json      the 12 people over 5 images of the fixture (one with the centre placeholder [-1, -1])
    annot/test.json                   the same people without joints
    annot/gt_valid.mat                dataset_joints, jnt_missing, pos_gt_src, headboxes_src (only with gt=True: needs scipy)
    images/im<k>.npy                  seeded noise, uint8 [h,w,3] in B,G,R order, five different odd sizes

and the quantity the fixture's precondition is about (scaled_errors / threshold_margin)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mpii_ref.npz')
IMAGE_SHAPES = ((91, 133), (157, 99), (113, 151), (129, 95), (101, 145))          # (h, w)
JOINT_NAMES = ('rank', 'rkne', 'rhip', 'lhip', 'lkne', 'lank', 'pelv', 'thor', 'neck', 'head', 'rwri', 'relb', 'rsho', 'lsho',
               'lelb', 'lwri')
INPUT_KEYS = ('in_image', 'in_center', 'in_scale', 'in_joints', 'in_joints_vis', 'in_jnt_missing', 'in_pos_gt_src',
              'in_headboxes_src', 'in_preds')
THRESHOLDS = np.arange(0, 0.5 + 0.01, 0.01)


def load_golden():
    return dict(np.load(GOLDEN))


def image(k):
    """Image k of the tree: seeded noise with three different channel planes."""
    h, w = IMAGE_SHAPES[k]
    return np.random.default_rng(1000 + k).integers(0, 256, (h, w, 3), dtype=np.uint8)


def records(g, with_joints=True):
    out = []
    for i in range(len(g['in_image'])):
        a = {'image': str(g['in_image'][i]), 'center': [float(v) for v in g['in_center'][i]], 'scale': float(g['in_scale'][i])}
        if with_joints:
            a['joints'] = [[float(v) for v in xy] for xy in g['in_joints'][i]]
            a['joints_vis'] = [int(v) for v in g['in_joints_vis'][i]]
        out.append(a)
    return out


def write_tree(root, g, gt=False, images=True):
    """g: the in_* arrays (the loaded fixture, or the generator's).  -> root"""
    root = str(root)
    os.makedirs(os.path.join(root, 'annot'), exist_ok=True)
    os.makedirs(os.path.join(root, 'images'), exist_ok=True)
    for name, with_joints in (('train', True), ('valid', True), ('test', False)):
        with open(os.path.join(root, 'annot', name + '.json'), 'w') as f:
            json.dump(records(g, with_joints), f)
    if gt:
        from scipy.io import savemat
        savemat(os.path.join(root, 'annot', 'gt_valid.mat'),
                {'dataset_joints': np.array([list(JOINT_NAMES)], dtype=object), 'jnt_missing': g['in_jnt_missing'],
                 'pos_gt_src': g['in_pos_gt_src'], 'headboxes_src': g['in_headboxes_src']})
    if images:
        for k in range(len(IMAGE_SHAPES)):
            np.save(os.path.join(root, 'images', 'im%d.npy' % k), image(k))
    return root


def scaled_errors(g):
    """The head-normalised errors of the fixture's predictions that PCKh compares with its thresholds, [16,N], and the
    mask of the annotated joints (the others are multiplied by 0 and never counted)."""
    preds = g['in_preds'][:, :, 0:2] + 1.0
    err = np.linalg.norm(np.transpose(preds, [1, 2, 0]) - g['in_pos_gt_src'], axis=1)
    head = np.linalg.norm(g['in_headboxes_src'][1] - g['in_headboxes_src'][0], axis=0) * 0.6
    return err / head[None, :], g['in_jnt_missing'] == 0


def threshold_margin(g):
    """The smallest distance between a scaled error of an annotated joint and any of the 51 thresholds."""
    e, visible = scaled_errors(g)
    return float(np.abs(e[visible][:, None] - THRESHOLDS[None, :]).min())


class AD(dict):
    __getattr__ = dict.__getitem__


def make_cfg(root, **dataset):
    """The library's default config, pointed at the tree: 16 joints, 64x64 input, PROB_HALF_BODY on."""
    from fpd_amd.lib.config import _defaults
    cfg = _defaults()
    cfg.MODEL.IMAGE_SIZE, cfg.MODEL.HEATMAP_SIZE, cfg.MODEL.NUM_JOINTS = [64, 64], [16, 16], 16
    cfg.DATASET.DATASET, cfg.DATASET.ROOT, cfg.DATASET.PROB_HALF_BODY = 'mpii', str(root), 0.3
    cfg.DATASET.merge_from_dict(dataset)
    return cfg
