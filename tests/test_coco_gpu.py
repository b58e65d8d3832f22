"""The COCO dataset on the MI355X end to end: pictures shared between the people of one picture, batches equal to those of a
private copy per person, box scores carried through `validate`, `evaluate` against the results list the reference's own
class wrote (tests/golden/coco_ref.npz), and tools/fpd_train.py + tools/test.py on a COCO directory
(lib/dataset/coco.py, lib/dataset/device_dataset.py; the tree and the fixture: tests/_coco_tree.py)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _coco_tree as T
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

G = T.load_golden()
TABLE_ROW = np.dtype([('img', '<u8'), ('h', '<i4'), ('w', '<i4'), ('row_bytes', '<i8')])
KEYS = ('input', 'target', 'target_weight', 'trans', 'joints')
STAT_NAMES = ['AP', 'Ap .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)']


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return T.write_tree(tmp_path_factory.mktemp('coco'), G)


_DBS = {}


def databases(tree):
    """(COCODataset over train2017, its device database with shared pictures, the same records over a private copy of the
    picture per person) -- made once, shared by the tests, never modified."""
    if tree not in _DBS:
        from fpd_amd.lib.dataset import COCODataset, DeviceJointsDB
        from fpd_amd.lib.dataset.mpii import read_image
        ds = COCODataset(T.make_cfg(tree), tree, 'train2017', True)
        stack = lambda k: np.stack([rec[k] for rec in ds.db])  # noqa: E731
        private = DeviceJointsDB([read_image(rec['image']) for rec in ds.db], stack('joints_3d'), stack('joints_3d_vis'), stack('center'),
                                 stack('scale'), ds.flip_pairs, ds.upper_body_ids, ds.aspect_ratio, joints_weight=ds.joints_weight,
                                 device='cuda')
        _DBS[tree] = (ds, ds.to_device('cuda'), private)
    return _DBS[tree]


def one_batch(db, cfg, is_train, idx, draws=None):
    from fpd_amd.lib.dataset import DeviceAugmentLoader
    loader = DeviceAugmentLoader(db, cfg, len(idx), is_train, shuffle=False, drop_last=False)
    x, tg, tw, meta = loader.batch(np.asarray(idx, np.int32), draws=draws)
    torch.cuda.synchronize()
    return dict(input=x, target=tg, target_weight=tw, trans=meta['trans'], joints=meta['joints'], meta=meta)


def test_to_device_shares_pictures_and_gives_the_batches_of_a_private_copy(tree):
    ds, shared, private = databases(tree)
    n = len(ds)
    assert n == 9 and shared.box_f32 and private.box_f32
    cfg = T.make_cfg(tree)
    cfg.LOSS.USE_DIFFERENT_JOINTS_WEIGHT = True
    draws = np.random.default_rng(5).random((n, 6))                     # u_half, n_half, n_scale, n_rot, u_rot, u_flip
    draws[:, 1:4] = np.random.default_rng(6).standard_normal((n, 3))
    draws[0, 4:6], draws[1, 4:6] = (0.2, 0.2), (0.9, 0.9)               # rotated and flipped / neither
    a, b = one_batch(shared, cfg, True, np.arange(n), draws), one_batch(private, cfg, True, np.arange(n), draws)
    flipped = a['meta']['flipped'].cpu().numpy()
    assert flipped[0] == 1 and flipped[1] == 0
    assert a['input'].shape == (n, 3, 64, 48) and a['input'].abs().max() > 0 and a['target'].max() == 1.0
    assert set(np.unique(a['target_weight'].cpu().numpy()).tolist()) <= {0.0, 1.0, float(np.float32(1.2)), 1.5}
    assert float(a['target_weight'].max()) == 1.5                       # joints_weight went along
    for k in KEYS:
        assert torch.equal(a[k], b[k]), ('train', k)
    va, vb = one_batch(shared, cfg, False, np.arange(n)), one_batch(private, cfg, False, np.arange(n))
    for k in KEYS:
        assert torch.equal(va[k], vb[k]), ('valid', k)
    assert not torch.equal(va['input'], a['input'])
    assert torch.equal(va['meta']['score'], torch.ones(n, dtype=torch.float64))          # no scores: ones, as before
    # each distinct picture once, in order of first appearance; the rows of its people point at the same pixels
    rows = np.frombuffer(shared.table.cpu().numpy().tobytes(), TABLE_ROW)
    paths = list(dict.fromkeys(rec['image'] for rec in ds.db))
    shape_of = {os.path.join(tree, 'images', 'train2017', '%012d.jpg' % i): T.IMAGE_SHAPES[k] for k, i in enumerate(T.IMAGE_IDS)}
    sizes = [shape_of[p][0] * shape_of[p][1] * 3 for p in paths]
    assert len(paths) == 5 and len(np.unique(rows['img'])) == 5
    assert shared.pixels.numel() == sum(sizes) and private.pixels.numel() == sum(sizes[paths.index(rec['image'])] for rec in ds.db)
    base = shared.pixels.data_ptr()
    for i, rec in enumerate(ds.db):
        k = paths.index(rec['image'])
        assert rows['img'][i] == base + sum(sizes[:k]) and (rows['h'][i], rows['w'][i]) == shape_of[rec['image']]
    assert shared.names == [rec['image'] for rec in ds.db] and va['meta']['image'] == shared.names
    # the decoded pixels are the JPEG's (PIL), B,G,R
    from PIL import Image
    with Image.open(paths[0]) as im:
        want = np.asarray(im.convert('RGB'))[:, :, ::-1].reshape(-1)
    assert np.array_equal(shared.pixels[:sizes[0]].cpu().numpy(), want)


def test_validate_carries_the_box_scores_of_a_detection_set(tree, tmp_path):
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.dataset import COCODataset, DeviceAugmentLoader
    from fpd_amd.lib.models import hourglass
    cfg = T.make_cfg(tree, test={'USE_GT_BBOX': False})
    cfg.MODEL.IMAGE_SIZE, cfg.MODEL.HEATMAP_SIZE = [64, 64], [16, 16]
    cfg.MODEL.EXTRA.NUM_FEATURES, cfg.MODEL.EXTRA.NUM_STACKS, cfg.TEST.FLIP_TEST, cfg.PRINT_FREQ = 64, 2, True, 1
    valid = COCODataset(cfg, tree, 'val2017', False)
    assert len(valid) == 12 and np.array_equal(np.array([rec['score'] for rec in valid.db]), G['db/val_det/score'])
    db = valid.to_device('cuda')
    assert np.array_equal(db.h_scores, G['db/val_det/score']) and len(np.unique(db.image_index)) == 5
    loader = DeviceAugmentLoader(db, cfg, 5, False)                     # 5 + 5 + 2
    torch.manual_seed(2)
    model = hourglass.get_pose_net(cfg, is_train=False).cuda()
    perf = F.validate(cfg, loader, valid, model, JointsMSELoss(True).cuda(), str(tmp_path), str(tmp_path), None)
    last = F.validate.last
    assert last['all_preds'].shape == (12, 17, 3) and np.isfinite(last['all_preds']).all() and np.isfinite(last['loss'])
    assert np.array_equal(last['all_boxes'][:, 5], G['db/val_det/score'])
    assert np.array_equal(last['all_boxes'][:, 0:2], G['db/val_det/center'].astype(np.float64))
    assert np.array_equal(last['all_boxes'][:, 2:4], np.stack([rec['scale'] for rec in valid.db]).astype(np.float64))      # (64x64 input: not the fixture's aspect ratio)
    with open(os.path.join(str(tmp_path), 'results', 'keypoints_val2017_results_0.json')) as f:
        results = json.load(f)
    assert 1 <= len(results) <= 12 and sorted(results[0]) == ['category_id', 'center', 'image_id', 'keypoints', 'scale', 'score']
    assert -1.0 <= perf <= 1.0


@pytest.mark.parametrize('mode', ['hard', 'soft'])
def test_evaluate_writes_the_results_list_of_the_reference(tree, tmp_path, mode):
    from fpd_amd.lib.dataset import COCODataset
    cfg = T.make_cfg(tree, test={'USE_GT_BBOX': False, 'SOFT_NMS': mode == 'soft'})
    ds = COCODataset(cfg, tree, 'val2017', False)
    paths = [os.path.join(tree, p) for p in G['in_paths']]
    preds, boxes = G['in_preds'].copy(), G['in_boxes'].copy()
    name_value, perf = ds.evaluate(cfg, preds, str(tmp_path), boxes, paths)
    assert np.array_equal(preds, G['in_preds']) and np.array_equal(boxes, G['in_boxes'])            # the inputs are left alone
    assert list(name_value) == STAT_NAMES and perf == name_value['AP']
    assert all(isinstance(v, float) and (v == -1.0 or 0.0 <= v <= 1.0) for v in name_value.values()), name_value
    with open(os.path.join(str(tmp_path), 'results', 'keypoints_val2017_results_0.json')) as f:
        got = T.results_arrays(json.load(f))
    for k in T.RESULT_KEYS:
        want = G['res/%s/%s' % (mode, k)]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape and np.array_equal(got[k], want), k
    assert len(got['score']) == {'hard': 32, 'soft': 36}[mode]
    # a test set: the file is written, nothing is scored
    test = COCODataset(cfg, tree, T.TEST_SET, False)
    out = tmp_path / 'test'
    assert test.evaluate(cfg, preds, str(out), boxes, paths) == ({'Null': 0}, 0)
    with open(os.path.join(str(out), 'results', 'keypoints_%s_results_0.json' % T.TEST_SET)) as f:
        assert np.array_equal(T.results_arrays(json.load(f))['score'], G['res/%s/score' % mode])


def _table_rows(log):
    """The value rows of the AP tables in a tool's log, each next to its header."""
    lines = log.splitlines()
    return [re.sub(r'^.*?\| ', '| ', lines[i + 2]) for i, l in enumerate(lines) if '| Arch | AP | Ap .5 ' in l and i + 2 < len(lines)]


def test_tools_train_and_test_on_a_coco_directory(tree, tmp_path):
    cfgd = os.path.join(ROOT, 'experiments', 'fpd_synthetic')
    shape = ['OUTPUT_DIR', str(tmp_path), 'MODEL.EXTRA.NUM_FEATURES', '32', 'MODEL.EXTRA.NUM_STACKS', '2', 'MODEL.IMAGE_SIZE', '128,128',
             'MODEL.HEATMAP_SIZE', '32,32', 'MODEL.NUM_JOINTS', '17', 'TEST.BATCH_SIZE_PER_GPU', '4', 'DATASET.DATASET', 'coco',
             'DATASET.ROOT', tree, 'DATASET.TRAIN_SET', 'train2017', 'DATASET.TEST_SET', 'val2017', 'DATASET.PROB_HALF_BODY', '0.3',
             'TEST.USE_GT_BBOX', 'False', 'TEST.COCO_BBOX_FILE', os.path.join(tree, 'detections.json'), 'TEST.IMAGE_THRE', '0.1',
             'TEST.OKS_THRE', '0.9', 'TEST.IN_VIS_THRE', '0.2', 'LOSS.USE_DIFFERENT_JOINTS_WEIGHT', 'True', 'PRINT_FREQ', '1',
             'MODEL.DTYPE', 'fp32']
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'fpd_train.py'), '--cfg', os.path.join(cfgd, 'hg4x128_student.yaml'),
           '--tcfg', os.path.join(cfgd, 'hg8x256_teacher.yaml'), '--max-iters', '2', 'TRAIN.BATCH_SIZE_PER_GPU', '4',
           'TRAIN.END_EPOCH', '1'] + shape
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    log = r.stdout + r.stderr
    last = [float(m) for m in re.findall(r'last logged loss ([0-9.eE+-]+)', log)]
    assert len(last) == 1 and np.isfinite(last[0]) and 0 < last[0] < 10, last
    assert log.count('\tPOSE_Loss') == 2 and log.count('Test: [0/3]') == 3
    assert '=> load 9 samples' in log and '=> load 12 samples' in log and '12 samples over 5 images' in log
    rows = _table_rows(log)
    assert len(rows) == 3 and all(row.count('|') == 12 for row in rows), rows                      # Arch + ten columns
    ckpts = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f == 'checkpoint.pth']
    assert len(ckpts) == 1
    res = os.path.join(os.path.dirname(ckpts[0]), 'results', 'keypoints_val2017_results_0.json')
    with open(res) as f:
        assert 1 <= len(json.load(f)) <= 12
    os.remove(res)
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), '--cfg', os.path.join(cfgd, 'hg4x128_student.yaml'),
                         'TEST.MODEL_FILE', ckpts[0]] + shape, env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, (r2.stdout[-1500:], r2.stderr[-3000:])
    log2 = r2.stdout + r2.stderr
    assert 'validation done' in log2 and _table_rows(log2) == rows[-1:], (_table_rows(log2), rows)
    with open(res) as f:
        assert 1 <= len(json.load(f)) <= 12
