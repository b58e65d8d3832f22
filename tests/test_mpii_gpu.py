"""The MPII dataset on the MI355X: images shared between the people of one picture, the streamed upload, the channel
order, the rank-aware loader order, `validate` with PCKh, and tools/fpd_train.py + tools/test.py on an MPII directory
(lib/dataset/mpii.py, lib/dataset/device_dataset.py; the tree and the fixture: tests/_mpii_tree.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _mpii_tree as T
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

G = T.load_golden()
TABLE_ROW = np.dtype([('img', '<u8'), ('h', '<i4'), ('w', '<i4'), ('row_bytes', '<i8')])
KEYS = ('input', 'target', 'target_weight', 'trans', 'joints')


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return T.write_tree(tmp_path_factory.mktemp('mpii'), G, gt=True)


_DBS = {}


def databases(tree):
    """(MPIIDataset, its device database with shared images, the same records over a private copy of the image per sample
    built the way databases were built before) -- made once, shared by the tests, never modified."""
    if tree not in _DBS:
        from fpd_amd.lib.dataset import DeviceJointsDB, MPIIDataset
        from fpd_amd.lib.dataset.mpii import read_image
        ds = MPIIDataset(T.make_cfg(tree), tree, 'valid', True)
        stack = lambda k: np.stack([rec[k] for rec in ds.db])  # noqa: E731
        private = DeviceJointsDB([read_image(rec['image']) for rec in ds.db], stack('joints_3d'), stack('joints_3d_vis'), stack('center'),
                                 stack('scale'), ds.flip_pairs, ds.upper_body_ids, ds.aspect_ratio, device='cuda')
        _DBS[tree] = (ds, ds.to_device('cuda'), private)
    return _DBS[tree]


def table(db):
    return np.frombuffer(db.table.cpu().numpy().tobytes(), TABLE_ROW)


def one_batch(db, cfg, is_train, idx, draws=None, **kw):
    from fpd_amd.lib.dataset import DeviceAugmentLoader
    loader = DeviceAugmentLoader(db, cfg, len(idx), is_train, shuffle=False, drop_last=False, **kw)
    x, tg, tw, meta = loader.batch(np.asarray(idx, np.int32), draws=draws)
    torch.cuda.synchronize()
    return dict(input=x, target=tg, target_weight=tw, trans=meta['trans'], joints=meta['joints'], meta=meta)


def test_shared_images_give_the_batches_of_a_private_copy_per_sample(tree):
    ds, shared, private = databases(tree)
    n = len(ds)
    cfg = T.make_cfg(tree)
    vis = np.stack([rec['joints_3d_vis'][:, 0] for rec in ds.db])
    half = int(np.flatnonzero((vis.sum(1) > cfg.DATASET.NUM_JOINTS_HALF_BODY) & (G['in_center'][:, 0] != -1))[0])
    draws = np.random.default_rng(5).random((n, 6))                     # u_half, n_half, n_scale, n_rot, u_rot, u_flip
    draws[:, 1:4] = np.random.default_rng(6).standard_normal((n, 3))
    draws[:, 0] = 0.9                                                   # no half-body crop but for `half`
    draws[half] = (0.1, 0.0, 0.0, 1.0, 0.2, 0.2)                        # half-body (upper), no jitter of the scale, rotated, flipped
    draws[(half + 1) % n, 4:6] = (0.9, 0.9)                             # neither rotated nor flipped
    a, b = one_batch(shared, cfg, True, np.arange(n), draws), one_batch(private, cfg, True, np.arange(n), draws)
    m = a['meta']
    flipped, rotation, scale = m['flipped'].cpu().numpy(), m['rotation'].cpu().numpy(), m['scale'].cpu().numpy()
    assert flipped[half] == 1 and flipped[(half + 1) % n] == 0 and rotation[half] != 0 and rotation[(half + 1) % n] == 0
    assert not np.array_equal(scale[half], shared.h_scale[half])        # the half-body crop replaced the person box
    assert a['input'].shape == (n, 3, 64, 64) and a['input'].abs().max() > 0 and a['target'].max() == 1.0
    for k in KEYS:
        assert torch.equal(a[k], b[k]), ('train', k)
    va, vb = one_batch(shared, cfg, False, np.arange(n)), one_batch(private, cfg, False, np.arange(n))
    for k in KEYS:
        assert torch.equal(va[k], vb[k]), ('valid', k)
    assert not torch.equal(va['input'], a['input'])
    # each of the 5 images once; the rows of its people point at the same pixels
    rows, sizes = table(shared), [h * w * 3 for h, w in T.IMAGE_SHAPES]
    assert len(np.unique(rows['img'])) == 5 and len(np.unique(table(private)['img'])) == n
    assert shared.pixels.numel() == sum(sizes) and private.pixels.numel() == sum(sizes[int(k[2])] for k in G['in_image'])
    base = shared.pixels.data_ptr()
    for i, name in enumerate(G['in_image']):
        k = int(name[2])                                                # 'im<k>.npy'; the images appear in the order 0..4
        assert rows['img'][i] == base + sum(sizes[:k]) and (rows['h'][i], rows['w'][i]) == T.IMAGE_SHAPES[k]
        assert rows['row_bytes'][i] == 3 * T.IMAGE_SHAPES[k][1]
    assert shared.names == [rec['image'] for rec in ds.db] and va['meta']['image'] == shared.names


def test_streaming_in_chunks_smaller_than_an_image_fills_the_same_buffer(tree):
    ds, shared, _ = databases(tree)
    assert min(h * w * 3 for h, w in T.IMAGE_SHAPES) > 1000
    small = ds.to_device('cuda', chunk_bytes=1000)
    assert small.pixels.numel() == shared.pixels.numel() and torch.equal(small.pixels, shared.pixels)
    odd = ds.to_device('cuda', chunk_bytes=40961)                       # images end inside a chunk
    assert torch.equal(odd.pixels, shared.pixels)
    want = np.concatenate([T.image(k).reshape(-1) for k in range(5)])
    assert np.array_equal(shared.pixels.cpu().numpy(), want)
    assert np.array_equal(table(small)['img'] - small.pixels.data_ptr(), table(shared)['img'] - shared.pixels.data_ptr())


def test_images_that_do_not_fit_raise_with_both_byte_counts(tree, monkeypatch):
    from fpd_amd.runtime import FpdError
    ds, shared, _ = databases(tree)
    need = shared.pixels.numel()
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda device=None: (need - 1, 1 << 38))
    with pytest.raises(FpdError, match=r'%d bytes.*%d bytes are free' % (need, need - 1)):
        ds.to_device('cuda')


def test_color_rgb_reverses_the_channel_axis(tree):
    from fpd_amd.lib.dataset import MPIIDataset
    ds, shared, _ = databases(tree)
    rgb_cfg = T.make_cfg(tree, COLOR_RGB=True)
    rgb = MPIIDataset(rgb_cfg, tree, 'valid', True).to_device('cuda')
    plain = dict(mean=(0, 0, 0), std=(1, 1, 1))
    idx = np.arange(len(ds))
    a, b = one_batch(shared, T.make_cfg(tree), False, idx, **plain), one_batch(rgb, rgb_cfg, False, idx, **plain)
    assert a['input'].abs().max() > 0 and not torch.equal(a['input'], b['input'])
    assert torch.equal(b['input'], a['input'].flip(1))
    assert torch.equal(a['target'], b['target'])


def _present_formula(loader, seed, epoch, n, batch):
    """The order and the batches the loader gave before it knew about ranks: one generator seeded by (seed, epoch) draws
    the permutation and then, per batch, rng.random((b,3)) -> u_half, u_rot, u_flip and rng.standard_normal((b,3)) ->
    n_half, n_scale, n_rot."""
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, epoch])))
    order = rng.permutation(n).astype(np.int32)
    out = []
    for k in range((n + batch - 1) // batch):
        idx = order[k * batch:(k + 1) * batch]
        u, nrm = rng.random((len(idx), 3)), rng.standard_normal((len(idx), 3))
        draws = np.zeros((len(idx), 6))
        draws[:, (0, 4, 5)], draws[:, 1:4] = u, nrm
        out.append((idx, loader.batch(idx, draws=draws)))
    return order, out


def test_two_ranks_partition_the_epoch_and_one_process_keeps_its_order(tree):
    from fpd_amd.lib.dataset import DeviceAugmentLoader
    ds, shared, _ = databases(tree)
    cfg, n = T.make_cfg(tree), len(ds)
    ranks = [DeviceAugmentLoader(shared, cfg, 4, True, shuffle=True, drop_last=False, seed=9, rank=r, world_size=2) for r in (0, 1)]
    single = DeviceAugmentLoader(shared, cfg, 4, True, shuffle=True, drop_last=False, seed=9)
    assert [len(l) for l in ranks] == [2, 2] and len(single) == 3
    for epoch in (0, 1):
        for l in ranks + [single]:
            l.set_epoch(epoch)
        got = [[(m['index'].cpu().numpy(), x.clone()) for x, _, _, m in l] for l in ranks]
        assert [[len(i) for i, _ in g] for g in got] == [[4, 2], [4, 2]]
        order, want = _present_formula(single, 9, epoch, n, 4)
        parts = [np.concatenate([i for i, _ in g]) for g in got]
        assert np.array_equal(parts[0], order[0::2]) and np.array_equal(parts[1], order[1::2])
        assert sorted(np.concatenate(parts).tolist()) == list(range(n))
        # each rank draws from its own generator: the same rows on rank 1 with rank 0's generator give other crops
        from fpd_amd.lib.dataset import epoch_order
        x01 = ranks[0].batch(parts[1][:4], rng=epoch_order(n, 9, epoch, True, 0, 2)[1])[0]
        assert not torch.equal(x01, got[1][0][1])
        # one process: order, draws and batches of the formula in use before
        batches = [(m['index'].cpu().numpy(), x, t, w, m['trans']) for x, t, w, m in single]
        assert len(batches) == len(want) == 3
        for (i, x, t, w, tr), (wi, (wx, wt, ww, wm)) in zip(batches, want):
            assert np.array_equal(i, wi) and torch.equal(x, wx) and torch.equal(t, wt) and torch.equal(w, ww) and torch.equal(tr, wm['trans'])
    # 12 samples over 5 ranks: 3 each after the wrap-around padding
    assert len(DeviceAugmentLoader(shared, cfg, 4, True, drop_last=True, rank=1, world_size=5)) == 0
    assert len(DeviceAugmentLoader(shared, cfg, 2, True, drop_last=True, rank=1, world_size=5)) == 1


def test_validate_reports_pckh_of_its_predictions(tree, tmp_path):
    pytest.importorskip('scipy.io')
    from scipy.io import loadmat
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.dataset import DeviceAugmentLoader, MPIIDataset
    from fpd_amd.lib.models import hourglass
    cfg = T.make_cfg(tree)
    cfg.MODEL.EXTRA.NUM_FEATURES, cfg.MODEL.EXTRA.NUM_STACKS, cfg.TEST.FLIP_TEST, cfg.PRINT_FREQ = 64, 2, True, 1
    ds, shared, _ = databases(tree)
    valid = MPIIDataset(cfg, tree, 'valid', False)
    loader = DeviceAugmentLoader(shared, cfg, 4, False)
    torch.manual_seed(2)
    model = hourglass.get_pose_net(cfg, is_train=False).cuda()
    seen = []
    valid.evaluate = lambda c, preds, out, boxes, paths, *a, **k: (seen.append(list(paths)), MPIIDataset.evaluate(valid, c, preds, out))[1]
    perf = F.validate(cfg, loader, valid, model, JointsMSELoss(True).cuda(), str(tmp_path), str(tmp_path), None)
    last = F.validate.last
    assert last['all_preds'].shape == (12, 16, 3) and np.isfinite(last['all_preds']).all() and np.isfinite(last['loss'])
    name_value, indicator = MPIIDataset.evaluate(valid, cfg, last['all_preds'], '')
    assert perf == indicator == name_value['Mean'] and 0.0 <= perf <= 100.0
    assert list(name_value)[-2:] == ['Mean', 'Mean@0.1']
    mat = loadmat(os.path.join(str(tmp_path), 'pred.mat'))['preds']
    assert np.array_equal(mat, last['all_preds'][:, :, 0:2] + np.float32(1.0))
    assert seen == [[rec['image'] for rec in valid.db]] and all(p.endswith('.npy') for p in seen[0])
    assert np.array_equal(last['all_boxes'][:, 0:2], np.stack([rec['center'] for rec in valid.db]))


def _table_rows(log):
    """The value rows of the metric tables in a tool's log, each next to its header."""
    lines = log.splitlines()
    return [re.sub(r'^.*?\| ', '| ', lines[i + 2]) for i, l in enumerate(lines) if '| Arch | Head ' in l and i + 2 < len(lines)]


def test_tools_train_and_test_on_an_mpii_directory(tree, tmp_path):
    pytest.importorskip('scipy.io')
    cfgd = os.path.join(ROOT, 'experiments', 'fpd_synthetic')
    shape = ['OUTPUT_DIR', str(tmp_path), 'MODEL.EXTRA.NUM_FEATURES', '32', 'MODEL.EXTRA.NUM_STACKS', '2', 'MODEL.IMAGE_SIZE', '128,128',
             'MODEL.HEATMAP_SIZE', '32,32', 'TEST.BATCH_SIZE_PER_GPU', '4', 'DATASET.DATASET', 'mpii', 'DATASET.ROOT', tree,
             'DATASET.PROB_HALF_BODY', '0.3', 'PRINT_FREQ', '1', 'MODEL.DTYPE', 'fp32']
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'fpd_train.py'), '--cfg', os.path.join(cfgd, 'hg4x128_student.yaml'),
           '--tcfg', os.path.join(cfgd, 'hg8x256_teacher.yaml'), '--max-iters', '3', 'TRAIN.BATCH_SIZE_PER_GPU', '4',
           'TRAIN.END_EPOCH', '1'] + shape
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    log = r.stdout + r.stderr
    last = [float(m) for m in re.findall(r'last logged loss ([0-9.eE+-]+)', log)]
    assert len(last) == 1 and np.isfinite(last[0]) and 0 < last[0] < 10, last
    assert log.count('\tPOSE_Loss') == 3 and log.count('Test: [0/3]') == 3
    assert '=> load 12 samples' in log and '12 samples over 5 images' in log
    rows = _table_rows(log)
    assert log.count('| Mean | Mean@0.1 |') == 3 and len(rows) == 3 and all(row.count('|') == 11 for row in rows), rows
    ckpts = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f == 'checkpoint.pth']
    assert len(ckpts) == 1 and os.path.exists(os.path.join(os.path.dirname(ckpts[0]), 'pred.mat'))
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), '--cfg', os.path.join(cfgd, 'hg4x128_student.yaml'),
                         'TEST.MODEL_FILE', ckpts[0]] + shape, env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, (r2.stdout[-1500:], r2.stderr[-3000:])
    log2 = r2.stdout + r2.stderr
    assert 'validation done' in log2 and _table_rows(log2) == rows[-1:], (_table_rows(log2), rows)
