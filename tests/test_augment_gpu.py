"""On-device training augmentation on the MI355X (csrc/data.hip augment_params / warp_affine_aug / render_targets_w,
lib/dataset/device_dataset.py) against the fixture written by the reference's own `JointsDataset.__getitem__`
(tests/golden/augment_ref.npz), against the existing per-sample DevicePipeline kernels on the same inputs, and through
`fpd_train` and tools/fpd_train.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _augment_ref as A
from tests._cases_infer import digest
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'augment_ref.npz'))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class AD(dict):
    __getattr__ = dict.__getitem__


def make_cfg(g, image_size=A.IMAGE_SIZE, heatmap_size=A.HEATMAP_SIZE):
    return AD(MODEL=AD(IMAGE_SIZE=list(image_size), HEATMAP_SIZE=list(heatmap_size), SIGMA=A.SIGMA, NUM_JOINTS=g['J']),
              DATASET=AD(FLIP=g['flip'], SCALE_FACTOR=g['sf'], ROT_FACTOR=g['rf'], PROB_HALF_BODY=g['prob_half'],
                         NUM_JOINTS_HALF_BODY=g['num_half']),
              LOSS=AD(USE_DIFFERENT_JOINTS_WEIGHT=g['weight']))


_RUNS = {}


def run(name):
    """One batch of a fixture group through the three launches (computed once, shared by the tests, never modified)."""
    if name in _RUNS:
        return _RUNS[name]
    from fpd_amd.lib.dataset import DeviceAugmentLoader, DeviceJointsDB
    g = A.GROUPS[name]
    inp = {k: GOLD['%s/in_%s' % (name, k)] for k in ('shapes', 'joints', 'vis', 'center', 'scale', 'draws')}
    B, J = inp['vis'].shape
    pairs, upper = A.tables(J)
    images = [A.scene(31 * i + J, int(h), int(w)) for i, (h, w) in enumerate(inp['shapes'])]
    db = DeviceJointsDB(images, inp['joints'], inp['vis'], inp['center'], inp['scale'], pairs, upper, A.ASPECT,
                        joints_weight=A.COCO_WEIGHT if J == 17 else None, device='cuda')
    loader = DeviceAugmentLoader(db, make_cfg(g), B, g['train'], shuffle=False, drop_last=False, seed=0)
    x, tg, tw, meta = loader.batch(np.arange(B, dtype=np.int32), draws=inp['draws'])
    rows = torch.zeros((B, 8), dtype=torch.float64)
    rows.numpy().view(np.int32)[:, 0] = np.arange(B)
    rows.numpy()[:, 1:7] = inp['draws']
    _, _, _, p = loader.launch(rows.cuda(), B)
    torch.cuda.synchronize()
    _RUNS[name] = dict(g=g, inp=inp, images=images, db=db, loader=loader, x=x, target=tg, weight=tw, meta=meta,
                       p={k: v.cpu().numpy() for k, v in p.items() if k != 'crop'})
    return _RUNS[name]


@pytest.mark.parametrize('name', list(A.GROUPS))
def test_parameters_match_the_reference_fixture(name):
    """Centre, scale, rotation, flip flag and visibility exact.  The matrix: applied to the four corners of the person
    box and to every visible joint, each result within 2e-3 px of the fixture's -- the device's sin / cos may differ from
    numpy's in the last place, which can move one float32 point coordinate below 4096 by one ulp (4.9e-4 px), and the
    3-point solve amplifies that by less than 4."""
    r = run(name)
    p, inp = r['p'], r['inp']
    for k in ('center', 'scale', 'rotation', 'flipped'):
        print(name, k, np.abs(p[k] - GOLD['%s/%s' % (name, k)]).max())
        assert np.array_equal(p[k], GOLD['%s/%s' % (name, k)]), (name, k, p[k], GOLD['%s/%s' % (name, k)])
    assert np.array_equal(p['vis'], GOLD[name + '/joints_vis'])
    worst = 0.0
    for i in range(p['trans'].shape[0]):
        c, s = inp['center'][i].astype(np.float64), inp['scale'][i].astype(np.float64) * 200
        pts = [c + np.array([sx, sy]) * s * 0.5 for sx in (-1, 1) for sy in (-1, 1)]
        pts += [xy for xy, v in zip(inp['joints'][i][:, 0:2], inp['vis'][i]) if v > 0]
        pts = np.concatenate([np.array(pts), np.ones((len(pts), 1))], 1)
        worst = max(worst, np.abs(pts @ p['trans'][i].T - pts @ GOLD[name + '/trans'][i].T).max())
        v = p['vis'][i] > 0
        worst = max(worst, np.abs(p['joints'][i][v] - GOLD[name + '/joints'][i][v]).max())
        assert np.array_equal(p['joints'][i][~v], GOLD[name + '/joints'][i][~v] * np.array([1, 1, 0]))
    print(name, 'max point deviation', worst)
    assert worst < 2e-3, worst


@pytest.mark.parametrize('name', list(A.GROUPS))
def test_crop_equals_the_per_sample_pipeline_on_the_same_matrices(name):
    """The device matrices fed to the existing DevicePipeline.crop, flipped samples mirrored on the host by torch.flip:
    bit-identical to the new crop (which mirrors by reading column w-1-X, not by composing the flip into the matrix)."""
    from fpd_amd.lib.dataset import DevicePipeline
    r = run(name)
    pipe = DevicePipeline(A.IMAGE_SIZE, A.HEATMAP_SIZE, A.SIGMA, 'cuda', MEAN, STD)
    imgs = [torch.from_numpy(im).cuda() for im in r['images']]
    imgs = [torch.flip(im, dims=[1]).contiguous() if f else im for im, f in zip(imgs, r['p']['flipped'])]
    want = pipe.crop(imgs, r['p']['trans'])
    assert r['x'].shape == want.shape and r['x'].abs().max() > 0
    assert torch.equal(r['x'], want), (name, (r['x'] != want).sum().item())


@pytest.mark.parametrize('name', ['coco_valid', 'mpii_valid'])
def test_validation_crop_equals_the_oracle_warp_of_the_host_matrix(name):
    """is_train = 0: the crop is bit-identical to oracle.infer_ref.warp_affine_u8 + to_tensor_normalize driven by the host's
    get_affine_transform(center, scale, 0, image_size) (well defined by the second precondition of the cases)."""
    from fpd_amd.lib.utils.transforms import get_affine_transform
    from oracle import infer_ref
    r = run(name)
    got = r['x'].cpu().numpy()
    for i, im in enumerate(r['images']):
        t = get_affine_transform(r['inp']['center'][i], r['inp']['scale'][i], 0, np.array(A.IMAGE_SIZE))
        u8 = infer_ref.warp_affine_u8(im, infer_ref.invert_affine(t), A.IMAGE_SIZE[0], A.IMAGE_SIZE[1])
        want = infer_ref.to_tensor_normalize(u8, MEAN, STD)
        assert want.dtype == np.float32 and np.array_equal(got[i], want), (name, i, np.abs(got[i] - want).max())
    assert (r['p']['flipped'] == 0).all() and (r['p']['rotation'] == 0).all()


@pytest.mark.parametrize('name', list(A.GROUPS))
def test_targets_equal_the_per_sample_pipeline_and_the_fixture(name):
    from fpd_amd.lib.dataset import DevicePipeline
    r = run(name)
    pipe = DevicePipeline(A.IMAGE_SIZE, A.HEATMAP_SIZE, A.SIGMA, 'cuda', MEAN, STD)
    tg, tw = pipe.generate_target(r['p']['joints'], r['p']['vis'])
    if r['g']['weight']:
        tw = tw * torch.from_numpy(A.COCO_WEIGHT).cuda().view(1, -1, 1)
    assert torch.equal(r['target'], tg) and torch.equal(r['weight'], tw)
    got, w = r['target'].cpu().numpy(), r['weight'].cpu().numpy()
    assert w.dtype == np.float32 and np.array_equal(w, GOLD[name + '/target_weight'])
    assert np.array_equal(got[:3], GOLD[name + '/target_full'])
    assert np.array_equal(digest(got), GOLD[name + '/target_sha'])
    if r['g']['weight']:
        assert (w > 1).any()


def _scene_loader(is_train, batch, seed=3, n=10, J=17, **kw):
    from fpd_amd import synth
    from fpd_amd.lib.dataset import DeviceAugmentLoader, DeviceJointsDB
    g = dict(A.GROUPS['coco_train'], J=J, weight=(J == 17), prob_half=0.3, num_half=8)
    scenes = synth.make_scenes(11, n, J, size=(70, 110), aspect_ratio=A.ASPECT)
    db = DeviceJointsDB(device='cuda', **scenes)
    db.scenes = scenes
    return db, DeviceAugmentLoader(db, make_cfg(g), batch, is_train, seed=seed, **kw)


def test_loader_is_seeded_per_epoch_handles_a_short_last_batch_and_validates_in_order():
    db, loader = _scene_loader(True, 4, shuffle=True, drop_last=False)
    assert len(loader) == 3
    loader.set_epoch(0)
    a = [(x.clone(), t.clone(), w.clone(), m['index'].clone()) for x, t, w, m in loader]
    loader.set_epoch(0)
    b = [(x.clone(), t.clone(), w.clone(), m['index'].clone()) for x, t, w, m in loader]
    c = [(x.clone(), t.clone(), w.clone(), m['index'].clone()) for x, t, w, m in loader]          # epoch 1 follows by itself
    assert [v[0].shape[0] for v in a] == [4, 4, 2] and a[0][1].shape == (4, 17, 16, 12) and a[2][2].shape == (2, 17, 1)
    for u, v in zip(a, b):
        assert all(torch.equal(p, q) for p, q in zip(u, v))
    assert sorted(torch.cat([v[3] for v in a]).tolist()) == list(range(10))
    assert not all(torch.equal(u[0], v[0]) for u, v in zip(a, c))
    assert all(torch.isfinite(v[0]).all() and v[1].max() == 1.0 for v in a)
    _, dl = _scene_loader(True, 4, shuffle=True, drop_last=True)
    assert len(dl) == 2 and [x.shape[0] for x, _, _, _ in dl] == [4, 4]
    # validation: the unaugmented crops in database order, host copies of centre / scale / score / image for validate()
    from fpd_amd.lib.dataset import DevicePipeline
    from fpd_amd.lib.utils.transforms import get_affine_transform
    pipe = DevicePipeline(A.IMAGE_SIZE, A.HEATMAP_SIZE, A.SIGMA, 'cuda', MEAN, STD)
    vdb, vl = _scene_loader(False, 4)
    seen = 0
    for x, t, w, m in vl:
        n = x.shape[0]
        assert m['image'] == vdb.names[seen:seen + n] and not m['center'].is_cuda and m['score'].shape == (n,)
        assert np.array_equal(m['center'].numpy(), vdb.h_center[seen:seen + n]) and np.array_equal(m['scale'].numpy(), vdb.h_scale[seen:seen + n])
        tr = m['trans'].cpu().numpy()
        for k in range(n):
            want = get_affine_transform(vdb.h_center[seen + k].astype(np.float32), vdb.h_scale[seen + k].astype(np.float32), 0, np.array(A.IMAGE_SIZE))
            np.testing.assert_allclose(tr[k], want, rtol=0, atol=1e-9)
        plain = pipe.crop([torch.from_numpy(im).cuda() for im in vdb.scenes['images'][seen:seen + n]], tr)
        assert torch.equal(x, plain) and torch.equal(m['joints_vis'].cpu(), torch.from_numpy(vdb.h_vis[seen:seen + n]))
        seen += n
    assert seen == 10


def _tiny_models(J=16):
    from fpd_amd.lib.models import hourglass
    from tests.test_model_gpu import make_cfg as model_cfg
    torch.manual_seed(1)
    student = hourglass.get_pose_net(model_cfg(64, 2, J), is_train=True).cuda()
    torch.manual_seed(2)
    teacher = hourglass.get_pose_net(model_cfg(64, 2, J), is_train=False).cuda()
    return student, teacher


def test_fpd_train_over_the_loader_equals_fpd_train_over_the_same_batches_as_a_list():
    """Tiny hourglass (S=2, F=64, 64x64 input, B=4), three iterations: the three logged losses with the loader are
    bit-identical to those of fpd_train fed the same three batches materialised as a list -- the loader hands complete
    batches to the step (its kernels have run, in stream order, before set_batch copies them)."""
    from fpd_amd import synth
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.dataset import DeviceAugmentLoader, DeviceJointsDB
    from fpd_amd.lib.utils.utils import FusedAdam
    J = 16
    g = dict(A.GROUPS['mpii_train'], prob_half=0.3, num_half=8)
    cfg = make_cfg(g, (64, 64), (16, 16))
    db = DeviceJointsDB(device='cuda', **synth.make_scenes(23, 12, J, size=(80, 120), aspect_ratio=1.0))
    loader = DeviceAugmentLoader(db, cfg, 4, True, shuffle=True, drop_last=True, seed=5)
    run_cfg = AD(KD=AD(ALPHA=0.5), PRINT_FREQ=1, DEBUG=AD(DEBUG=False))
    crit = JointsMSELoss(True).cuda()

    def losses(batches):
        student, teacher = _tiny_models(J)
        opt = FusedAdam(student, lr=2.5e-4)
        F.fpd_train(run_cfg, batches, student, teacher, crit, crit, opt, 0, '/tmp', '/tmp', None)
        step = F.fused_step_for(student, teacher, opt, (4, 3, 64, 64), 0.5, 1, (True, True))
        return step.metric.log.view(-1, 4)[:3].cpu().numpy().copy()
    loader.set_epoch(0)
    live = losses(loader)
    loader.set_epoch(0)
    frozen = [(x.clone(), t.clone(), w.clone(), m) for x, t, w, m in loader]
    torch.cuda.synchronize()
    assert len(frozen) == 3
    listed = losses(frozen)
    print('live', live, 'listed', listed)
    assert np.isfinite(live).all() and (live[:, 2] > 0).all()
    assert np.array_equal(live, listed), (live, listed)


def test_tools_fpd_train_runs_on_synthetic_aug_with_joint_weights(tmp_path):
    """`tools/fpd_train.py ... DATASET.DATASET synthetic_aug LOSS.USE_DIFFERENT_JOINTS_WEIGHT True` with 17 joints: exits 0,
    logs a finite loss, validates on the device-cropped scenes and writes a checkpoint."""
    cfgd = os.path.join(ROOT, 'experiments', 'fpd_synthetic')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'fpd_train.py'), '--cfg', os.path.join(cfgd, 'hg4x128_student.yaml'),
           '--tcfg', os.path.join(cfgd, 'hg8x256_teacher.yaml'), '--max-iters', '3', 'OUTPUT_DIR', str(tmp_path),
           'MODEL.EXTRA.NUM_FEATURES', '32', 'MODEL.EXTRA.NUM_STACKS', '2', 'MODEL.IMAGE_SIZE', '128,128', 'MODEL.HEATMAP_SIZE', '32,32',
           'MODEL.NUM_JOINTS', '17', 'TRAIN.BATCH_SIZE_PER_GPU', '4', 'TEST.BATCH_SIZE_PER_GPU', '4', 'DATASET.DATASET', 'synthetic_aug',
           'DATASET.NUM_SCENES', '12', 'DATASET.NUM_VALID_SAMPLES', '8', 'DATASET.PROB_HALF_BODY', '0.3',
           'LOSS.USE_DIFFERENT_JOINTS_WEIGHT', 'True', 'PRINT_FREQ', '1', 'TRAIN.END_EPOCH', '1', 'MODEL.DTYPE', 'fp32']
    r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    log = r.stdout + r.stderr
    last = [float(m) for m in re.findall(r'last logged loss ([0-9.eE+-]+)', log)]
    assert len(last) == 1 and np.isfinite(last[0]) and 0 < last[0] < 10, last
    assert log.count('\tPOSE_Loss') == 3 and 'PCK@0.5' in log and log.count('Test: [0/') == 3
    assert any(f == 'checkpoint.pth' for _, _, fs in os.walk(tmp_path) for f in fs)
