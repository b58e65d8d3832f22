"""utils.vis on the device: the four fpd_vis_* kernels against the host restatement (tests/_vis_ref.py) byte for byte, and the
debug images of core.function.fpd_train / validate end to end on a tiny synthetic_aug database."""
import os

import numpy as np
import pytest
import torch

from tests import _vis_ref as ref

pytestmark = pytest.mark.gpu


def _vis():
    from fpd_amd.lib.utils import vis
    return vis


# ---- fpd_vis_minmax ----

@pytest.mark.parametrize('shape', [(1, 3, 5, 7), (2, 3, 64, 48)])
def test_minmax_is_exact(shape):
    vis = _vis()
    rng = np.random.RandomState(shape[0])
    n = int(np.prod(shape))
    cases = {'seeded': rng.standard_normal(n).astype(np.float32), 'equal': np.full(n, -2.75, np.float32)}
    first = rng.uniform(-1, 1, n).astype(np.float32)
    first[0], first[-1] = -5.5, 7.25                                  # the extremes at the first and the last element
    last = rng.uniform(-1, 1, n).astype(np.float32)
    last[0], last[-1] = 9.0, -1e30
    zeros = np.abs(rng.standard_normal(n)).astype(np.float32)
    zeros[n // 2] = -0.0                                              # the minimum is a negative zero
    neg = -np.abs(rng.standard_normal(n)).astype(np.float32) - 1.0    # all negative; all positive
    cases.update(first=first, last=last, zeros=zeros, neg=neg, pos=-neg, zero_max=-np.abs(zeros))
    for name, x in cases.items():
        got = vis.image_minmax(torch.from_numpy(x.reshape(shape)).cuda()).cpu().numpy()
        assert got.dtype == np.float32 and got[0] == x.min() and got[1] == x.max(), (name, got, x.min(), x.max())


# ---- fpd_vis_max_preds ----

def _layouts(hm):
    """The three forms of a float32 [N,J,h,w] array whose values are bf16-exact: (name, device tensor of logical NCHW shape)."""
    t = torch.from_numpy(hm).cuda()
    nhwc = t.permute(0, 2, 3, 1).contiguous()
    return [('f32 nchw', t), ('f32 nhwc', nhwc.permute(0, 3, 1, 2)), ('bf16 nhwc', nhwc.to(torch.bfloat16).permute(0, 3, 1, 2))]


def _bf16_exact(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def planted_maps():
    """N=2, J=3, 4x6: ties (first in row-major order wins), an all-negative map, maxima in the corners, a zero maximum."""
    rng = np.random.RandomState(5)
    hm = _bf16_exact(rng.uniform(-1, 0.5, (2, 3, 4, 6)))
    hm[0, 0, 1, 4] = hm[0, 0, 2, 1] = hm[0, 0, 3, 5] = 2.0            # ties -> (4, 1)
    hm[0, 1] = -np.abs(hm[0, 1]) - 0.25                               # all negative -> (0, 0), the maximum kept
    hm[0, 2, 3, 5] = 3.0                                              # bottom-right corner
    hm[1, 0, 0, 0] = 3.0                                              # top-left
    hm[1, 1, 0, 5] = hm[1, 1, 3, 0] = 1.5                             # the two other corners, tied -> (5, 0)
    hm[1, 2] = np.minimum(hm[1, 2], 0.0)
    hm[1, 2, 2, 3] = 0.0                                              # a maximum of exactly 0 is zeroed
    return _bf16_exact(hm)                                            # (the planted values are bf16-exact)


def test_max_preds_in_the_three_layouts():
    from fpd_amd.lib.core.inference import get_max_preds
    vis = _vis()
    hm = planted_maps()
    want_p, want_m = ref.get_max_preds(hm)
    assert want_p[0].tolist() == [[4, 1], [0, 0], [5, 3]] and want_p[1].tolist() == [[0, 0], [5, 0], [0, 0]]
    pkg_p, pkg_m = get_max_preds(torch.from_numpy(hm).cuda())
    assert np.array_equal(pkg_p.cpu().numpy(), want_p) and np.array_equal(pkg_m.cpu().numpy(), want_m)
    for name, t in _layouts(hm):
        p, m = vis.max_preds(t)
        assert p.dtype == torch.float32 and tuple(p.shape) == (2, 3, 2) and tuple(m.shape) == (2, 3, 1), name
        assert np.array_equal(p.cpu().numpy(), want_p) and np.array_equal(m.cpu().numpy(), want_m), name


# ---- fpd_vis_joints_grid ----

def _joints_case(n, seed, constant=False):
    """Images [n,3,16,12], J = 4 joints per image (x, y, -) in image pixels and their visibility."""
    rng = np.random.RandomState(seed)
    img = np.full((n, 3, 16, 12), 0.375, np.float32) if constant else rng.standard_normal((n, 3, 16, 12)).astype(np.float32)
    joints = np.zeros((n, 4, 3))
    vis = np.ones((n, 4, 1), np.float32)
    for k in range(n):
        joints[k, 0] = [0, 0, 0]                                      # the cell's origin: cell 0's mark is clipped by the canvas edge
        joints[k, 1] = [10.75, 5.5, 0]                                # fractional; reaches into the padding and the next cell
        joints[k, 2] = [11.25, 6.0, 0]                                # overlaps joint 1's mark
        joints[k, 3] = rng.uniform(-6, 20, 3)                         # anywhere, outside the cell included
    joints[0, 3] = [-1.5, -0.75, 0]                                   # negative sums truncate towards zero (int(0.5) = 0 with padding 2)
    joints[n - 1, 3] = [1000.0, 1000.0, 0]                            # beyond the bottom-right of the canvas
    joints[n - 1, 2] = [13.0, 17.0, 0]                                # past the last cell's corner: partly off the canvas
    vis[0, 2, 0] = 0.0                                                # not drawn
    if n > 1:
        vis[1, :, 0] = [0.0, 2.0, 0.0, -1.0]                          # anything non-zero draws
    return img, joints, vis


@pytest.mark.parametrize('padding', [2, 0])
@pytest.mark.parametrize('n,nrow', [(3, 2), (9, 8), (1, 8)])
def test_joints_grid_equals_the_restatement(n, nrow, padding):
    vis = _vis()
    for constant in (False, True):
        img, joints, jv = _joints_case(n, 10 * n + padding, constant)
        x = torch.from_numpy(img)
        # float64 joints as the loaders deliver them, coord_scale 1
        want = ref.save_batch_image_with_joints(x, joints, jv, nrow, padding)
        assert want.shape == vis.grid_shape(n, 16, 12, nrow, padding) + (3,)
        assert (want == [255, 0, 0]).all(2).any()
        jd = torch.from_numpy(joints).cuda()
        before = jd.clone()
        got = vis.render_image_with_joints(x.cuda(), jd, torch.from_numpy(jv).cuda(), nrow, padding).cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (n, nrow, padding, constant)
        assert torch.equal(jd, before)                                # the reference's in-place edit is not copied
        # float32 predictions in heat-map pixels, coord_scale 4; joints_vis as [B,J] and [B,J,3]
        q = (joints[:, :, :2] / 4).astype(np.float32)
        want4 = ref.save_batch_image_with_joints(x, q * np.float32(4), jv, nrow, padding)
        for v in (jv[:, :, 0], np.repeat(jv, 3, 2)):
            got4 = vis.render_image_with_joints(x.cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(v.copy()).cuda(), nrow, padding,
                                                coord_scale=4.0).cpu().numpy()
            assert np.array_equal(got4, want4), (n, nrow, padding, constant)


def test_save_batch_image_with_joints_writes_the_canvas(tmp_path):
    from PIL import Image
    vis = _vis()
    img, joints, jv = _joints_case(3, 1)
    path = str(tmp_path / 'grid.jpg')
    canvas = vis.save_batch_image_with_joints(torch.from_numpy(img).cuda(), torch.from_numpy(joints).cuda(), torch.from_numpy(jv).cuda(), path, nrow=2)
    assert np.array_equal(canvas, ref.save_batch_image_with_joints(torch.from_numpy(img), joints, jv, 2, 2))
    assert Image.open(path).size == (canvas.shape[1], canvas.shape[0])


# ---- fpd_vis_heatmap_grid ----

def _heat_values(rng, shape):
    """Float32 heat values below 0, above 1, at multiples of 1/255 and in between."""
    k = rng.randint(0, 256, shape).astype(np.float32) / np.float32(255)
    pick = rng.randint(0, 5, shape)
    v = np.where(pick == 0, k, np.where(pick == 1, rng.uniform(-0.5, 0.0, shape), np.where(pick == 2, rng.uniform(1.0, 1.5, shape),
                                                                                          rng.uniform(0.0, 1.0, shape))))
    return v.astype(np.float32)


def _check_heatmaps(img, hm, normalize=True):
    """The float32 maps in both float32 layouts, and their bf16 rounding in the bf16 layout, each against the restatement on
    the values that layout holds; returns the float32 canvas."""
    vis = _vis()
    x = torch.from_numpy(img)
    first = None
    for src, forms in ((hm, _layouts(hm)[:2]), (_bf16_exact(hm), _layouts(_bf16_exact(hm))[2:])):
        want = ref.save_batch_heatmaps(x, torch.from_numpy(src), normalize)
        first = want if first is None else first
        for name, t in forms:
            got = vis.render_heatmaps(x.cuda(), t, normalize).cpu().numpy()
            assert got.dtype == np.uint8 and got.shape == want.shape, name
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (name, normalize, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    return first


@pytest.mark.parametrize('normalize', [True, False])
def test_heatmap_grid_small_with_overlapping_marks(normalize):
    """N=2, J=3, 4x6 from 16x24; sample 0's maxima are hand-placed so that the marks overlap across joints: joint 1's peak lies
    on joint 0's mark, joint 2's peak on joint 0's peak -- the cumulative base of tiles 2 and 3 shows joint 0's mark."""
    rng = np.random.RandomState(2)
    img = (rng.standard_normal((2, 3, 16, 24)) * (1.0 if normalize else 0.5) + (0.0 if normalize else 0.5)).astype(np.float32)
    hm = np.minimum(_heat_values(rng, (2, 3, 4, 6)), np.float32(0.996))
    hm[0, 0, 1, 2] = hm[0, 1, 1, 3] = hm[0, 2, 1, 2] = 1.25
    hm[1, 0, 0, 0] = hm[1, 1, 3, 5] = 1.25                            # marks clipped by the tile's corners
    hm[1, 2] = -np.abs(hm[1, 2]) - 0.125                              # all negative: the mark goes to (0, 0)
    want = _check_heatmaps(img, hm, normalize)
    assert want.shape == (8, 24, 3)
    red = [0, 0, 255]
    assert want[1, 1].tolist() == red and want[1, 3].tolist() == red and want[0, 2].tolist() == red      # tile 0: all marks
    assert want[1, 6 + 1].tolist() == red and want[1, 12 + 2].tolist() == red                           # tile 1: joint 0, tile 2: joint 1
    # tile 2, joint 0's mark at (1, 1): the base there is (0, 0, 255), blended, not overwritten
    heat = int(min(max(np.float32(hm[0, 1, 1, 1]) * np.float32(255), np.float32(0)), np.float32(255)))
    assert want[1, 12 + 1].tolist() == [int(c * 0.7 + b * 0.3) for c, b in zip(ref.JET_BGR[heat].tolist(), red)]


def test_heatmap_grid_at_the_real_tile():
    """N=2, J=16, 64x64 from 256x256, seeded: several trips of the grid, 393 216 blended bytes over every class of pair."""
    rng = np.random.RandomState(9)
    img = rng.standard_normal((2, 3, 256, 256)).astype(np.float32)
    hm = _heat_values(rng, (2, 16, 64, 64))
    want = _check_heatmaps(img, hm, True)
    assert want.shape == (128, 17 * 64, 3) and len(np.unique(want)) > 200


def test_save_batch_heatmaps_writes_the_canvas(tmp_path):
    from PIL import Image
    vis = _vis()
    rng = np.random.RandomState(4)
    img, hm = rng.standard_normal((2, 3, 16, 24)).astype(np.float32), _heat_values(rng, (2, 3, 4, 6))
    path = str(tmp_path / 'hm.jpg')
    canvas = vis.save_batch_heatmaps(torch.from_numpy(img).cuda(), torch.from_numpy(hm).cuda(), path)
    assert np.array_equal(canvas, ref.save_batch_heatmaps(torch.from_numpy(img), torch.from_numpy(hm)))
    assert Image.open(path).size == (24, 8)


# ---- end to end ----

def _e2e_cfg(debug, dataset='synthetic_aug'):
    from fpd_amd.lib.config import _defaults
    cfg = _defaults()
    cfg.DATASET.DATASET, cfg.DATASET.NUM_SCENES, cfg.DATASET.NUM_VALID_SAMPLES, cfg.DATASET.NUM_SAMPLES = dataset, 6, 3, 6
    cfg.TRAIN.BATCH_SIZE_PER_GPU = cfg.TEST.BATCH_SIZE_PER_GPU = 3
    cfg.TRAIN.SHUFFLE = False
    cfg.PRINT_FREQ = 1
    cfg.TEST.FLIP_TEST = cfg.TEST.SHIFT_HEATMAP = cfg.TEST.POST_PROCESS = True
    cfg.MODEL.EXTRA.NUM_FEATURES, cfg.MODEL.EXTRA.NUM_STACKS = 32, 2          # the student of tests/_cases.py 'tiny'
    cfg.MODEL.IMAGE_SIZE, cfg.MODEL.HEATMAP_SIZE = [128, 128], [32, 32]
    d = cfg.DEBUG
    d.DEBUG = d.SAVE_BATCH_IMAGES_GT = d.SAVE_BATCH_IMAGES_PRED = d.SAVE_HEATMAPS_GT = d.SAVE_HEATMAPS_PRED = bool(debug)
    return cfg


def _e2e_models(cfg):
    from fpd_amd.lib.models import hourglass
    torch.manual_seed(1)
    student = hourglass.get_pose_net(cfg, is_train=True).cuda()
    torch.manual_seed(2)
    teacher = hourglass.get_pose_net(cfg, is_train=False).cuda()
    return student, teacher


def _train_two_iterations(cfg, out_dir):
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.dataset.device_dataset import synthetic_aug
    from fpd_amd.lib.utils.utils import FusedAdam
    loader, valid_loader, valid_db = synthetic_aug(cfg, 'cuda')
    assert len(loader) == 2
    student, teacher = _e2e_models(cfg)
    crit = JointsMSELoss(True).cuda()
    before = student._flat['param'].detach().clone()
    F.fpd_train(cfg, loader, student, teacher, crit, crit, FusedAdam(student, lr=2.5e-4), 0, out_dir, out_dir, None)
    assert not torch.equal(before, student._flat['param'])           # the two iterations did update the arena
    torch.cuda.synchronize()
    return student, valid_loader, valid_db, student._flat['param'].detach().clone().cpu()


def test_debug_images_of_the_train_and_validate_loops(tmp_path, monkeypatch):
    from PIL import Image

    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    vis = _vis()
    calls, written = [], []
    real_save, real_writer = vis.save_debug_images, vis.AsyncImageWriter

    def spy(config, input, meta, target, joints_pred, output, prefix, writer=None):
        assert writer is not None and joints_pred is None
        calls.append(dict(prefix=prefix, input=input.clone(), target=target.clone(), output=output.float().contiguous().clone(),
                          joints=meta['joints'].clone(), joints_vis=meta['joints_vis'].clone()))
        return real_save(config, input, meta, target, joints_pred, output, prefix, writer=writer)

    class Recorder(real_writer):
        def put(self, path, canvas, event=None):
            written.append((path, canvas))                            # (the pinned array: complete once the writer is closed)
            real_writer.put(self, path, canvas, event)
    monkeypatch.setattr(vis, 'save_debug_images', spy)
    monkeypatch.setattr(vis, 'AsyncImageWriter', Recorder)

    on, off = str(tmp_path / 'on'), str(tmp_path / 'off')
    os.makedirs(on), os.makedirs(off)
    student, valid_loader, valid_db, params_on = _train_two_iterations(_e2e_cfg(True), on)
    cfg = _e2e_cfg(True)
    F.validate(cfg, valid_loader, valid_db, student, JointsMSELoss(True).cuda(), on, on)
    names = ['%s_%d_%s.jpg' % (p, i, k) for p, n in (('train', 2), ('val', 1)) for i in range(n) for k in ('gt', 'pred', 'hm_gt', 'hm_pred')]
    assert sorted(f for f in os.listdir(on) if f.endswith('.jpg')) == sorted(names) and len(names) == 12
    assert len(calls) == 3 and [os.path.basename(p) for p, _ in written] == names
    for path, canvas in written:
        want = (3 * 130 + 2, 130 + 2) if ('_gt.jpg' in path or '_pred.jpg' in path) and '_hm_' not in path else (17 * 32, 3 * 32)
        assert Image.open(path).size == want == (canvas.shape[1], canvas.shape[0]), path
    by_name = dict((os.path.basename(p), c) for p, c in written)
    for c in calls:
        x, tgt, out = c['input'].cpu(), c['target'].cpu().float(), c['output'].cpu()
        joints, jv = c['joints'].cpu().numpy(), c['joints_vis'].cpu().numpy()
        base = os.path.basename(c['prefix'])
        preds = ref.get_max_preds(out.numpy())[0]
        assert np.array_equal(by_name[base + '_gt.jpg'], ref.save_batch_image_with_joints(x, joints, jv)), base
        assert np.array_equal(by_name[base + '_pred.jpg'], ref.save_batch_image_with_joints(x, preds * np.float32(4), jv)), base
        assert np.array_equal(by_name[base + '_hm_gt.jpg'], ref.save_batch_heatmaps(x, tgt)), base
        assert np.array_equal(by_name[base + '_hm_pred.jpg'], ref.save_batch_heatmaps(x, out)), base
    # the hook reads, the step is untouched: the same two iterations with DEBUG.DEBUG off leave the same parameters, bit for bit
    monkeypatch.setattr(vis, 'save_debug_images', real_save)
    monkeypatch.setattr(vis, 'AsyncImageWriter', real_writer)
    _, _, _, params_off = _train_two_iterations(_e2e_cfg(False), off)
    assert os.listdir(off) == [] and len(calls) == 3
    assert params_on.numel() > 1000 and torch.equal(params_on, params_off)


def test_the_plain_synthetic_set_is_refused_when_joints_are_to_be_drawn(tmp_path):
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.dataset.synthetic import SyntheticPose
    from fpd_amd.lib.utils.utils import FusedAdam
    from fpd_amd.runtime import FpdError
    cfg = _e2e_cfg(True, 'synthetic')
    train_set = SyntheticPose(cfg, cfg.DATASET.NUM_SAMPLES, seed=0)
    loader = torch.utils.data.DataLoader(train_set, batch_size=3, shuffle=False, num_workers=0, drop_last=True, collate_fn=train_set.collate)
    student, teacher = _e2e_models(cfg)
    crit = JointsMSELoss(True).cuda()
    with pytest.raises(FpdError, match="meta\\['joints'\\]"):
        F.fpd_train(cfg, loader, student, teacher, crit, crit, FusedAdam(student, lr=2.5e-4), 0, str(tmp_path), str(tmp_path), None)
    torch.cuda.synchronize()
    assert [f for f in os.listdir(str(tmp_path)) if f.endswith('.jpg')] == []
