"""DARK's unbiased target encoding on the device: fpd_render_targets_unbiased against the float64 numpy restatement
(tests/_encode_ref.py) under the tolerance of the specification, the designed guard cases, the round trip through
fpd_dark_refine, DeviceAugmentLoader / DevicePipeline with MODEL.TARGET_TYPE gaussian_unbiased, and tools/fpd_train.py.

With FPD_ENCODE_RECORD=<file> every value case appends its counts to that file."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _dark_ref as D
from tests import _encode_ref as E
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
_REF = {}


def reference(name, weighted):
    """(inputs, restatement) of a case, computed once on the CPU and only read afterwards."""
    key = (name, weighted)
    if key not in _REF:
        if name == 'designed':
            joints, vis, names, size, stride, sigma = E.designed_case()
            jw = np.linspace(0.5, 1.5, len(names)).astype(np.float32)
        else:
            joints, vis, jw, size, stride, sigma = E.random_case(name)
        jw = jw if weighted else None
        tg, tw, e, p = E.unbiased(joints, vis, size, stride, sigma, jw)
        for a in (tg, tw, e):
            a.setflags(write=False)
        _REF[key] = ((joints, vis, jw, size, stride, sigma), (tg, tw, e, p))
    return _REF[key]


def run_kernel(joints, vis, size, stride, sigma, jw=None):
    """fpd_render_targets_unbiased through the struct, the target pre-filled with NaN -> (target [B,J,H,W], weight [B,J]) numpy."""
    from fpd_amd import runtime as R
    b, j = vis.shape
    w, h = size
    jt = torch.from_numpy(np.ascontiguousarray(joints, np.float64)).cuda()
    vs = torch.from_numpy(np.ascontiguousarray(vis, np.float32)).cuda()
    target = torch.full((b, j, h, w), float('nan'), dtype=torch.float32, device='cuda')
    weight = torch.full((b, j), SENTINEL, dtype=torch.float32, device='cuda')
    a = R.TargetsUnbiasedT()
    a.B, a.J, a.H, a.W, a.sigma, a.stride_x, a.stride_y = b, j, h, w, sigma, stride[0], stride[1]
    a.joints, a.vis, a.target, a.weight = jt.data_ptr(), vs.data_ptr(), target.data_ptr(), weight.data_ptr()
    if jw is not None:
        wt = torch.from_numpy(np.ascontiguousarray(jw, np.float32)).cuda()
        a.joints_weight = wt.data_ptr()
    R.check(R.lib().fpd_render_targets_unbiased(a, R.current_stream()), 'fpd_render_targets_unbiased')
    return target.cpu().numpy(), weight.cpu().numpy()


def check_values(name, weighted):
    (joints, vis, jw, size, stride, sigma), (tg, tw, e, p) = reference(name, weighted)
    got, gw = run_kernel(joints, vis, size, stride, sigma, jw)
    assert not np.isnan(got).any(), 'a pixel was not written'
    ok, unequal, steps, small = E.within(got, e)
    line = '%-8s %s %s sigma %d: %d of %d maps drawn; %d of %d values not bit-equal to float32(exp(float64)); worst %d float32 steps, %.3e below 2^-126' % (
        name, 'weighted' if weighted else 'plain   ', vis.shape + (size[1], size[0]), sigma, int(p['drawn'].sum()), p['drawn'].size, unequal,
        got.size, steps, small)
    print(line)
    if os.environ.get('FPD_ENCODE_RECORD'):
        with open(os.environ['FPD_ENCODE_RECORD'], 'a') as f:
            f.write(line + '\n')
    assert gw.tobytes() == tw.tobytes(), (gw, tw)
    zero = ~p['drawn']
    assert got[zero].tobytes() == tg[zero].tobytes() == np.zeros_like(got[zero]).tobytes()          # +0.0f, bit for bit
    assert ok, (name, weighted, unequal, steps, small)
    return got, gw, p


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('name', sorted(E.SHAPES))
def test_kernel_matches_the_float64_restatement(name, weighted):
    """E2: 560 pixels, several trips of the 256 threads; E4: the float64 factors underflow; E5: odd W, scalar stores."""
    got, _, p = check_values(name, weighted)
    assert p['drawn'].any() and got[p['drawn']].max() > 0.5


def test_an_unaligned_target_buffer_takes_the_scalar_stores_and_writes_the_same_values():
    """W % 4 == 0 but the buffer starts 4 bytes off a 16-byte boundary."""
    from fpd_amd import runtime as R
    (joints, vis, jw, size, stride, sigma), (tg, tw, e, p) = reference('E1', False)
    b, j = vis.shape
    w, h = size
    jt, vs = torch.from_numpy(joints).cuda(), torch.from_numpy(vis).cuda()
    buf = torch.full((b * j * h * w + 4,), float('nan'), dtype=torch.float32, device='cuda')
    weight = torch.empty((b, j), dtype=torch.float32, device='cuda')
    a = R.TargetsUnbiasedT()
    a.B, a.J, a.H, a.W, a.sigma, a.stride_x, a.stride_y = b, j, h, w, sigma, stride[0], stride[1]
    a.joints, a.vis, a.target, a.weight = jt.data_ptr(), vs.data_ptr(), buf.data_ptr() + 4, weight.data_ptr()
    R.check(R.lib().fpd_render_targets_unbiased(a, R.current_stream()), 'fpd_render_targets_unbiased')
    out = buf.cpu().numpy()
    assert np.isnan(out[0]) and np.isnan(out[-3:]).all()
    assert out[1:-3].tobytes() == run_kernel(joints, vis, size, stride, sigma)[0].tobytes()


@pytest.mark.parametrize('weighted', [False, True])
def test_designed_cases_fall_on_their_side_of_every_guard(weighted):
    names = E.designed_case()[2]
    got, gw, p = check_values('designed', weighted)
    outside, drawn = E.designed_expectation(names)
    assert np.array_equal(p['outside'][0], outside) and np.array_equal(p['drawn'][0], drawn)
    assert np.array_equal(got[0].reshape(len(names), -1).any(1), drawn)
    assert (gw[0][outside] == 0).all() and (gw[0][~outside & (np.array(names) != 'vis = 0')] > 0).all()
    q = names.index('vis = 0.5')
    assert gw[0, q] == np.float32(0.5) * (np.linspace(0.5, 1.5, len(names)).astype(np.float32)[q] if weighted else np.float32(1))


@pytest.mark.parametrize('size', [(48, 64), (12, 16)])
def test_round_trip_through_the_device_decode_lands_on_the_true_centre(size):
    """Encode on the device, decode the same device map with fpd_dark_refine and with the restatement: the coordinates agree
    within the decode test's own bound 4 * E32 + 2^-17, and the device result is no farther from the true centre than the
    restatement's plus that bound."""
    from tests.test_dark_gpu import run_dark
    sigma, k = 2, 11
    joints, vis, cen = E.accuracy_case(size, n=64)
    joints, vis, cen = joints.reshape(4, 16, 3), vis.reshape(4, 16), cen.reshape(4, 16, 2)
    maps, gw = run_kernel(joints, vis, size, (4.0, 4.0), sigma)
    assert (gw == 1).all()
    c64, v64, r64, _ = D.decode(maps, k)
    c32 = D.decode(maps, k, np.float32)[0]
    bound = 4 * float(np.abs(c64.astype(np.float64) - c32).max()) + 2.0 ** -17
    coords, maxvals, refined, _ = run_dark(maps, k, 'nchw')
    assert refined.all() and np.array_equal(refined, r64) and maxvals.tobytes() == v64.tobytes()
    err = np.abs(coords.astype(np.float64) - c64).max()
    d_dev, d_ref = np.linalg.norm(coords - cen, axis=-1), np.linalg.norm(c64 - cen, axis=-1)
    d_arg = np.linalg.norm(D.argmax_coords(maps)[0] - cen, axis=-1)
    print('%dx%d: device against restatement %.3e (bound %.3e); distance to the true centre: device median %.3e max %.3e, '
          'restatement median %.3e max %.3e, arg-max median %.3e' % (size[1], size[0], err, bound, np.median(d_dev), d_dev.max(),
                                                                     np.median(d_ref), d_ref.max(), np.median(d_arg)))
    assert err <= bound
    assert (d_dev <= d_ref + bound).all()
    assert np.median(d_dev) < 0.05 * np.median(d_arg)          # and it is the sub-pixel centre that comes back


# ---- the loader and the pipeline ----
class AD(dict):
    __getattr__ = dict.__getitem__


def _loader_cfg(target_type, weight):
    model = AD(IMAGE_SIZE=[96, 128], HEATMAP_SIZE=[24, 32], SIGMA=2, NUM_JOINTS=17)
    if target_type is not None:
        model['TARGET_TYPE'] = target_type
    return AD(MODEL=model, DATASET=AD(FLIP=True, SCALE_FACTOR=0.3, ROT_FACTOR=40, PROB_HALF_BODY=0.3, NUM_JOINTS_HALF_BODY=8),
              LOSS=AD(USE_DIFFERENT_JOINTS_WEIGHT=weight))


@pytest.mark.parametrize('weight', [False, True])
def test_loader_with_unbiased_targets_changes_the_targets_and_nothing_else(weight):
    from fpd_amd import runtime as R
    from fpd_amd import synth
    from fpd_amd.lib.dataset import DeviceAugmentLoader, DeviceJointsDB, DevicePipeline
    J, B = 17, 6
    scenes = dict(synth.make_scenes(11, 10, J, size=(70, 110), aspect_ratio=0.75))
    jw = scenes['joints_weight'] = np.linspace(0.5, 1.5, J).astype(np.float32)
    db = DeviceJointsDB(device='cuda', **scenes)
    rng = np.random.RandomState(5)
    draws = np.concatenate([rng.rand(B, 1), rng.randn(B, 3), rng.rand(B, 2)], 1)
    idx = np.arange(B, dtype=np.int32)
    out = {}
    for tt in (None, 'gaussian', 'gaussian_unbiased'):
        loader = DeviceAugmentLoader(db, _loader_cfg(tt, weight), B, True, shuffle=False, drop_last=False, seed=0)
        out[tt] = loader.batch(idx, draws=draws)
    torch.cuda.synchronize()
    (x0, t0, w0, m0), (x1, t1, w1, m1), (x2, t2, w2, m2) = out[None], out['gaussian'], out['gaussian_unbiased']
    assert sorted(m0) == sorted(m1) == sorted(m2) and 'trans' in m2 and 'joints' in m2
    for other_x, other_m in ((x0, m0), (x1, m1)):
        assert torch.equal(x2, other_x)
        for k in m2:
            assert torch.equal(m2[k], other_m[k]), k
    assert t2.shape == t1.shape == (B, J, 32, 24) and w2.shape == w1.shape == (B, J, 1)
    assert torch.equal(t0, t1) and torch.equal(w0, w1) and torch.equal(w2, w1) and not torch.equal(t2, t1)
    # the unbiased target is the kernel's on meta['joints'], and the restatement's within the tolerance
    joints, vis = m2['joints'].cpu().numpy(), m2['joints_vis'].cpu().numpy()
    direct, dw = run_kernel(joints, vis, (24, 32), (4.0, 4.0), 2, jw if weight else None)
    assert t2.cpu().numpy().tobytes() == direct.tobytes() and w2.cpu().numpy().tobytes() == dw.tobytes()
    tg, tw, e, p = E.unbiased(joints, vis, (24, 32), (4.0, 4.0), 2, jw if weight else None)
    assert E.within(direct, e)[0] and dw.tobytes() == tw.tobytes() and p['drawn'].any()
    assert bool((w2 > 1).any()) == weight
    # DevicePipeline makes the same choice
    pipe = DevicePipeline((96, 128), (24, 32), 2, 'cuda', target_type='gaussian_unbiased')
    pt, pw = pipe.generate_target(m2['joints'], m2['joints_vis'])
    assert torch.equal(pt, t2) and pw.shape == (B, J, 1)
    if not weight:
        assert torch.equal(pw, w2)
    plain = DevicePipeline((96, 128), (24, 32), 2, 'cuda').generate_target(m2['joints'], m2['joints_vis'])[0]
    assert torch.equal(plain, t1)
    # the default type: nothing moved -- the loader's targets are fpd_render_targets_w's, called directly
    from fpd_amd.lib.dataset.device_pipeline import gaussian_patch
    g = torch.from_numpy(np.ascontiguousarray(gaussian_patch(2), np.float32)).cuda()
    target = torch.full((B, J, 32, 24), float('nan'), dtype=torch.float32, device='cuda')
    wts = torch.empty((B, J, 1), dtype=torch.float32, device='cuda')
    t = R.TargetsWT()
    t.t.B, t.t.J, t.t.H, t.t.W, t.t.patch, t.t.stride_x, t.t.stride_y = B, J, 32, 24, 13, 4.0, 4.0
    t.t.joints, t.t.vis, t.t.g = m1['joints'].data_ptr(), m1['joints_vis'].data_ptr(), g.data_ptr()
    t.t.target, t.t.weight = target.data_ptr(), wts.data_ptr()
    if weight:
        t.joints_weight = db.joints_weight.data_ptr()
    R.check(R.lib().fpd_render_targets_w(t, R.current_stream()), 'fpd_render_targets_w')
    assert torch.equal(target, t1) and torch.equal(wts, w1)
    bt, bw = E.biased(joints, vis, (24, 32), (4.0, 4.0), 2, jw if weight else None)
    assert t1.cpu().numpy().tobytes() == bt.tobytes() and w1.cpu().numpy()[..., 0].tobytes() == bw.tobytes()


def test_tools_fpd_train_runs_on_synthetic_aug_with_unbiased_targets_and_dark(tmp_path):
    """The shipped YAML (MODEL.TARGET_TYPE gaussian_unbiased, TEST.DARK) shrunk to a tiny net: a two-iteration epoch plus
    validation; the losses are finite and the first train loss differs from the `gaussian` run on the same seed."""
    cfgd = os.path.join(ROOT, 'experiments', 'fpd_synthetic')
    base = [sys.executable, os.path.join(ROOT, 'tools', 'fpd_train.py'), '--cfg', os.path.join(cfgd, 'hg4x128_student_dark.yaml'),
            '--tcfg', os.path.join(cfgd, 'hg8x256_teacher.yaml'), '--max-iters', '2',
            'MODEL.EXTRA.NUM_FEATURES', '32', 'MODEL.EXTRA.NUM_STACKS', '2', 'MODEL.IMAGE_SIZE', '128,128', 'MODEL.HEATMAP_SIZE', '32,32',
            'TRAIN.BATCH_SIZE_PER_GPU', '4', 'TEST.BATCH_SIZE_PER_GPU', '4', 'DATASET.NUM_SCENES', '8', 'DATASET.NUM_VALID_SAMPLES', '4',
            'PRINT_FREQ', '1', 'TRAIN.END_EPOCH', '1', 'MODEL.DTYPE', 'fp32']
    runs = {}
    for tt in ('gaussian_unbiased', 'gaussian'):               # side by side: two short processes
        out = tmp_path / tt
        runs[tt] = subprocess.Popen(base + ['OUTPUT_DIR', str(out), 'LOG_DIR', str(out), 'MODEL.TARGET_TYPE', tt],
                                    env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    first = {}
    for tt, proc in runs.items():
        log = proc.communicate(timeout=600)[0]
        assert proc.returncode == 0, log[-3000:]
        pose = [float(m) for m in re.findall(r'\tPOSE_Loss ([0-9.eE+-]+|nan|inf)', log)]
        last = [float(m) for m in re.findall(r'last logged loss ([0-9.eE+-]+|nan|inf)', log)]
        val = [float(m) for m in re.findall(r'Test: \[0/\d+\].*?Loss ([0-9.eE+-]+|nan|inf)', log)]
        assert len(pose) == 2 and len(last) == 1 and len(val) == 3 and np.isfinite(pose + last + val).all(), (pose, last, val, log[-2000:])
        assert 'PCK@0.5' in log
        first[tt] = pose[0]
    print('first train pose loss: unbiased %.5f, gaussian %.5f' % (first['gaussian_unbiased'], first['gaussian']))
    assert first['gaussian_unbiased'] != first['gaussian']
