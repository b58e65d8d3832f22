"""On-device augmentation, the parts that need no GPU: the numpy restatement (tests/_augment_ref.py) against the fixture
written by the reference's own `__getitem__` (tests/golden/augment_ref.npz), the preconditions every case must meet, a
HOST build of the kernel's scalar arithmetic (csrc/augment_math.h) against the same fixture, the ABI surface and the new
config defaults (/root/reference/lib/config/default.py:66-71)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _augment_ref as A
from tests._cases_infer import digest
from tests.conftest import ROOT

GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'augment_ref.npz'))


def inputs(name):
    return {k: GOLD['%s/in_%s' % (name, k)] for k in ('shapes', 'joints', 'vis', 'center', 'scale', 'draws')}


def test_fixture_inputs_are_the_declared_cases_and_cover_every_branch():
    for name in A.GROUPS:
        want, got = A.group_inputs(name), inputs(name)
        for k in want:
            assert want[k].dtype == got[k].dtype and np.array_equal(want[k], got[k]), (name, k)
    for name in ('coco_train', 'mpii_train'):
        g, inp = A.GROUPS[name], inputs(name)
        fl, rot, dr = GOLD[name + '/flipped'], GOLD[name + '/rotation'], inp['draws']
        assert set(fl.tolist()) == {0, 1}
        assert (rot == 2 * g['rf']).any() and (rot == -2 * g['rf']).any() and (rot[dr[:, 4] > 0.6] == 0).all() and (dr[:, 4] > 0.6).any()
        ratio = GOLD[name + '/scale'][:, 0] / inp['scale'][:, 0].astype(np.float64)
        kept = np.array([i for i in range(len(fl)) if i not in (2, 3, 4)])            # samples without a half-body crop
        assert np.isclose(ratio[kept], 1 + g['sf']).any() and np.isclose(ratio[kept], 1 - g['sf']).any()
        assert (inp['vis'] == 0).any()
        # half-body: upper (2), lower (3), fallback to upper (4) took a new centre; rejected (5) and not entered (9) kept it
        c_in = inp['center'].astype(np.float64).copy()
        c_in[fl == 1, 0] = np.nan
        moved = [i for i in range(len(fl)) if fl[i] == 0 and not np.array_equal(GOLD[name + '/center'][i], c_in[i])]
        assert moved == [3, 4], moved
    shapes = np.concatenate([inputs(n)['shapes'] for n in A.GROUPS])
    assert shapes.min(0).tolist() == [61, 97] and shapes.max(0).tolist() == [300, 420]
    for name in A.GROUPS:           # a visible joint whose patch lies fully outside the map
        assert ((GOLD[name + '/joints_vis'] > 0) & (GOLD[name + '/target_weight'][..., 0] == 0)).any(), name


def test_half_body_cases_take_both_aspect_ratio_branches():
    """Sample 3 selects the lower body of a wide layout (w > aspect_ratio * h: h is grown), sample 4 falls back to the upper
    body of a tall one (w < aspect_ratio * h: w is grown)."""
    for name in ('coco_train', 'mpii_train'):
        inp, upper = inputs(name), A.tables(A.GROUPS[name]['J'])[1]
        for i, want_upper, wide in ((3, False, True), (4, True, False)):
            sel = np.array([inp['joints'][i][k] for k in range(inp['vis'].shape[1])
                            if inp['vis'][i, k] > 0 and (k in upper) == want_upper], np.float32)
            assert sel.shape[0] > 2
            w, h = np.ptp(sel[:, 0]), np.ptp(sel[:, 1])
            assert (w > np.float32(A.ASPECT) * h) if wide else (w < np.float32(A.ASPECT) * h), (name, i, w, h)


@pytest.mark.parametrize('name', list(A.GROUPS))
def test_numpy_restatement_reproduces_the_reference_fixture(name):
    g, inp = A.GROUPS[name], inputs(name)
    tgs = []
    for i in range(inp['vis'].shape[0]):
        o = A.augment(inp, i, g)
        for k in ('center', 'scale', 'rotation', 'flipped'):
            assert np.array_equal(np.asarray(o[k]), GOLD['%s/%s' % (name, k)][i]), (name, i, k, o[k], GOLD['%s/%s' % (name, k)][i])
        assert np.array_equal(o['vis'], GOLD[name + '/joints_vis'][i])
        np.testing.assert_allclose(o['trans'], GOLD[name + '/trans'][i], rtol=1e-12, atol=0)
        tg, tw = A.targets(o['joints'], o['vis'], A.group_weight(g))
        assert tw.dtype == np.float32 and np.array_equal(tw, GOLD[name + '/target_weight'][i]), (name, i)
        tgs.append(tg)
    tgs = np.stack(tgs)
    assert np.array_equal(digest(tgs), GOLD[name + '/target_sha'])
    assert np.array_equal(tgs[:3], GOLD[name + '/target_full'])


@pytest.mark.parametrize('name', list(A.GROUPS))
def test_every_case_meets_the_two_preconditions(name):
    for i in range(GOLD[name + '/trans'].shape[0]):
        d1, d2 = A.check_preconditions(GOLD[name + '/joints'][i], GOLD[name + '/joints_vis'][i], GOLD[name + '/trans'][i])
        assert d1 >= 1e-3 and d2 >= 1e-6, (name, i, d1, d2)


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler for the host build of csrc/augment_math.h')
    so = str(tmp_path_factory.mktemp('aug') / 'libaugment_host.so')
    pkg = os.path.join(ROOT, 'fast-human-pose-estimation.pytorch_amd', 'csrc')
    subprocess.check_call([cxx, '-O2', '-ffp-contract=off', '-Wno-unknown-pragmas', '-shared', '-fPIC', '-I' + pkg,
                           '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'native', 'augment_host.cpp'), '-o', so])
    return C.CDLL(so)


class SampleT(C.Structure):
    _fields_ = [('c', C.c_double * 2), ('s', C.c_double * 2), ('r', C.c_double), ('flip', C.c_int32), ('trans', C.c_double * 6),
                ('minv', C.c_double * 6)]


@pytest.mark.parametrize('name', list(A.GROUPS))
def test_host_build_of_the_kernel_arithmetic_matches_the_fixture(host_lib, name):
    """csrc/augment_math.h compiled for the host: centre, scale, rotation and flip flag exact; the matrix (closed-form
    solve instead of the fixture's LU) to 1e-11 relative to the largest entry of its row; its inverse is bit for bit
    lib.utils.transforms.invert_affine of the matrix it returned."""
    from fpd_amd import runtime as R
    from oracle import infer_ref
    assert host_lib.augment_host_sizeof() == C.sizeof(SampleT)
    g, inp = A.GROUPS[name], inputs(name)
    B, J = inp['vis'].shape
    pairs, upper = A.tables(J)
    table = (R.AugImgT * B)()
    for i in range(B):
        table[i].h, table[i].w = int(inp['shapes'][i, 0]), int(inp['shapes'][i, 1])
    joints, vis = np.ascontiguousarray(inp['joints']), np.ascontiguousarray(inp['vis'], np.float32)
    center, scale = inp['center'].astype(np.float64), inp['scale'].astype(np.float64)
    up = np.array([1 if k in upper else 0 for k in range(J)], np.int32)
    draws = np.ascontiguousarray(inp['draws'])
    a = R.AugmentT()
    a.db.N, a.db.J, a.db.box_f32 = B, J, int(inp['center'].dtype == np.float32)
    a.db.images, a.db.joints, a.db.vis = C.addressof(table), joints.ctypes.data, vis.ctypes.data
    a.db.center, a.db.scale, a.db.upper = center.ctypes.data, scale.ctypes.data, up.ctypes.data
    a.db.aspect_ratio, a.db.pixel_std = A.ASPECT, 200.0
    a.B, a.is_train, a.flip, a.num_joints_half_body = B, int(g['train']), int(g['flip']), g['num_half']
    a.draw_stride, a.out_w, a.out_h = 6, A.IMAGE_SIZE[0], A.IMAGE_SIZE[1]
    a.sf, a.rf, a.prob_half_body, a.draws = g['sf'], g['rf'], g['prob_half'], draws.ctypes.data
    for i in range(B):
        o = SampleT()
        host_lib.augment_host(C.byref(a), i, i, C.byref(o))
        assert np.array_equal(np.array(o.c), GOLD[name + '/center'][i]) and np.array_equal(np.array(o.s), GOLD[name + '/scale'][i]), (name, i)
        assert o.r == GOLD[name + '/rotation'][i] and o.flip == GOLD[name + '/flipped'][i], (name, i)
        t, ref = np.array(o.trans).reshape(2, 3), GOLD[name + '/trans'][i]
        assert (np.abs(t - ref) <= 1e-11 * np.abs(ref).max(1, keepdims=True)).all(), (name, i, t - ref)
        assert np.array_equal(np.array(o.minv).reshape(2, 3), infer_ref.invert_affine(t))


def test_abi_has_the_augmentation_structs_and_symbols():
    from fpd_amd import runtime as R
    lib = R.lib()
    for name in ('fpd_aug_img_t', 'fpd_aug_db_t', 'fpd_aug_crop_t', 'fpd_augment_t', 'fpd_warp_aug_t', 'fpd_targets_w_t'):
        assert lib.fpd_abi_sizeof(name.encode()) == C.sizeof(R._STRUCTS[name]) > 0, name
    assert C.sizeof(R.AugImgT) == 24 and C.sizeof(R.AugCropT) == 56
    for sym in ('fpd_augment_params', 'fpd_warp_affine_aug', 'fpd_render_targets_w'):
        assert hasattr(lib, sym)
    assert lib.fpd_abi_version() == 2
    # validation fails loudly without touching a device
    a = R.AugmentT()
    assert lib.fpd_augment_params(a, None) != 0 and b'null' in lib.fpd_last_error()
    w = R.WarpAugT()
    assert lib.fpd_warp_affine_aug(w, None) != 0 and b'null' in lib.fpd_last_error()
    t = R.TargetsWT()
    assert lib.fpd_render_targets_w(t, None) != 0 and b'null' in lib.fpd_last_error()


def test_config_defaults_are_the_references():
    from fpd_amd.lib.config import _defaults
    d = _defaults().DATASET
    assert (d.FLIP, d.SCALE_FACTOR, d.ROT_FACTOR, d.PROB_HALF_BODY, d.NUM_JOINTS_HALF_BODY) == (True, 0.25, 30, 0.0, 8)
    assert d.NUM_SCENES == 64 and d.DATASET == 'synthetic'


def test_scene_generator_is_seeded_and_follows_box2cs():
    from fpd_amd import synth
    a, b = synth.make_scenes(5, 3, 17, size=(80, 120)), synth.make_scenes(5, 3, 17, size=(80, 120))
    assert all(np.array_equal(x, y) for x, y in zip(a['images'], b['images'])) and np.array_equal(a['joints'], b['joints'])
    assert a['center'].dtype == np.float32 and a['joints_weight'].shape == (17,) and a['flip_pairs'] == A.COCO_PAIRS
    assert len({im.shape for im in a['images']}) > 1 and all(im.dtype == np.uint8 and 80 <= im.shape[0] <= 120 for im in a['images'])
    m = synth.make_scenes(5, 2, 16, size=(80, 120), aspect_ratio=0.75)
    assert m['center'].dtype == np.float64 and m['joints_weight'] is None and tuple(m['upper_body_ids']) == A.MPII_UPPER
    assert np.allclose(m['scale'][:, 0] / m['scale'][:, 1], 0.75)
