"""DARK's unbiased target encoding, the parts that need no GPU: a HOST build of the kernel's decisions (csrc/encode_math.h)
against the numpy restatement (tests/_encode_ref.py) bit for bit and under the host sanitizers as a stand-alone program,
the ABI surface and refusals of fpd_render_targets_unbiased, the config key, and the accuracy condition that motivates
the encoding: DARK decodes unbiased targets two orders of magnitude closer than biased ones."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _dark_ref as D
from tests import _encode_ref as E
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'fast-human-pose-estimation.pytorch_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'native', 'encode_host.cpp')
_vp = C.c_void_p


class Place(C.Structure):
    _fields_ = [('mu_x', C.c_double), ('mu_y', C.c_double), ('ulx', C.c_int32), ('uly', C.c_int32), ('brx', C.c_int32),
                ('bry', C.c_int32), ('outside', C.c_int32), ('drawn', C.c_int32), ('w', C.c_float), ('weight', C.c_float)]


def _cxx():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler for the host build of csrc/encode_math.h')
    return cxx


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('encode') / 'libencode_host.so')
    subprocess.check_call([_cxx(), '-O2', '-ffp-contract=off', '-Wno-unknown-pragmas', '-shared', '-fPIC', '-I' + CSRC, SRC, '-o', so])
    lib = C.CDLL(so)
    lib.encode_place_host.restype = None
    lib.encode_place_host.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                      C.c_float, C.POINTER(Place)]
    lib.encode_factor_host.restype = C.c_double
    lib.encode_factor_host.argtypes = [C.c_int, C.c_double, C.c_int]
    lib.encode_value_host.restype = C.c_float
    lib.encode_value_host.argtypes = [C.c_double, C.c_double]
    return lib


def _host_place(lib, joints, vis, size, stride, sigma, jw):
    b, j = vis.shape
    out = {}
    for a in range(b):
        for k in range(j):
            p = Place()
            lib.encode_place_host(joints[a, k, 0], joints[a, k, 1], stride[0], stride[1], sigma, size[0], size[1], float(vis[a, k]),
                                  int(jw is not None), float(jw[k]) if jw is not None else 0.0, p)
            out[a, k] = p
    return out


def _same_decisions(lib, joints, vis, size, stride, sigma, jw):
    want = E.place(joints, vis, size, stride, sigma, jw)
    got = _host_place(lib, joints, vis, size, stride, sigma, jw)
    for (a, k), p in got.items():
        where = (a, k, joints[a, k].tolist())
        assert np.float64(p.mu_x).tobytes() == want['mu'][a, k, 0].tobytes() and np.float64(p.mu_y).tobytes() == want['mu'][a, k, 1].tobytes(), where
        assert bool(p.outside) == bool(want['outside'][a, k]) and bool(p.drawn) == bool(want['drawn'][a, k]), where
        if np.isfinite(want['mu'][a, k]).all():
            assert (p.ulx, p.uly, p.brx, p.bry) == tuple(want['ul'][a, k]) + tuple(want['br'][a, k]), where
        assert np.float32(p.w).tobytes() == want['w'][a, k].tobytes() and np.float32(p.weight).tobytes() == want['weight'][a, k].tobytes(), where
    return want


# ---- the host build of csrc/encode_math.h ----

@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('name', sorted(E.SHAPES))
def test_host_build_of_the_decisions_is_numpys_bit_for_bit_on_seeded_joints(host_lib, name, weighted):
    joints, vis, jw, size, stride, sigma = E.random_case(name)
    want = _same_decisions(host_lib, joints, vis, size, stride, sigma, jw if weighted else None)
    assert want['drawn'].any()
    if name == 'E3':                                           # 17 joints: both outcomes of both tests occur
        assert want['outside'].any() and (~want['drawn'] & ~want['outside']).any()


@pytest.mark.parametrize('weighted', [False, True])
def test_host_build_holds_the_designed_cases_on_both_sides_of_every_guard(host_lib, weighted):
    joints, vis, names, size, stride, sigma = E.designed_case()
    jw = np.linspace(0.5, 1.5, len(names)).astype(np.float32) if weighted else None
    want = _same_decisions(host_lib, joints, vis, size, stride, sigma, jw)
    outside, drawn = E.designed_expectation(names)
    assert np.array_equal(want['outside'][0], outside) and np.array_equal(want['drawn'][0], drawn), names
    # truncation, not a floor: at mu = -tmp - 1.5 the box ends at (int)(-0.5) = 0, a floor would say -1 and outside
    q = names.index('x: mu = -tmp - 1.5 (inside under truncation)')
    assert want['br'][0, q, 0] == 0 and np.floor(want['mu'][0, q, 0] + 3 * sigma + 1) == -1
    q = names.index('vis = 0.5')                               # weight 0.5 and an all-zero map
    assert want['w'][0, q] == np.float32(0.5) and not want['drawn'][0, q] and not want['outside'][0, q]
    tg, tw, _, _ = E.unbiased(joints, vis, size, stride, sigma, jw)
    assert tw[0, q] == np.float32(0.5) * (jw[q] if weighted else np.float32(1)) and not tg[0, q].any() and tg[0, names.index('vis = 1')].max() > 0.8


def test_host_build_of_the_separable_value_is_within_the_tolerance_of_the_direct_expression(host_lib):
    """The product of the two float64 factors against float32(exp(float64 expression)): the derivation says one float32 step."""
    for name in ('E1', 'E5', 'E4'):
        joints, vis, _, size, stride, sigma = E.random_case(name)
        _, _, e, p = E.unbiased(joints[:1, :2], vis[:1, :2], size, stride, sigma)
        w, h = size
        for k in range(2):
            if not p['drawn'][0, k]:
                continue
            ex = [host_lib.encode_factor_host(x, p['mu'][0, k, 0], sigma) for x in range(w)]
            ey = [host_lib.encode_factor_host(y, p['mu'][0, k, 1], sigma) for y in range(h)]
            got = np.array([[host_lib.encode_value_host(ex[x], ey[y]) for x in range(w)] for y in range(h)], np.float32)
            ok, unequal, steps, small = E.within(got, e[0, k])
            print('%s joint %d: %d of %d values not bit-equal, worst %d float32 steps, %.3e below 2^-126' % (name, k, unequal, got.size, steps, small))
            assert ok, (name, k, unequal, steps, small)


def test_the_header_walks_seeded_cases_clean_under_the_host_sanitizers(tmp_path):
    """The same text with a small main, built with -fsanitize=address,undefined and run as a program of its own."""
    exe = str(tmp_path / 'encode_san')
    subprocess.check_call([_cxx(), '-O1', '-g', '-ffp-contract=off', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DENCODE_MAIN', '-I' + CSRC, SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b'cases ok' in r.stdout, r.stdout.decode()


# ---- the restatement's own properties ----

def test_unbiased_and_biased_targets_agree_on_pixel_centres_and_differ_between_them():
    """A joint on a pixel centre: inside the patch both encodings draw the same Gaussian (to float32 rounding); the unbiased
    one goes on beyond the patch.  Off centre the maps differ."""
    size, stride, sigma = (12, 16), (4.0, 4.0), 1
    joints = np.array([[[5 * 4.0, 7 * 4.0, 0], [5.4 * 4.0, 7.3 * 4.0, 0]]])
    vis = np.ones((1, 2), np.float32)
    u, uw, _, _ = E.unbiased(joints, vis, size, stride, sigma)
    b, bw = E.biased(joints, vis, size, stride, sigma)
    assert np.array_equal(uw, bw)
    patch = b[0, 0] > 0
    assert patch.sum() == 49 and np.abs(u[0, 0][patch] - b[0, 0][patch]).max() < 1e-7 and (u[0, 0][~patch] > 0).any()
    assert u[0, 0].max() == 1.0 and u[0, 1].max() < 1.0 and np.abs(u[0, 1] - b[0, 1]).max() > 0.05


# ---- the C ABI ----

def test_abi_has_render_targets_unbiased_and_it_refuses_bad_arguments_without_a_device():
    from fpd_amd import runtime as R
    lib = R.lib()
    assert lib.fpd_abi_sizeof(b'fpd_targets_unbiased_t') == C.sizeof(R.TargetsUnbiasedT) > 0
    assert lib.fpd_abi_version() == R.ABI_VERSION == 2
    assert hasattr(lib, 'fpd_render_targets_unbiased')

    def args():
        a = R.TargetsUnbiasedT()
        a.B, a.J, a.H, a.W, a.sigma, a.stride_x, a.stride_y = 2, 16, 64, 48, 2, 4.0, 4.0
        a.joints, a.vis, a.joints_weight, a.target, a.weight = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000    # never dereferenced: every case is refused before a launch
        return a

    def refused(a, word):
        assert lib.fpd_render_targets_unbiased(a, None) < 0 and word in lib.fpd_last_error(), (word, lib.fpd_last_error())

    assert lib.fpd_render_targets_unbiased(None, None) < 0 and b'null' in lib.fpd_last_error()
    for field in ('joints', 'vis', 'target', 'weight'):
        a = args()
        setattr(a, field, None)
        refused(a, b'null')
    for field in ('B', 'J', 'H', 'W'):
        for v in (0, -3):
            a = args()
            setattr(a, field, v)
            refused(a, b'bad dims')
    for s in (0, -2):
        a = args()
        a.sigma = s
        refused(a, b'sigma')
    for field in ('stride_x', 'stride_y'):
        for v in (0.0, -4.0, float('nan')):
            a = args()
            setattr(a, field, v)
            refused(a, b'stride')
    a = args()
    a.H, a.W = 8000, 193                                       # one factor more than the LDS holds
    refused(a, b'LDS')


# ---- config ----

def test_config_default_is_gaussian_and_a_yaml_or_the_command_line_turns_unbiased_on(tmp_path):
    from fpd_amd.lib.config import _defaults
    from fpd_amd.lib.dataset import SyntheticPose
    from fpd_amd.lib.dataset.device_pipeline import DevicePipeline, unbiased_targets
    from fpd_amd.runtime import FpdError
    cfg = _defaults()
    assert cfg.MODEL.TARGET_TYPE == 'gaussian' and not unbiased_targets(cfg)
    y = tmp_path / 'unbiased.yaml'
    y.write_text('MODEL:\n  TARGET_TYPE: gaussian_unbiased\nTEST:\n  DARK: true\n')
    cfg.merge_from_file(str(y))
    assert unbiased_targets(cfg) and cfg.TEST.DARK is True
    cfg = _defaults()
    cfg.merge_from_list(['MODEL.TARGET_TYPE', 'gaussian_unbiased'])          # the command-line form of the tools
    assert unbiased_targets(cfg)
    cfg.merge_from_list(['MODEL.TARGET_TYPE', 'coordinate'])                # any other value: as before, the reference's targets
    assert not unbiased_targets(cfg)
    shipped = _defaults()
    shipped.merge_from_file(os.path.join(ROOT, 'experiments', 'fpd_synthetic', 'hg4x128_student_dark.yaml'))
    assert unbiased_targets(shipped) and shipped.TEST.DARK is True and shipped.DATASET.DATASET == 'synthetic_aug'

    class AD(dict):                                            # the bare configs of the older tests: no TARGET_TYPE key at all
        __getattr__ = dict.__getitem__
    assert not unbiased_targets(AD(MODEL=AD(SIGMA=2)))
    # the plain synthetic set has no joints to render from: asking for the unbiased form there is an error, the default is not
    cfg = _defaults()
    cfg.MODEL.IMAGE_SIZE, cfg.MODEL.HEATMAP_SIZE = [64, 64], [16, 16]
    assert len(SyntheticPose(cfg, 4, seed=1)) == 4
    cfg.MODEL.TARGET_TYPE = 'gaussian_unbiased'
    with pytest.raises(FpdError, match='synthetic_aug'):
        SyntheticPose(cfg, 4, seed=1)
    with pytest.raises(FpdError):
        DevicePipeline((64, 64), (16, 16), 2, 'cpu', target_type='gaussian_unbiased')
    with pytest.raises(FpdError):
        DevicePipeline((64, 64), (16, 16), 2, 'cuda', target_type='unbiased')


# ---- why: encode and decode together ----

def test_dark_on_unbiased_targets_is_a_hundred_times_closer_than_on_biased_ones_at_64x48():
    """A condition, not a measurement: 200 seeded sub-pixel centres in [4, W-5] x [4, H-5] of a 64x48 map, sigma 2, k 11,
    encoded both ways by the restatement and decoded by tests/_dark_ref.decode (float64).  Every joint is refined; DARK's
    median distance to the true centre on unbiased targets is below 1/100 of its median on biased ones (2.3e-4 against 0.389
    heat-map pixels were seen); on biased targets DARK's median is within 5 % of the arg-max's, i.e. it recovers the integer."""
    size, sigma, k = (48, 64), 2, 11
    joints, vis, cen = E.accuracy_case(size)
    err = {}
    for name, enc in (('biased', E.biased), ('unbiased', E.unbiased)):
        maps = enc(joints, vis, size, (4.0, 4.0), sigma)[0]
        coords, _, refined, _ = D.decode(maps, k)
        arg, _, _ = D.argmax_coords(maps)
        assert refined.all(), name
        err[name] = (np.linalg.norm(coords - cen, axis=-1), np.linalg.norm(arg - cen, axis=-1))
        print('%-8s targets: DARK median %.3e max %.3e, arg-max median %.3e max %.3e heat-map pixels' % (
            name, np.median(err[name][0]), err[name][0].max(), np.median(err[name][1]), err[name][1].max()))
    assert np.median(err['unbiased'][0]) < 0.01 * np.median(err['biased'][0])
    assert abs(np.median(err['biased'][0]) - np.median(err['biased'][1])) <= 0.05 * np.median(err['biased'][1])
