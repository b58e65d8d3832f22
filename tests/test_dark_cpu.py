"""DARK sub-pixel decoding, the parts that need no GPU: the numpy restatement's own properties (tests/_dark_ref.py), a HOST
build of the kernel's Newton step (csrc/dark_math.h) against numpy bit for bit and under the host sanitizers as a
stand-alone program, the ABI surface and refusals of fpd_dark_refine, and the config keys."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _dark_ref as D
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'fast-human-pose-estimation.pytorch_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'native', 'dark_host.cpp')
_vp = C.c_void_p


def _cxx():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler for the host build of csrc/dark_math.h')
    return cxx


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('dark') / 'libdark_host.so')
    subprocess.check_call([_cxx(), '-O2', '-ffp-contract=off', '-Wno-unknown-pragmas', '-shared', '-fPIC', '-I' + CSRC, SRC, '-o', so])
    lib = C.CDLL(so)
    lib.dark_step_host.argtypes = [_vp, _vp]
    lib.dark_apply_host.restype = C.c_float
    lib.dark_apply_host.argtypes = [C.c_float, C.c_double]
    lib.dark_tap_host.argtypes = [C.c_int, _vp]
    return lib


# ---- the restatement's own properties ----

@pytest.mark.parametrize('k', [9, 11, 17, 31])
def test_taps_sum_to_one_and_are_symmetric(k):
    from fpd_amd.lib.core.inference import dark_taps
    t = D.taps(k)
    assert t.dtype == np.float64 and len(t) == k and abs(t.sum() - 1.0) < 1e-15
    assert np.array_equal(t, t[::-1]) and t.argmax() == k // 2 and (np.diff(t[:k // 2 + 1]) > 0).all()
    assert dark_taps(k).tobytes() == t.tobytes()              # the package hands the kernel the same float64 taps


@pytest.mark.parametrize('name', ['S1', 'S2', 'S4'])
def test_the_published_padded_and_reflected_blur_is_the_zero_border_blur_bit_for_bit(name):
    maps, _, k = D.random_case(name)
    for m in maps.reshape((-1,) + maps.shape[2:]):
        assert D.blur_published(m.astype(np.float64), k).tobytes() == D.blur(m, k).tobytes()


def test_median_distance_to_the_true_centre_is_below_a_quarter_of_the_arg_maxs_at_64x48():
    """0.016 against 0.40 heat-map pixels was seen on such maps; a quarter needs no measurement."""
    n, j, h, w, k = D.SHAPES['S3']
    cases = [D.random_case('S3', seed=100 + s) for s in range(6)]
    maps, cen = np.concatenate([c[0] for c in cases]), np.concatenate([c[1] for c in cases])
    arg, _, _ = D.argmax_coords(maps)
    dark, _, refined, _ = D.decode(maps, k)
    assert refined.all()
    d_arg = np.median(np.linalg.norm(arg - cen, axis=-1))
    d_dark = np.median(np.linalg.norm(dark - cen, axis=-1))
    print('median distance: arg-max %.4f, DARK %.4f heat-map pixels over %d maps' % (d_arg, d_dark, arg.shape[0] * arg.shape[1]))
    assert d_dark < 0.25 * d_arg


@pytest.mark.parametrize('name', sorted(D.SHAPES))
def test_random_cases_meet_their_input_condition_and_float32_stays_close(name):
    maps, _, k = D.random_case(name)                           # asserts: all refined, |det| >= MIN_DET
    c64, v64, r64, _ = D.decode(maps, k)
    c32, v32, r32, _ = D.decode(maps, k, np.float32)
    assert np.array_equal(r64, r32) and v64.tobytes() == v32.tobytes()
    assert np.abs(c64.astype(np.float64) - c32).max() < 1e-4


def test_designed_cases_sit_on_both_sides_of_both_guards():
    maps, names = D.designed_case()
    coords, maxvals, refined, _ = D.decode(maps, 11)
    arg, _, _ = D.argmax_coords(maps)
    assert np.array_equal(refined[0], D.designed_expectation(names))
    keep = refined[0] == 0
    assert coords[0][keep].tobytes() == arg[0][keep].tobytes()
    q = names.index('spike')                                    # the clamp is active around the spike; the step is exactly zero
    assert (D.blur(maps[0, q], 11) * (maxvals[0, q] / D.blur(maps[0, q], 11).max()) < 1e-10).any()
    assert refined[0, q] == 1 and coords[0, q].tobytes() == arg[0, q].tobytes()


# ---- the host build of csrc/dark_math.h ----

def _step(host_lib, v):
    v = np.ascontiguousarray(v, np.float64)
    off = np.full(2, 7.0)
    r = host_lib.dark_step_host(v.ctypes.data, off.ctypes.data)
    return r, off


def test_host_build_of_the_newton_step_is_numpys_bit_for_bit(host_lib):
    for i, (a, b) in enumerate(zip((0, 1, -1, 0, 0, 2, -2, 0, 0, 1, 1, -1, -1), (0, 0, 0, 1, -1, 0, 0, 2, -2, 1, -1, 1, -1))):
        d = (C.c_int * 2)()
        host_lib.dark_tap_host(i, d)
        assert (d[0], d[1]) == (a, b)
    checked = 0
    for name in ('S1', 'S2', 'S3', 'S4'):
        maps, _, k = D.random_case(name)
        n, j, h, w = maps.shape
        arg, maxvals, _ = D.argmax_coords(maps)
        B = D.blur(maps, k)
        for a in range(n):
            for b in range(j):
                px, py = int(arg[a, b, 0]), int(arg[a, b, 1])
                L = np.log(np.maximum(B[a, b] * (np.float64(maxvals[a, b]) / B[a, b].max()), 1e-10))
                v = D.gather13(L, px, py)
                want = D.newton(v)
                r, off = _step(host_lib, v)
                assert r == want[0] == 1
                assert off.tobytes() == np.array([want[1], want[2]], np.float64).tobytes(), (name, a, b)
                for c, o in zip(arg[a, b], off):
                    ref = np.array([c], np.float32)
                    ref += np.array([o])                         # numpy's float32 += float64
                    assert np.float32(host_lib.dark_apply_host(float(c), float(o))).tobytes() == ref[0].tobytes()
                checked += 1
    assert checked == 6 + 10 + 17 + 6


def test_host_build_takes_no_step_where_the_determinant_is_zero_and_holds_the_guards(host_lib):
    r, off = _step(host_lib, np.full(13, -2.5))                # thirteen equal values
    assert r == 0 and off.tolist() == [0.0, 0.0] and D.newton(np.full(13, -2.5))[0] == 0
    for w, h in ((12, 16), (5, 5), (4, 9)):
        for px in range(w):
            for py in range(h):
                assert host_lib.dark_interior_host(px, py, w, h) == int(1 < px < w - 2 and 1 < py < h - 2)


def test_the_header_walks_seeded_cases_clean_under_the_host_sanitizers(tmp_path):
    """The same text with a small main, built with -fsanitize=address,undefined and run as a program of its own."""
    exe = str(tmp_path / 'dark_san')
    subprocess.check_call([_cxx(), '-O1', '-g', '-ffp-contract=off', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DDARK_MAIN', '-I' + CSRC, SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b'cases ok' in r.stdout, r.stdout.decode()


# ---- the C ABI ----

def test_abi_has_dark_refine_and_it_refuses_bad_arguments_without_a_device():
    from fpd_amd import runtime as R
    lib = R.lib()
    assert lib.fpd_abi_sizeof(b'fpd_dark_t') == C.sizeof(R.DarkT) > 0
    assert lib.fpd_abi_version() == R.ABI_VERSION == 2
    assert hasattr(lib, 'fpd_dark_refine')

    def args(form):
        a = R.DarkT()
        a.N, a.J, a.H, a.W, a.layout, a.ksize, a.rows = 2, 16, 8, 8, R.DARK_NHWC, 11, 2
        a.hm, a.taps, a.coords, a.maxvals = 0x1000, 0x2000, 0x3000, 0x4000      # never dereferenced: every case is refused before a launch
        if form == 'a':
            a.trans, a.preds = 0x5000, 0x6000
        if form == 'b':
            a.center, a.scale, a.all_preds = 0x7000, 0x8000, 0x9000
        return a

    def refused(a, word):
        assert lib.fpd_dark_refine(a, None) < 0 and word in lib.fpd_last_error(), (word, lib.fpd_last_error())

    assert lib.fpd_dark_refine(None, None) < 0
    for form in ('a', 'b', None):
        for field in ('hm', 'taps'):
            a = args(form)
            setattr(a, field, None)
            refused(a, b'null')
        for k in (0, 7, 10, 12, 33, -11):
            a = args(form)
            a.ksize = k
            refused(a, b'ksize')
        a = args(form)
        a.J = R.MAX_JOINTS + 1
        refused(a, b'J <=')
        a = args(form)
        a.H, a.W = 128, 129                                    # one row more than the 128x128 of the LDS limit
        refused(a, b'LDS')
        a = args(form)
        a.layout = 2
        refused(a, b'layout')
    a = args('a')
    a.center, a.scale, a.all_preds = 0x7000, 0x8000, 0x9000
    refused(a, b'both')
    a = args(None)
    a.coords = None
    refused(a, b'no output')
    for field in ('trans', 'preds'):
        a = args('a')
        setattr(a, field, None)
        refused(a, b'go together')
    for field in ('center', 'scale', 'all_preds'):
        a = args('b')
        setattr(a, field, None)
        refused(a, b'go together')
    a = args('b')
    a.row0 = -1
    refused(a, b'negative')
    a = args('b')
    a.row0 = 1                                                 # rows 1..2 of 2
    refused(a, b'outside')


def test_python_refuses_a_cpu_tensor_and_a_bad_blur_size():
    import torch

    from fpd_amd.lib.core import inference as I
    from fpd_amd.runtime import FpdError
    with pytest.raises(FpdError):
        I.final_preds_device(torch.zeros(1, 2, 16, 12), None, False, dark=11)
    for k in (10, 7, 33, 11.5, True):
        with pytest.raises(FpdError):
            I.dark_ksize(k)
    assert I.dark_ksize(0) == 0 and I.dark_ksize(None) == 0 and I.dark_ksize(False) == 0 and I.dark_ksize(17) == 17


# ---- config ----

def test_config_defaults_keep_dark_off_and_a_yaml_turns_it_on(tmp_path):
    from fpd_amd.lib.config import _defaults
    from fpd_amd.lib.core.inference import dark_config
    from fpd_amd.runtime import FpdError
    cfg = _defaults()
    assert cfg.TEST.DARK is False and cfg.TEST.BLUR_KERNEL == 11 and dark_config(cfg) == 0
    y = tmp_path / 'dark.yaml'
    y.write_text('TEST:\n  DARK: true\n  BLUR_KERNEL: 17\n  POST_PROCESS: true\n')
    cfg.merge_from_file(str(y))
    assert cfg.TEST.DARK is True and cfg.TEST.BLUR_KERNEL == 17 and dark_config(cfg) == 17
    cfg = _defaults()
    cfg.merge_from_list(['TEST.DARK', 'True'])                 # the command-line form of tools/test.py, fpd_train.py, train.py
    assert dark_config(cfg) == 11
    cfg.merge_from_list(['TEST.BLUR_KERNEL', '12'])
    with pytest.raises(FpdError):
        dark_config(cfg)

    class AD(dict):                                            # the bare configs of the older tests: no DARK key at all
        __getattr__ = dict.__getitem__
    assert dark_config(AD(TEST=AD(POST_PROCESS=True))) == 0
