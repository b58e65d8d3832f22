"""Gradient accumulation (FusedFPDStep accum= / fpd_grad_accum), the parts that need no GPU: a HOST build of the kernel's
arithmetic (csrc/grad_accum_math.h) against the numpy restatement (tests/_accum_ref.py) bit for bit and under the host
sanitizers as a stand-alone program, the ABI surface, refusals and geometry query of fpd_grad_accum, the config key and the
step cache's key.

Denormals: the inputs are chosen so that no operand and no result is subnormal (asserted below); device denormal behaviour
is not part of the op's contract."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _accum_ref as K
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'fast-human-pose-estimation.pytorch_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'native', 'accum_host.cpp')


def _cxx():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler for the host build of csrc/grad_accum_math.h')
    return cxx


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('accum') / 'libaccum_host.so')
    subprocess.check_call([_cxx(), '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-I' + CSRC, SRC, '-o', so])
    lib = C.CDLL(so)
    lib.accum_array_host.restype = None
    lib.accum_array_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float]
    return lib


def _run(lib, grad, acc, mode, s=0.0):
    grad, acc = grad.copy(), acc.copy()
    lib.accum_array_host(grad.ctypes.data, acc.ctypes.data, grad.size, mode, np.float32(s))
    return grad, acc


# ---- the host build of csrc/grad_accum_math.h ----

def _value_sets():
    sa, sb = K.special_pairs()
    return [('normals', K.normals(4099, 1), K.normals(4099, 2)),
            ('dyadic', K.dyadic(1027, 3), K.dyadic(1027, 4)),
            ('specials', sa, sb)]


def test_host_build_of_the_three_modes_is_numpys_bit_for_bit(host_lib):
    for label, g, a in _value_sets():
        nan_acc = np.full_like(a, np.nan)
        got_g, got_a = _run(host_lib, g, nan_acc, K.FIRST)
        assert np.array_equal(K.bits(got_a), K.bits(g)) and np.array_equal(K.bits(got_g), K.bits(g)), label     # a copy of the BITS
        got_g, got_a = _run(host_lib, g, a, K.ADD)
        want = K.add(a, g)
        assert K.no_subnormal(g, a, want)
        assert K.same(got_a, want) and np.array_equal(K.bits(got_g), K.bits(g)), label
        for m in (1, 2, 3, 4, 7, 1024):
            s = K.scale_of(m)
            got_g, got_a = _run(host_lib, g, a, K.FIN, s)
            want = K.fin(a, s)
            assert K.no_subnormal(want, s)
            assert K.same(got_g, want) and np.array_equal(K.bits(got_a), K.bits(a)), (label, m)
    sa, sb = K.special_pairs()
    want = K.add(sa, sb)
    assert np.isnan(want).sum() > np.isnan(sa).sum() and np.isinf(want).any() and (want == 0).any()     # inf - inf, overflow, 0 + -0


def test_host_build_of_a_window_is_the_restatement(host_lib):
    for m in (1, 2, 3, 4, 5):
        for label, make in (('normals', K.normals), ('dyadic', K.dyadic)):
            grads = [make(2051, 10 * m + i) for i in range(m)]
            acc = np.full(2051, np.nan, np.float32)
            g, acc = _run(host_lib, grads[0], acc, K.FIRST)
            for gi in grads[1:]:
                _, acc = _run(host_lib, gi, acc, K.ADD)
            g, acc = _run(host_lib, grads[-1], acc, K.FIN, K.scale_of(m))
            want = K.window(grads)
            assert K.no_subnormal(want, acc) and K.same(g, want), (m, label)
    # what makes the identical-micro-batch tests exact: ((g + g) + g) + g = 4 g and 4 g * 0.25 = g for ANY float32 g short of overflow
    g = K.normals(4099, 5)
    assert np.array_equal(K.bits(K.window([g, g])), K.bits(g)) and np.array_equal(K.bits(K.window([g] * 4)), K.bits(g))
    assert not np.array_equal(K.bits(K.window([g] * 3)), K.bits(g))               # 1/3 is not a float32: k = 3 does round


def test_the_header_walks_its_cases_clean_under_the_host_sanitizers(tmp_path):
    """The same text with a small main, built with -fsanitize=address,undefined and run as a program of its own."""
    exe = str(tmp_path / 'accum_san')
    subprocess.check_call([_cxx(), '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DACCUM_MAIN', '-I' + CSRC, SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b'cases ok' in r.stdout, r.stdout.decode()


# ---- the C ABI ----

@pytest.fixture(scope='module')
def runtime():
    from fpd_amd import runtime as R
    if not os.path.exists(R.LIB_PATH):
        subprocess.check_call(['bash', os.path.join(os.path.dirname(R.LIB_PATH), 'build.sh')])
    R.lib()
    return R


GRAD, ACC, SCALE = 0x10000000, 0x40000000, 0x30000      # never dereferenced: every call is a query or refused


def _args(R, n=4099, off=0, mode=None):
    a = R.GradAccumT()
    a.n, a.grad, a.acc, a.scale_dev = n, GRAD + 4 * off, ACC + 4 * off, SCALE
    a.mode = R.ACCUM_FIN if mode is None else mode
    return a


def test_abi_has_fpd_grad_accum_with_the_mirrors_size_and_the_plan_takes_the_op(runtime):
    R, lib = runtime, runtime.lib()
    assert lib.fpd_abi_sizeof(b'fpd_grad_accum_t') == C.sizeof(R.GradAccumT) == 40
    assert lib.fpd_abi_version() == R.ABI_VERSION == 2 and R.OP_GRAD_ACCUM == 30 and R.OP_GRAD_CLIP == 29
    assert (R.ACCUM_FIRST, R.ACCUM_ADD, R.ACCUM_FIN) == (K.FIRST, K.ADD, K.FIN) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, 'include', 'fpd_amd.h')).read()
    assert 'FPD_OP_GRAD_ACCUM = 30' in hdr and '} fpd_grad_accum_t;' in hdr and '#define FPD_ABI_VERSION 2' in hdr
    assert 'int fpd_grad_accum(const fpd_grad_accum_t*' in hdr and 'int fpd_grad_accum_geometry(const fpd_grad_accum_t*' in hdr
    assert 'FPD_ACCUM_FIRST = 0, FPD_ACCUM_ADD = 1, FPD_ACCUM_FIN = 2' in hdr
    p = lib.fpd_plan_create()
    assert lib.fpd_plan_add(p, R.OP_GRAD_ACCUM, C.byref(_args(R)), C.sizeof(R.GradAccumT)) == 0
    assert lib.fpd_plan_add(p, R.OP_GRAD_ACCUM, C.byref(_args(R)), C.sizeof(R.GradAccumT) - 8) < 0
    lib.fpd_plan_destroy(p)


def _expected_geometry(n, aligned):
    nvec = n // 4 if aligned else 0
    work = max(nvec, n - 4 * nvec)
    return min(max(-(-work // 256), 1), 4096), 4 * nvec


CAP = 4 * 256 * 4096      # elements of an aligned arena that fill the capped grid exactly once


@pytest.mark.parametrize('off', [0, 1])
def test_geometry_query_over_alignment_the_cap_and_the_two_models(runtime, off):
    R, lib = runtime, runtime.lib()
    for mode in (R.ACCUM_FIRST, R.ACCUM_ADD, R.ACCUM_FIN):
        got = {}
        for n in (0, 1, 3, 255, 256, 257, CAP, CAP + 7, 3287936, 28536113):
            blocks, vec = C.c_int32(-1), C.c_int64(-1)
            assert lib.fpd_grad_accum_geometry(_args(R, n, off, mode), blocks, vec) == 0, lib.fpd_last_error()
            assert (blocks.value, vec.value) == _expected_geometry(n, off == 0), n
            got[n] = (blocks.value, vec.value)
        if off == 0:
            assert got[0] == (1, 0) and got[3] == (1, 0) and got[255] == (1, 252) and got[257] == (1, 256)
            assert got[CAP] == (4096, CAP) and got[CAP + 7] == (4096, CAP + 4)
            assert got[3287936] == (3211, 3287936) and got[28536113] == (4096, 28536112)
        else:
            assert got[0] == (1, 0) and got[255] == (1, 0) and got[256] == (1, 0) and got[257] == (2, 0)
            assert got[CAP] == (4096, 0) and got[3287936] == (4096, 0)
    # one base aligned and the other not: element by element
    a = _args(R, 4099, 0)
    a.acc = ACC + 4
    blocks, vec = C.c_int32(-1), C.c_int64(-1)
    assert lib.fpd_grad_accum_geometry(a, blocks, vec) == 0 and (blocks.value, vec.value) == (17, 0)


def refusals(R):
    """(label, mutated arguments, word of the message): every case fpd_grad_accum refuses before it launches."""
    out = []

    def case(label, word, **kw):
        a = _args(R, mode=kw.pop('mode', None))
        for k, v in kw.items():
            setattr(a, k, v)
        out.append((label, a, word))
    case('negative n', b'negative', n=-1)
    case('n too large', b'too large', n=1 << 60)
    case('null grad', b'null', grad=None)
    case('null acc', b'null', acc=None)
    case('null acc in FIRST', b'null', acc=None, mode=R.ACCUM_FIRST)
    case('grad misaligned', b'misaligned', grad=GRAD + 2)
    case('acc misaligned', b'misaligned', acc=ACC + 1)
    case('scale misaligned', b'misaligned', scale_dev=SCALE + 2)
    case('acc is grad', b'overlaps', acc=GRAD)
    case('acc over the end of grad', b'overlaps', acc=GRAD + 4 * 4098)
    case('acc over the head of grad', b'overlaps', acc=GRAD - 4 * 4098)
    case('scale inside grad', b'overlaps', scale_dev=GRAD + 16)
    case('scale inside acc', b'overlaps', scale_dev=ACC + 4 * 4098)
    case('scale inside acc in ADD', b'overlaps', scale_dev=ACC, mode=R.ACCUM_ADD)
    case('mode 3', b'mode', mode=3)
    case('mode -1', b'mode', mode=-1)
    case('null scale in FIN', b'scale_dev', scale_dev=None)
    return out


def test_fpd_grad_accum_refuses_bad_arguments_without_a_device(runtime):
    R, lib = runtime, runtime.lib()
    assert lib.fpd_grad_accum(None, None) < 0 and b'null' in lib.fpd_last_error()
    blocks, vec = C.c_int32(), C.c_int64()
    assert lib.fpd_grad_accum_geometry(None, blocks, vec) < 0 and b'null' in lib.fpd_last_error()
    for label, a, word in refusals(R):
        assert lib.fpd_grad_accum_geometry(a, blocks, vec) < 0 and word in lib.fpd_last_error(), (label, lib.fpd_last_error())
        assert lib.fpd_grad_accum(a, None) < 0 and word in lib.fpd_last_error(), label
    # what is NOT refused: n = 0 with null arenas, a null scale_dev in FIRST and ADD, adjacent ranges
    a = _args(R, n=0)
    a.grad = a.acc = None
    assert lib.fpd_grad_accum_geometry(a, blocks, vec) == 0 and (blocks.value, vec.value) == (1, 0)
    for mode in (R.ACCUM_FIRST, R.ACCUM_ADD):
        a = _args(R, mode=mode)
        a.scale_dev = None
        assert lib.fpd_grad_accum_geometry(a, blocks, vec) == 0, lib.fpd_last_error()
    a = _args(R)
    a.acc, a.scale_dev = GRAD + 4 * a.n, GRAD - 4
    assert lib.fpd_grad_accum_geometry(a, blocks, vec) == 0 and (blocks.value, vec.value) == (17, 0)      # acc's base is 12 mod 16


# ---- config and the step cache's key ----

def test_config_key_defaults_to_one_and_the_shipped_yaml_sets_four():
    from fpd_amd.lib.config import _defaults
    cfg = _defaults()
    assert cfg.TRAIN.ACCUM_STEPS == 1 and isinstance(cfg.TRAIN.ACCUM_STEPS, int)
    cfg.merge_from_list(['TRAIN.ACCUM_STEPS', '4'])
    assert cfg.TRAIN.ACCUM_STEPS == 4 and isinstance(cfg.TRAIN.ACCUM_STEPS, int)
    shipped = _defaults()
    shipped.merge_from_file(os.path.join(ROOT, 'experiments', 'fpd_synthetic', 'hg4x128_student_accum.yaml'))
    assert shipped.TRAIN.ACCUM_STEPS == 4 and shipped.TRAIN.BATCH_SIZE_PER_GPU == 32
    plain = _defaults()
    plain.merge_from_file(os.path.join(ROOT, 'experiments', 'fpd_synthetic', 'hg4x128_student.yaml'))
    assert plain.TRAIN.ACCUM_STEPS == 1
    # what the tools pass to the loop: the key as it stands, a value below 1 raises
    from fpd_amd.lib.utils.utils import get_accum_steps
    assert get_accum_steps(plain) == 1 and get_accum_steps(shipped) == 4
    for bad in ('0', '-2'):
        cfg.merge_from_list(['TRAIN.ACCUM_STEPS', bad])
        with pytest.raises(ValueError, match='ACCUM_STEPS'):
            get_accum_steps(cfg)


class _Student:
    """What fused_step_for touches of a student before it builds the step."""
    cfg_hg = {}

    def device_state(self):
        return None


class _Optimizer:
    param_groups = [{'lr': 1e-3}]


def test_step_cache_key_tells_accumulation_lengths_apart(monkeypatch):
    from fpd_amd.lib.core import function as F
    built = []

    class FakeStep:
        def __init__(self, *a, **kw):
            built.append(kw.get('accum'))
    monkeypatch.setattr(F.E, 'FusedFPDStep', FakeStep)
    s, opt, shape = _Student(), _Optimizer(), (2, 3, 128, 128)
    steps = {k: F.fused_step_for(s, None, opt, shape, 0.0, accum=k) for k in (None, 1, 2, 3)}
    assert steps[None] is steps[1] and built == [None, 2, 3]                 # None and 1 are one step, built once
    assert steps[1] is not steps[2] and steps[2] is not steps[3]
    keys = list(s._fused_steps)
    assert len(keys) == 3 and len(set(keys)) == 3
    assert sorted(k[-1] for k in keys if k[-1] and k[-1][0] == 'accum') == [('accum', 2), ('accum', 3)]
    assert not any('accum' in str(k) for k in keys if k[-1] not in (('accum', 2), ('accum', 3)))     # k = 1: today's key
    assert F.fused_step_for(s, None, opt, shape, 0.0, accum=2) is steps[2] and built == [None, 2, 3]      # a hit builds nothing
    assert F.fused_step_for(s, None, opt, shape, 0.0) is steps[1]
