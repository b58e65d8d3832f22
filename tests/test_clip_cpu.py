"""Global gradient-norm clipping (utils.GradClipper / fpd_grad_clip), the parts that need no GPU: a HOST build of the kernels'
arithmetic (csrc/grad_clip_math.h) against the numpy restatement (tests/_clip_ref.py) bit for bit and under the host
sanitizers as a stand-alone program, the ABI surface, refusals and geometry query of fpd_grad_clip, and the config key."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _clip_ref as K
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'fast-human-pose-estimation.pytorch_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'native', 'clip_host.cpp')


def _cxx():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler for the host build of csrc/grad_clip_math.h')
    return cxx


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('clip') / 'libclip_host.so')
    subprocess.check_call([_cxx(), '-O2', '-ffp-contract=off', '-Wno-unknown-pragmas', '-shared', '-fPIC', '-I' + CSRC, SRC, '-o', so])
    lib = C.CDLL(so)
    lib.clip_norm_host.restype = C.c_float
    lib.clip_norm_host.argtypes = [C.c_double]
    lib.clip_coef_host.restype = C.c_float
    lib.clip_coef_host.argtypes = [C.c_float, C.c_float]
    lib.clip_scale_host.restype = C.c_float
    lib.clip_scale_host.argtypes = [C.c_float, C.c_float]
    lib.clip_array_host.restype = None
    lib.clip_array_host.argtypes = [C.c_void_p, C.c_int64, C.c_float, C.c_void_p]
    return lib


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """Bit equality, a NaN matching any NaN (its payload is not compared)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


# ---- the host build of csrc/grad_clip_math.h ----

def test_host_build_of_norm_and_coefficient_is_numpys_bit_for_bit(host_lib):
    cases = K.math_cases()
    seen = set()
    for S, max_norm in cases:
        norm, got_norm = K.norm_of(S), np.float32(host_lib.clip_norm_host(S))
        assert _same(got_norm, norm), (S, float(got_norm), float(norm))
        coef, got = K.coef_of(norm, max_norm), np.float32(host_lib.clip_coef_host(norm, max_norm))
        assert _same(got, coef), (S, float(max_norm), float(got), float(coef))
        assert np.isnan(coef) or coef <= 1.0
        if np.isinf(max_norm):                                  # measure only: 1 by the formula itself, NaN for a non-finite norm
            assert coef == 1.0 if np.isfinite(norm) else np.isnan(coef)
        seen.add('nan' if np.isnan(coef) else 'one' if coef == 1.0 else 'zero' if coef == 0.0 else 'clip')
    assert seen == {'nan', 'one', 'zero', 'clip'}
    # coef on both sides of 1 by one ulp: max_norm one ulp above the float32 denominator clamps to 1, one below gives 1 - 2^-24
    for norm in (np.float32(0.37), np.float32(1.0), np.float32(7.25)):
        denom = np.float32(norm + K.EPS)
        assert denom > norm
        for m, want in ((denom, 1.0), (K.next_after(denom, True), 1.0)):
            assert np.float32(host_lib.clip_coef_host(norm, m)) == np.float32(want) == K.coef_of(norm, m)
        below = np.float32(host_lib.clip_coef_host(norm, K.next_after(denom, False)))
        assert below < 1.0 and _bits(below) == _bits(K.coef_of(norm, K.next_after(denom, False)))
    # norm + 1e-6f rounds back to norm from 32 on: max_norm == norm is then "not clipped", exactly
    for norm in (np.float32(32.0), np.float32(100.0)):
        assert np.float32(norm + K.EPS) == norm and np.float32(host_lib.clip_coef_host(norm, norm)) == 1.0
    assert np.float32(host_lib.clip_coef_host(np.float32(31.0), np.float32(31.0))) < 1.0
    # S = 0: norm 0, coef = max_norm / 1e-6f clamps to 1 for every max_norm of any use; a tiny one does clip
    assert host_lib.clip_norm_host(0.0) == 0.0 and host_lib.clip_coef_host(0.0, 1e-3) == 1.0
    assert _bits(np.float32(host_lib.clip_coef_host(0.0, 1e-7))) == _bits(K.coef_of(0.0, 1e-7)) and K.coef_of(0.0, 1e-7) < 1.0


def test_host_build_of_the_whole_op_is_the_restatement_on_arrays(host_lib):
    rng = np.random.RandomState(3)
    arrays = [rng.standard_normal(n).astype(np.float32) for n in (1, 3, 257, 4099)]
    arrays.append(K.dyadic(1027)[0])
    arrays.append(np.array([1e30, -1e30, 1e30], np.float32))
    arrays.append(np.array([1.0, np.inf, -2.0, 0.0], np.float32))
    arrays.append(np.array([1.0, np.nan, -2.0], np.float32))
    arrays.append(np.zeros(5, np.float32))
    for g0 in arrays:
        n0 = K.norm_of(K.sumsq(g0))
        for max_norm in (np.float32(np.inf), np.float32(1e-3), np.float32(n0 * np.float32(0.5)) if np.isfinite(n0) and n0 > 0 else np.float32(1.0)):
            g, out = g0.copy(), np.zeros(2, np.float32)
            host_lib.clip_array_host(g.ctypes.data, g.size, max_norm, out.ctypes.data)
            norm, coef, want = K.clip(g0, max_norm)
            # the host loop adds in array order, fsum rounds once: they agree to n * 2^-53 relative, which the float32 rounding hides
            # except at a tie -- none of these arrays sits on one
            assert _same(out[0], norm) and _same(out[1], coef) and _same(g, want), (g0.size, float(max_norm))
    assert np.isfinite(K.clip(arrays[5], 1.0)[0])                                 # 1e30 elements: no float32 square is formed
    assert np.isinf(K.clip(arrays[6], 1.0)[0]) and K.clip(arrays[6], 1.0)[1] == 0.0
    assert np.isnan(K.clip(arrays[6], np.inf)[1]) and np.isnan(K.clip(arrays[7], 1.0)[2]).all()


def test_the_header_walks_its_cases_clean_under_the_host_sanitizers(tmp_path):
    """The same text with a small main, built with -fsanitize=address,undefined and run as a program of its own."""
    exe = str(tmp_path / 'clip_san')
    subprocess.check_call([_cxx(), '-O1', '-g', '-ffp-contract=off', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DCLIP_MAIN', '-I' + CSRC, SRC, '-o', exe])
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


GRAD, PARTIAL, OUT, COUNTERS = 0x100000, 0x10000, 0x20000, 0x30000       # never dereferenced: every call is a query or refused


def _args(R, n=4099, off=0):
    a = R.GradClipT()
    a.n, a.grad, a.max_norm = n, GRAD + 4 * off, 1.0
    a.partial, a.partial_bytes = PARTIAL, 8 * 4096
    a.out, a.counters = OUT, COUNTERS
    return a


def test_abi_has_fpd_grad_clip_with_the_mirrors_size_and_the_plan_takes_the_op(runtime):
    R, lib = runtime, runtime.lib()
    assert lib.fpd_abi_sizeof(b'fpd_grad_clip_t') == C.sizeof(R.GradClipT) == 56
    assert lib.fpd_abi_version() == R.ABI_VERSION == 2 and R.OP_GRAD_CLIP == 29 and R.OP_EMA == 28
    assert C.sizeof(R.SgdT) == 80                                        # the in-place scale: no optimizer struct grew
    hdr = open(os.path.join(ROOT, 'include', 'fpd_amd.h')).read()
    assert 'FPD_OP_GRAD_CLIP = 29' in hdr and 'int fpd_grad_clip(const fpd_grad_clip_t*' in hdr
    p = lib.fpd_plan_create()
    assert lib.fpd_plan_add(p, R.OP_GRAD_CLIP, C.byref(_args(R)), C.sizeof(R.GradClipT)) == 0
    assert lib.fpd_plan_add(p, R.OP_GRAD_CLIP, C.byref(_args(R)), C.sizeof(R.GradClipT) - 8) < 0
    lib.fpd_plan_destroy(p)


def _expected_geometry(n, aligned):
    nvec = n // 4 if aligned else 0
    work = max(nvec, n - 4 * nvec)
    return min(max(-(-work // 256), 1), 4096), 4 * nvec


CAP = 4 * 256 * 4096      # elements of an aligned arena that fill the capped grid exactly once


@pytest.mark.parametrize('off', [0, 1])
def test_geometry_query_over_alignment_the_cap_and_the_two_models(runtime, off):
    R, lib = runtime, runtime.lib()
    got = {}
    for n in (0, 1, 3, 255, 256, 257, CAP, CAP + 7, 3287936, 28536113):
        blocks, vec = C.c_int32(-1), C.c_int64(-1)
        assert lib.fpd_grad_clip_geometry(_args(R, n, off), blocks, vec) == 0, lib.fpd_last_error()
        assert (blocks.value, vec.value) == _expected_geometry(n, off == 0), n
        assert 8 * blocks.value <= lib.fpd_grad_clip_scratch_bytes(n) <= 8 * 4096
        got[n] = (blocks.value, vec.value)
    if off == 0:
        assert got[0] == (1, 0) and got[3] == (1, 0) and got[255] == (1, 252) and got[257] == (1, 256)
        assert got[CAP] == (4096, CAP) and got[CAP + 7] == (4096, CAP + 4)      # one vector more than the capped grid has threads
        assert got[3287936] == (3211, 3287936) and got[28536113] == (4096, 28536112)
    else:
        assert got[0] == (1, 0) and got[255] == (1, 0) and got[256] == (1, 0) and got[257] == (2, 0)
        assert got[CAP] == (4096, 0) and got[3287936] == (4096, 0)
    assert lib.fpd_grad_clip_scratch_bytes(0) == 8 and lib.fpd_grad_clip_scratch_bytes(257) == 16


def refusals(R):
    """(label, mutated arguments, word of the message): every case fpd_grad_clip refuses before it launches."""
    out = []

    def case(label, word, **kw):
        a = _args(R)
        for k, v in kw.items():
            setattr(a, k, v)
        out.append((label, a, word))
    case('negative n', b'negative', n=-1)
    case('n too large', b'too large', n=1 << 60)
    case('null grad', b'null', grad=None)
    case('null out', b'null', out=None)
    case('null partial', b'null', partial=None)
    case('scratch too small', b'too small', partial_bytes=8 * 17 - 1)
    case('scratch misaligned', b'misaligned', partial=PARTIAL + 4)
    case('out misaligned', b'misaligned', out=OUT + 2)
    case('max_norm 0', b'max_norm', max_norm=0.0)
    case('max_norm < 0', b'max_norm', max_norm=-1.0)
    case('max_norm nan', b'max_norm', max_norm=float('nan'))
    case('out inside grad', b'overlaps', out=GRAD + 4 * 4098)
    case('partial over grad', b'overlaps', partial=GRAD - 8 * 4096 + 8)
    case('counters inside grad', b'overlaps', counters=GRAD + 16)
    case('out inside partial', b'overlaps', out=PARTIAL + 8 * 4095)
    case('counters over out', b'overlaps', counters=OUT - 16)
    case('counters inside partial', b'overlaps', counters=PARTIAL + 8)
    return out


def test_fpd_grad_clip_refuses_bad_arguments_without_a_device(runtime):
    R, lib = runtime, runtime.lib()
    assert lib.fpd_grad_clip(None, None) < 0 and b'null' in lib.fpd_last_error()
    assert lib.fpd_grad_clip_scratch_bytes(-1) < 0 and b'negative' in lib.fpd_last_error()
    assert lib.fpd_grad_clip_scratch_bytes(1 << 60) < 0 and b'too large' in lib.fpd_last_error()
    blocks, vec = C.c_int32(), C.c_int64()
    for label, a, word in refusals(R):
        assert lib.fpd_grad_clip(a, None) < 0 and word in lib.fpd_last_error(), (label, lib.fpd_last_error())
        assert lib.fpd_grad_clip_geometry(a, blocks, vec) < 0 and word in lib.fpd_last_error(), label
    # what is NOT refused: n = 0 with a null grad, no counters, max_norm = inf, scratch of exactly the size asked for, adjacent ranges
    a = _args(R, n=0)
    a.grad, a.counters, a.max_norm, a.partial_bytes = None, None, float('inf'), 8
    assert lib.fpd_grad_clip_geometry(a, blocks, vec) == 0 and (blocks.value, vec.value) == (1, 0)
    a = _args(R)
    a.partial_bytes = lib.fpd_grad_clip_scratch_bytes(a.n)
    a.out, a.counters = PARTIAL + a.partial_bytes, PARTIAL + a.partial_bytes + 8
    assert lib.fpd_grad_clip_geometry(a, blocks, vec) == 0 and (blocks.value, vec.value) == (4, 4096)


# ---- config and the clipper on a CPU model ----

class AD(dict):
    __getattr__ = dict.__getitem__


def _model():
    import torch
    from fpd_amd.lib.models import hourglass
    torch.manual_seed(0)
    return hourglass.get_pose_net(AD(MODEL=AD(NUM_JOINTS=3, DTYPE='fp32', EXTRA=AD(NUM_FEATURES=16, NUM_STACKS=2, NUM_BLOCKS=1))), is_train=True)


def test_config_key_is_off_by_default_and_a_negative_value_raises(runtime):
    from fpd_amd.lib.config import _defaults
    from fpd_amd.lib.utils.utils import GradClipper, get_grad_clipper
    cfg = _defaults()
    assert cfg.TRAIN.CLIP_GRAD_NORM == 0.0 and get_grad_clipper(cfg, None) is None       # off: the tools build no clipper
    model = _model()
    for bad in ('-1.0', '-0.5', 'nan'):
        cfg.merge_from_list(['TRAIN.CLIP_GRAD_NORM', bad])
        with pytest.raises(ValueError, match='CLIP_GRAD_NORM'):
            get_grad_clipper(cfg, model)
    for text, want in (('0.05', 0.05), ('.inf', float('inf')), ('inf', float('inf')), ('2', 2.0)):
        cfg.merge_from_list(['TRAIN.CLIP_GRAD_NORM', text])
        clip = get_grad_clipper(cfg, model)
        assert isinstance(clip, GradClipper) and clip.max_norm == want and clip.model is model
    cfg.merge_from_list(['TRAIN.CLIP_GRAD_NORM', '0'])
    assert get_grad_clipper(cfg, model) is None
    shipped = _defaults()
    shipped.merge_from_file(os.path.join(ROOT, 'experiments', 'fpd_synthetic', 'hg4x128_student_clip.yaml'))
    assert shipped.TRAIN.CLIP_GRAD_NORM == 1.0 and shipped.TRAIN.LR == 0.001 and shipped.TRAIN.EMA is False
    plain = _defaults()
    plain.merge_from_file(os.path.join(ROOT, 'experiments', 'fpd_synthetic', 'hg4x128_student.yaml'))
    assert plain.TRAIN.CLIP_GRAD_NORM == 0.0


def test_clipper_owns_scratch_result_and_counters_on_the_models_device(runtime):
    import torch
    from fpd_amd.lib.utils.utils import GradClipper
    from fpd_amd.runtime import FpdError
    model = _model()
    clip = GradClipper(model, 0.5)
    n = model.table.sizes['param']
    assert clip.partial.dtype == torch.float64 and clip.partial.numel() * 8 == runtime.lib().fpd_grad_clip_scratch_bytes(n)
    assert clip.out.tolist() == [0.0, 1.0] and clip.stats() == {'calls': 0, 'clipped': 0, 'nonfinite': 0}
    assert clip.norm() == 0.0 and clip.coef() == 1.0 and clip.out.device == model._flat['param'].device
    with pytest.raises(FpdError, match='CUDA'):                              # the launch needs the device; there is no CPU path
        clip.clip()
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            GradClipper(model, bad)
    with pytest.raises(FpdError, match='HIP-backed'):
        GradClipper(torch.nn.Linear(2, 2), 1.0)
