"""The weight average (utils.ModelEma / fpd_ema), the parts that need no GPU: a HOST build of the kernel's arithmetic
(csrc/ema_math.h) against the numpy restatement (tests/_ema_ref.py) bit for bit and under the host sanitizers as a
stand-alone program, the config keys, the ABI surface and refusals of fpd_ema, and ModelEma's state on CPU tensors."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _ema_ref as E
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'fast-human-pose-estimation.pytorch_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'native', 'ema_host.cpp')


def _cxx():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler for the host build of csrc/ema_math.h')
    return cxx


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('ema') / 'libema_host.so')
    subprocess.check_call([_cxx(), '-O2', '-ffp-contract=off', '-Wno-unknown-pragmas', '-shared', '-fPIC', '-I' + CSRC, SRC, '-o', so])
    lib = C.CDLL(so)
    lib.ema_weight_host.restype = C.c_float
    lib.ema_weight_host.argtypes = [C.c_int64, C.c_double, C.c_int]
    lib.ema_update_host.restype = C.c_float
    lib.ema_update_host.argtypes = [C.c_float, C.c_float, C.c_float]
    lib.ema_update_array_host.restype = None
    lib.ema_update_array_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_float]
    return lib


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- the host build of csrc/ema_math.h ----

@pytest.mark.parametrize('warmup', [False, True])
@pytest.mark.parametrize('decay', E.DECAYS)
def test_host_build_of_the_weight_schedule_is_numpys_bit_for_bit(host_lib, decay, warmup):
    for u in E.UPDATES:
        got, want = np.float32(host_lib.ema_weight_host(u, decay, int(warmup))), E.weight(u, decay, warmup)
        assert _bits(got) == _bits(want), (u, decay, warmup, float(got), float(want))
        if not warmup:
            assert want == np.float32(1.0 - decay)
    if warmup and decay == 0.9998:
        # both sides of the crossing: the ramp rules up to 44 988 updates done, the decay from 44 990 on
        w = [E.weight(u, decay, True) for u in (44979, 44988, 44990, 44999, 49990)]
        assert w[0] > w[1] > w[2] == w[3] == w[4] == np.float32(1.0 - 0.9998)
        assert E.weight(0, decay, True) == np.float32(1.0 - 2.0 / 11.0)


def test_host_build_of_the_update_is_numpys_bit_for_bit_and_unfused(host_lib):
    # the designed triple first: the two restatements differ on it, so agreement with the unfused one shows contraction is off
    e, x, w = E.DESIGNED
    unfused, fused = E.update(e, x, w), E.update_fused(e, x, w)
    assert _bits(unfused) != _bits(fused) and unfused == E.DESIGNED_UNFUSED and fused == E.DESIGNED_FUSED
    assert _bits(np.float32(host_lib.ema_update_host(e, x, w))) == _bits(unfused)
    for w in (E.weight(0, 0.9998, True), E.weight(10 ** 7, 0.9998, True), E.weight(3, 0.5, False), np.float32(1.0), E.DESIGNED[2]):
        for e0, x0 in (E.seeded(4099), E.special_values()):
            want = E.update(e0, x0, w)
            got = e0.copy()
            host_lib.ema_update_array_host(got.ctypes.data, x0.ctypes.data, got.size, w)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan)                       # NaN stays NaN (its payload is not compared)
            assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), float(w)
    e0, x0 = E.special_values()
    assert np.isnan(E.update(e0, x0, np.float32(0.25))[np.isnan(e0) | np.isnan(x0)]).all()


def test_the_header_walks_its_cases_clean_under_the_host_sanitizers(tmp_path):
    """The same text with a small main, built with -fsanitize=address,undefined and run as a program of its own."""
    exe = str(tmp_path / 'ema_san')
    subprocess.check_call([_cxx(), '-O1', '-g', '-ffp-contract=off', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DEMA_MAIN', '-I' + CSRC, SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b'cases ok' in r.stdout, r.stdout.decode()


# ---- config ----

REFERENCE_STYLE_YAML = '''AUTO_RESUME: true
GPUS: (0,)
OUTPUT_DIR: 'output'
LOG_DIR: 'log'
WORKERS: 12
PRINT_FREQ: 100
DATASET:
  DATASET: mpii
  ROOT: 'data/mpii/'
  TEST_SET: valid
  TRAIN_SET: train
MODEL:
  NAME: hourglass
  NUM_JOINTS: 16
  IMAGE_SIZE: [256, 256]
  HEATMAP_SIZE: [64, 64]
  SIGMA: 2
  EXTRA:
    NUM_FEATURES: 128
    NUM_STACKS: 4
    NUM_BLOCKS: 1
LOSS:
  USE_TARGET_WEIGHT: true
TRAIN:
  BATCH_SIZE_PER_GPU: 4
  SHUFFLE: true
  BEGIN_EPOCH: 0
  END_EPOCH: 150
  OPTIMIZER: adam
  LR: 0.00025
  LR_FACTOR: 0.1
  LR_STEP: [90, 120]
  WD: 0.0001
  GAMMA1: 0.99
  GAMMA2: 0.0
  MOMENTUM: 0.9
  NESTEROV: false
TEST:
  BATCH_SIZE_PER_GPU: 32
  MODEL_FILE: ''
  FLIP_TEST: true
  POST_PROCESS: true
  SHIFT_HEATMAP: true
KD:
  TRAIN_TYPE: FPD
  TEACHER: 'models/teacher.pth'
  ALPHA: 0.5
'''


def test_config_has_the_four_keys_off_by_default_and_a_reference_yaml_still_loads(tmp_path):
    from fpd_amd.lib.config import _defaults
    cfg = _defaults()
    assert cfg.TRAIN.EMA is False and cfg.TRAIN.EMA_DECAY == 0.9998 and cfg.TRAIN.EMA_WARMUP is True and cfg.TEST.USE_EMA is False
    y = tmp_path / 'reference.yaml'
    y.write_text(REFERENCE_STYLE_YAML)
    cfg.merge_from_file(str(y))
    assert cfg.TRAIN.EMA is False and cfg.TRAIN.EMA_DECAY == 0.9998 and cfg.TRAIN.EMA_WARMUP is True and cfg.TEST.USE_EMA is False
    assert cfg.TRAIN.END_EPOCH == 150 and cfg.TEST.FLIP_TEST is True
    cfg.merge_from_list(['TRAIN.EMA', 'True', 'TRAIN.EMA_DECAY', '0.999', 'TRAIN.EMA_WARMUP', 'False', 'TEST.USE_EMA', 'True'])
    assert cfg.TRAIN.EMA is True and cfg.TRAIN.EMA_DECAY == 0.999 and cfg.TRAIN.EMA_WARMUP is False and cfg.TEST.USE_EMA is True
    shipped = _defaults()
    shipped.merge_from_file(os.path.join(ROOT, 'experiments', 'fpd_synthetic', 'hg4x128_student_ema.yaml'))
    assert shipped.TRAIN.EMA is True and shipped.TRAIN.EMA_DECAY == 0.9998 and shipped.TEST.USE_EMA is False


# ---- the C ABI ----

@pytest.fixture(scope='module')
def runtime():
    from fpd_amd import runtime as R
    if not os.path.exists(R.LIB_PATH):
        subprocess.check_call(['bash', os.path.join(os.path.dirname(R.LIB_PATH), 'build.sh')])
    R.lib()
    return R


def _args(R):
    a = R.EmaT()
    a.nseg, a.warmup, a.decay = 2, 1, 0.9998
    a.seg[0].src, a.seg[0].dst, a.seg[0].n = 0x10000, 0x20000, 4099        # never dereferenced: the query launches nothing,
    a.seg[1].src, a.seg[1].dst, a.seg[1].n = 0x30000, 0x40004, 1000        # and every fpd_ema call below is refused first
    a.copy_src, a.copy_dst, a.copy_n = 0x50000, 0x60000, 7
    a.updates_dev = 0x70000
    return a


def test_abi_has_fpd_ema_with_the_mirrors_size_and_the_geometry_query_is_pure_host_code(runtime):
    R, lib = runtime, runtime.lib()
    assert lib.fpd_abi_sizeof(b'fpd_ema_t') == C.sizeof(R.EmaT) == 4 * 24 + 8 + 8 + 24 + 8
    assert lib.fpd_abi_version() == R.ABI_VERSION == 2 and R.OP_EMA == 28 and R.EMA_MAX_SEG == 4
    blocks, vec = C.c_int32(-1), (C.c_int64 * 4)(-1, -1, -1, -1)
    assert lib.fpd_ema_geometry(_args(R), blocks, vec) == 0
    # the grid covers the longest loop of the launch: 1024 vectors and 3 single elements of segment 0, 1000 single elements of
    # segment 1 (its dst is 4 bytes off a 16-byte boundary), 7 copied integers; entries past nseg are not written
    assert blocks.value == 4 and list(vec) == [4096, 0, -1, -1]
    a = _args(R)
    a.seg[0].n = 4 * 256 * 3 + 1
    lib.fpd_ema_geometry(a, blocks, vec)
    assert blocks.value == 4 and vec[0] == 4 * 256 * 3                     # 1000 single elements of segment 1 need 4 blocks
    a.seg[0].src, a.seg[0].dst, a.seg[0].n = 1 << 44, 1 << 45, 1 << 32    # the cap of the other flat launches
    assert lib.fpd_ema_geometry(a, blocks, vec) == 0 and blocks.value == 4096 and vec[0] == 1 << 32
    p = lib.fpd_plan_create()
    assert lib.fpd_plan_add(p, R.OP_EMA, C.byref(_args(R)), C.sizeof(R.EmaT)) == 0
    assert lib.fpd_plan_add(p, R.OP_EMA, C.byref(_args(R)), C.sizeof(R.EmaT) - 8) < 0
    lib.fpd_plan_destroy(p)


def refusals(R):
    """(label, mutated arguments, word of the message): every case fpd_ema refuses before it launches."""
    out = []

    def case(label, word, **kw):
        a = _args(R)
        for k, v in kw.items():
            if k.startswith('seg'):
                setattr(a.seg[int(k[3])], k[5:], v)
            else:
                setattr(a, k, v)
        out.append((label, a, word))
    case('nseg 0', b'nseg', nseg=0)
    case('nseg 5', b'nseg', nseg=5)
    case('negative n', b'negative', seg1_n=-1)
    case('negative copy_n', b'negative', copy_n=-2)
    case('null src', b'null', seg0_src=None)
    case('null dst', b'null', seg1_dst=None)
    case('null copy_src', b'null', copy_src=None)
    case('null copy_dst', b'null', copy_dst=None)
    case('null counter', b'null', updates_dev=None)
    case('decay 1', b'decay', decay=1.0)
    case('decay < 0', b'decay', decay=-0.1)
    case('decay nan', b'decay', decay=float('nan'))
    case('src == dst', b'overlaps', seg0_dst=0x10000)
    case('dst inside its src', b'overlaps', seg0_dst=0x10000 + 4 * 4098)
    case('dst over the other src', b'overlaps', seg0_dst=0x30000 - 4 * 4098)
    case('dst over the other dst', b'overlaps', seg1_dst=0x20000 + 4 * 4098)
    case('counter inside a dst', b'overlaps', updates_dev=0x20008)
    case('copy_dst over a src', b'overlaps', copy_dst=0x10000)
    return out


def test_fpd_ema_refuses_bad_arguments_without_a_device(runtime):
    R, lib = runtime, runtime.lib()
    assert lib.fpd_ema(None, None) < 0 and b'null' in lib.fpd_last_error()
    blocks, vec = C.c_int32(), (C.c_int64 * 4)()
    for label, a, word in refusals(R):
        assert lib.fpd_ema(a, None) < 0 and word in lib.fpd_last_error(), (label, lib.fpd_last_error())
        assert lib.fpd_ema_geometry(a, blocks, vec) < 0 and word in lib.fpd_last_error(), label
    a = _args(R)                      # n = 0 with null pointers is an empty segment, adjacent ranges do not overlap
    a.seg[1].src, a.seg[1].dst, a.seg[1].n = None, None, 0
    a.seg[0].dst = 0x10000 + 4 * 4099
    a.copy_src = a.copy_dst = None
    a.copy_n = 0
    assert lib.fpd_ema_geometry(a, blocks, vec) == 0 and vec[0] == 0      # (dst 4 bytes off a 16-byte boundary)


# ---- ModelEma on CPU tensors ----

class AD(dict):
    __getattr__ = dict.__getitem__


def _model(seed=0):
    import torch
    from fpd_amd.lib.models import hourglass
    torch.manual_seed(seed)
    return hourglass.get_pose_net(AD(MODEL=AD(NUM_JOINTS=3, DTYPE='fp32', EXTRA=AD(NUM_FEATURES=16, NUM_STACKS=2, NUM_BLOCKS=1))), is_train=True)


def test_model_ema_state_round_trips_and_its_module_mirrors_the_model_on_the_cpu():
    import torch
    from fpd_amd.lib.utils.utils import ModelEma
    from fpd_amd.runtime import FpdError
    model = _model()
    state = torch.random.get_rng_state()
    ema = ModelEma(model, decay=0.99, warmup=False)
    assert torch.equal(torch.random.get_rng_state(), state)               # the second instance drew nothing from the run's generator
    sd, msd = ema.state_dict(), model.state_dict()
    assert sorted(sd) == ['decay', 'state_dict', 'updates', 'warmup'] and (sd['updates'], sd['decay'], sd['warmup']) == (0, 0.99, False)
    assert list(sd['state_dict']) == list(msd) == list(ema.module.state_dict())
    assert all(sd['state_dict'][k].shape == v.shape and torch.equal(sd['state_dict'][k], v) for k, v in msd.items())
    assert msd['conv1.weight'].shape == (4, 3, 7, 7)                       # OIHW
    assert type(ema.module).__name__ == 'EmaHourglassNet' and isinstance(ema.module, type(model)) and not ema.module.training
    assert ema.module._flat['param'].data_ptr() == ema.flat['param'].data_ptr() != model._flat['param'].data_ptr()
    assert ema.module.conv1.weight.data_ptr() - ema.flat['param'].data_ptr() == model.conv1.weight.data_ptr() - model._flat['param'].data_ptr()
    with pytest.raises(FpdError, match='eval'):
        ema.module.train()
    ema.module.eval()
    with pytest.raises(FpdError, match='CUDA'):
        ema.update()
    # the average is its own storage: the model moves, the average stays; set() follows and zeroes the counter
    with torch.no_grad():
        model._flat['param'].add_(1.0)
    assert torch.equal(ema.state_dict()['state_dict']['conv1.weight'], sd['state_dict']['conv1.weight'])
    # round trip into a second average of another model
    other = ModelEma(_model(seed=1), decay=0.5, warmup=True)
    assert not torch.equal(other.module.conv1.weight, ema.module.conv1.weight)
    sd['updates'] = 17
    other.load_state_dict(sd)
    back = other.state_dict()
    assert (back['updates'], back['decay'], back['warmup']) == (17, 0.99, False) and int(other.updates_dev) == 17
    assert all(torch.equal(back['state_dict'][k], v) for k, v in sd['state_dict'].items())
    other.load_state_dict({'state_dict': {'module.' + k: v for k, v in sd['state_dict'].items()}, 'updates': 3})      # a DataParallel-style dict
    assert other.updates == 3 and other.decay == 0.99
    ema.updates_dev.fill_(5)
    ema.set(model)
    assert ema.updates == 0 and torch.equal(ema.flat['param'], model._flat['param']) and torch.equal(ema.module.conv1.weight, model.conv1.weight)
    a = ema.ema_args()
    assert a.nseg == 2 and a.seg[0].n == model.table.sizes['param'] and a.seg[1].n == model.table.sizes['rstat'] and a.copy_n == model.table.sizes['nbt']
    assert a.seg[0].src == model._flat['param'].data_ptr() and a.seg[0].dst == ema.flat['param'].data_ptr() and (a.decay, a.warmup) == (0.99, 0)
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError):
            ModelEma(model, decay=bad)
