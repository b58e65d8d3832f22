"""JointsKLDLoss without a GPU: the closed-form CPU restatement tests/_kl_ref.py against torch's F.kl_div composition and its
autograd (float64), the public class, the C ABI of fpd_loss_kl (struct size, argument validation, plan op), the criterion check
of core.function, the config keys KD.LOSS / KD.TEMPERATURE and the criterion tools/fpd_train.py builds from them."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import _kl_ref
from tests.conftest import ROOT


@pytest.fixture(scope='module')
def runtime():
    from fpd_amd import runtime as R
    if not os.path.exists(R.LIB_PATH):
        subprocess.check_call(['bash', os.path.join(os.path.dirname(R.LIB_PATH), 'build.sh')])
    R.lib()
    return R


def _inputs(seed, B=3, J=5, H=6, W=7, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    s = (torch.randn(B, J, H, W, generator=gen, dtype=torch.float64) * scale).numpy()
    r = (torch.randn(B, J, H, W, generator=gen, dtype=torch.float64) * scale).numpy()
    w = torch.rand(B, J, generator=gen, dtype=torch.float64) * 1.5
    w[0, 1], w[1, 0], w[2, 3] = 0.0, 1.5, 1.0                    # zero and non-unit weights
    return s, r, w.numpy()


@pytest.mark.parametrize('T', [0.05, 0.5, 1.0, 4.0])
@pytest.mark.parametrize('seed', [1, 2])
def test_closed_form_matches_the_kl_div_composition_and_its_autograd(seed, T):
    s, r, w = _inputs(seed)
    ref = _kl_ref.criterion(s, r, w, T)
    loss, grad = _kl_ref.torch_composition(s, r, w, T, torch.float64)
    assert abs(ref['loss'] - loss) <= 1e-12 * max(1.0, abs(loss)), (ref['loss'], loss)
    assert np.abs(ref['grad'] - grad).max() <= 1e-12
    assert (ref['rows'] >= -1e-15).all() and ref['loss'] > 0    # a KL divergence
    assert (ref['grad'][0, 1] == 0).all()                        # a zero weight carries no gradient


def test_the_weight_enters_once_and_the_temperature_scales_as_defined():
    s, r, w = _inputs(3)
    one = _kl_ref.criterion(s, r, np.ones_like(w), 1.0)
    got = _kl_ref.criterion(s, r, w, 1.0)
    assert abs(got['loss'] - (w * one['rows']).sum() / w.size) < 1e-15
    assert np.allclose(got['grad'], w[:, :, None, None] * one['grad'], rtol=1e-14, atol=0)
    # q == 0 exactly: a one-hot reference row gives -w T^2 log p at that pixel; nothing is NaN
    T = 0.05
    r1 = np.full_like(r, -1e4)
    r1[:, :, 2, 3] = 0.0
    hot = _kl_ref.criterion(s, r1, w, T)
    B, J, H, W = s.shape
    y = s.reshape(B, J, -1) / T
    logp = y[:, :, 2 * W + 3] - (y.max(2) + np.log(np.exp(y - y.max(2, keepdims=True)).sum(2)))
    assert np.isfinite(hot['grad']).all() and np.allclose(hot['rows'], -T * T * logp, rtol=1e-13, atol=0)
    # equal maps: exactly zero
    same = _kl_ref.criterion(s, s, w, 0.3)
    assert same['loss'] == 0.0 and (same['grad'] == 0).all()
    # +-100 at T = 0.05 stays finite
    big = _kl_ref.criterion(np.sign(s) * 100.0, np.sign(r) * 100.0, w, 0.05)
    assert np.isfinite(big['loss']) and np.isfinite(big['grad']).all()
    with pytest.raises(ValueError):
        _kl_ref.criterion(s, r, w, 0.0)


def test_fused_restatement_adds_the_terms_of_every_stack():
    s, r, w = _inputs(4)
    s2, tg, wk = _inputs(5)
    f = _kl_ref.fused([s, s2], tg, r, w, wk, None, 0.5, 0.25, grad_scale=0.5)
    a0, a1 = _kl_ref.mse(s, tg, w), _kl_ref.mse(s2, tg, w)
    b0, b1 = _kl_ref.criterion(s, r, wk, 0.5), _kl_ref.criterion(s2, r, wk, 0.5)
    assert f['pose'] == a0['loss'] + a1['loss'] and f['kd'] == b0['loss'] + b1['loss']
    assert np.array_equal(f['grads'][1], 0.5 * (0.75 * a1['grad'] + 0.25 * b1['grad']))


def test_class_constructor_and_cpu_tensors_are_refused():
    from fpd_amd import runtime as R
    from fpd_amd.lib.core.loss import JointsKLDLoss
    sig = inspect.signature(JointsKLDLoss.__init__)
    assert list(sig.parameters) == ['self', 'use_target_weight', 'temperature'] and sig.parameters['temperature'].default == 1.0
    c = JointsKLDLoss(True)
    assert c.use_target_weight is True and c.temperature == 1.0 and JointsKLDLoss(False, temperature=0.05).temperature == 0.05
    assert list(inspect.signature(c.forward).parameters) == ['output', 'target', 'target_weight']
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            JointsKLDLoss(True, bad)
    with pytest.raises(R.FpdError):                              # CPU tensors: an error, not a fallback
        c(torch.zeros(1, 16, 4, 4), torch.zeros(1, 16, 4, 4), torch.ones(1, 16, 1))


def test_struct_size_matches_the_header(runtime):
    R = runtime
    assert R.lib().fpd_abi_sizeof(b'fpd_loss_kl_t') == ctypes.sizeof(R.LossKlT) == ctypes.sizeof(R.LossT) + 32
    assert R.LossKlT.base.offset == 0 and R.OP_LOSS_KL == 27 and R.OP_EW_MERGE == 26 and R.OP_LOSS_OHKM == 24
    assert R.lib().fpd_abi_version() == 2                        # additions only
    assert R._STRUCTS['fpd_loss_kl_t'] is R.LossKlT
    hdr = open(os.path.join(ROOT, 'include', 'fpd_amd.h')).read()
    assert 'FPD_OP_LOSS_KL = 27' in hdr and 'int fpd_loss_kl(const fpd_loss_kl_t*' in hdr
    assert 'int64_t fpd_loss_kl_scratch_bytes(const fpd_loss_t*' in hdr


def _args(R, J=16, S=2, kl=(0, 1), temps=(1.0, 1.0), dtype=0, scratch=True):
    k = R.LossKlT()
    a = k.base
    a.B, a.J, a.H, a.W, a.S, a.dtype, a.target_nchw, a.alpha, a.grad_scale = 2, J, 8, 8, S, dtype, 1, 0.5, 1.0
    a.teacher = a.target = a.weight = a.losses = 64             # never dereferenced: every call below fails validation
    for s in range(min(S, R.MAX_STACKS)):
        a.out[s] = 64
    k.kl_pose, k.kl_kd = kl
    k.temp_pose, k.temp_kd = temps
    if scratch:
        k.scratch, k.scratch_bytes = 64, 1 << 30
    return k


def test_validation_errors_without_device(runtime):
    R, lib = runtime, runtime.lib()
    err = lambda: lib.fpd_last_error().decode()
    assert lib.fpd_loss_kl(None, None) != 0 and 'null' in err()
    assert lib.fpd_loss_kl(R.LossKlT(), None) != 0 and 'null' in err()
    assert lib.fpd_loss_kl(_args(R, kl=(0, 0)), None) != 0 and 'neither' in err()
    for kl, temps in (((0, 1), (1.0, 0.0)), ((0, 1), (1.0, -1.0)), ((1, 0), (0.0, 1.0)), ((1, 1), (1.0, 0.0)),
                      ((0, 1), (1.0, float('nan'))), ((0, 1), (1.0, float('inf')))):
        assert lib.fpd_loss_kl(_args(R, kl=kl, temps=temps), None) != 0 and 'temperature' in err(), (kl, temps)
    assert lib.fpd_loss_kl(_args(R, J=33), None) != 0 and 'J=33' in err()
    assert lib.fpd_loss_kl(_args(R, S=R.MAX_STACKS + 1), None) != 0 and 'S=%d' % (R.MAX_STACKS + 1) in err()
    assert lib.fpd_loss_kl(_args(R, S=0), None) != 0 and 'S=0' in err()
    assert lib.fpd_loss_kl(_args(R, dtype=7), None) != 0 and 'dtype' in err()
    assert lib.fpd_loss_kl(_args(R, scratch=False), None) != 0 and 'scratch' in err()
    k = _args(R)
    need = lib.fpd_loss_kl_scratch_bytes(k.base)
    assert need == 2 * 1 * ((3 * 2 + 4) * 16 + 2) * 8            # double [B][chunks = 1][M: S + 2 rows, Z: 2 S + 2 rows, of J; 2 MSE sums]
    k.scratch_bytes = need - 1
    assert lib.fpd_loss_kl(k, None) != 0 and 'scratch' in err() and str(need) in err()
    k.scratch, k.scratch_bytes = 68, need                        # misaligned
    assert lib.fpd_loss_kl(k, None) != 0 and 'aligned' in err()
    big = _args(R).base
    big.B, big.H, big.W = 32, 64, 64                             # the benchmark's maps: 32 tiles per image in 16 chunks of 2
    assert lib.fpd_loss_kl_scratch_bytes(big) == 32 * 16 * ((3 * 2 + 4) * 16 + 2) * 8
    assert lib.fpd_loss_kl_scratch_bytes(_args(R, J=33).base) < 0 and lib.fpd_loss_kl_scratch_bytes(None) < 0


def test_plan_accepts_the_op_and_checks_its_args_size(runtime):
    R, lib = runtime, runtime.lib()
    k = _args(R)
    p = ctypes.c_void_p(lib.fpd_plan_create())
    assert lib.fpd_plan_add(p, R.OP_LOSS_KL, ctypes.byref(k), ctypes.sizeof(k)) == 0
    assert lib.fpd_plan_add(p, R.OP_LOSS_KL, ctypes.byref(k.base), ctypes.sizeof(k.base)) < 0 and b'expects' in lib.fpd_last_error()
    assert lib.fpd_plan_add(p, R.OP_LOSS, ctypes.byref(k), ctypes.sizeof(k)) < 0
    assert lib.fpd_plan_size(p) == 1
    lib.fpd_plan_destroy(p)


def test_check_supported_returns_the_temperature_pair_and_refuses_kl_with_ohkm(runtime):
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsKLDLoss, JointsMSELoss, JointsOHKMMSELoss
    from fpd_amd.lib.utils.utils import FusedAdam
    opt = object.__new__(FusedAdam)                             # the check looks at the type only
    mse, kl, kl0, hard = JointsMSELoss(True), JointsKLDLoss(True, 0.5), JointsKLDLoss(False), JointsOHKMMSELoss(True, topk=5)
    assert F._check_supported(opt, mse, mse) == ((True, True), None)                 # as before
    assert F._check_supported(opt, mse, kl) == ((True, True), None, (None, 0.5))
    assert F._check_supported(opt, kl0, mse) == ((False, True), None, (1.0, None))
    assert F._check_supported(opt, kl, kl0) == ((True, False), None, (0.5, 1.0))
    for pair in ((hard, kl), (kl, hard)):
        with pytest.raises(runtime.FpdError, match='JointsOHKMMSELoss'):
            F._check_supported(opt, *pair)
    for pair in ((torch.nn.KLDivLoss(), kl), (kl, torch.nn.KLDivLoss()), (mse, object())):
        with pytest.raises(runtime.FpdError):
            F._check_supported(opt, *pair)
    with pytest.raises(runtime.FpdError):
        F._check_supported(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), mse, kl)
    assert 'kl' in inspect.signature(F.fused_step_for).parameters


def test_config_defaults_and_the_criterion_the_tool_builds(monkeypatch):
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', os.environ.get('GPU_MAX_HW_QUEUES', '4'))     # importing the tool must not change it
    monkeypatch.syspath_prepend(os.path.join(ROOT, 'tools'))
    import fpd_train
    from fpd_amd.lib.config import cfg
    from fpd_amd.lib.core.loss import JointsKLDLoss, JointsMSELoss, JointsOHKMMSELoss
    c, tc = cfg.clone(), cfg.clone()
    assert c.KD.LOSS == 'mse' and c.KD.TEMPERATURE == 1.0       # every yaml of the reference: nothing changes
    assert c.KD.ALPHA == 0.5 and c.KD.TRAIN_TYPE == 'NORMAL'
    crit = fpd_train.make_kd_criterion(c, tc)
    assert type(crit) is JointsMSELoss and crit.use_target_weight is True
    tc.defrost()
    tc.LOSS.USE_OHKM = True
    assert type(fpd_train.make_kd_criterion(c, tc)) is JointsOHKMMSELoss      # 'mse': the teacher config decides, as before
    c.defrost()
    c.KD.LOSS, c.KD.TEMPERATURE = 'kl', 0.05
    with pytest.raises(SystemExit, match='USE_OHKM'):
        fpd_train.make_kd_criterion(c, tc)
    tc.LOSS.USE_OHKM, tc.LOSS.USE_TARGET_WEIGHT = False, False
    crit = fpd_train.make_kd_criterion(c, tc)
    assert type(crit) is JointsKLDLoss and crit.temperature == 0.05 and crit.use_target_weight is False
    assert type(fpd_train.make_criterion(c)) is JointsMSELoss   # the pose criterion is chosen as before
    c.LOSS.USE_OHKM = True                                       # ... and a mining pose criterion cannot be paired with it either
    with pytest.raises(SystemExit, match='USE_OHKM'):
        fpd_train.make_kd_criterion(c, tc)
    c.LOSS.USE_OHKM, c.KD.TEMPERATURE = False, 0.0
    with pytest.raises(SystemExit, match='TEMPERATURE'):
        fpd_train.make_kd_criterion(c, tc)
    c.KD.TEMPERATURE, c.KD.LOSS = 1.0, 'huber'
    with pytest.raises(SystemExit, match='KD.LOSS'):
        fpd_train.make_kd_criterion(c, tc)


def test_fused_step_argument_checks_come_before_any_device_work():
    from fpd_amd import executor as E
    from fpd_amd import runtime as R

    class _State:                                                # the checks run before the state is touched beyond these two
        device, dtype = 'cpu', 0
    for kw in ({'kl': (None, 1.0), 'ohkm': (8, None)}, {'kl': (None, 0.0)}, {'kl': (-1.0, None)}, {'kl': (None, None)}):
        with pytest.raises(R.FpdError):
            E.FusedFPDStep(_State(), {'J': 16}, None, None, 2, 64, 64, 0.5, **kw)
