"""JointsOHKMMSELoss without a GPU: the CPU restatement against the reference's own class (tests/golden/ohkm_small.npz, written by
tests/golden/make_golden_ohkm.py), the public class, the C ABI of fpd_loss_ohkm (struct size, argument validation, plan op), the
criterion check of core.function and the criterion tools/fpd_train.py builds from LOSS.USE_OHKM / LOSS.TOPK."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _ohkm_ref
from tests.conftest import ROOT

GOLD = os.path.join(ROOT, 'tests', 'golden', 'ohkm_small.npz')
CASES = [('j16', 1, 8), ('j16', 0, 8), ('j17', 1, 1), ('j17', 1, 17), ('j17', 0, 1), ('j17', 0, 17)]


@pytest.fixture(scope='module')
def runtime():
    from fpd_amd import runtime as R
    if not os.path.exists(R.LIB_PATH):
        subprocess.check_call(['bash', os.path.join(os.path.dirname(R.LIB_PATH), 'build.sh')])
    R.lib()
    return R


@pytest.mark.parametrize('name,use_w,k', CASES)
def test_ohkm_ref_reproduces_the_reference_class(name, use_w, k):
    g = np.load(GOLD)
    out, tg, wt = g[name + '/output'], g[name + '/target'], g[name + '/weight'][:, :, 0]
    r = _ohkm_ref.criterion(out, tg, wt if use_w else np.ones_like(wt), k)
    key = '%s/w%d/k%d' % (name, use_w, k)
    assert abs(r['loss'] - float(g[key + '/loss'])) <= 1e-12 * max(1.0, abs(float(g[key + '/loss'])))
    assert np.abs(r['grad'] - g[key + '/grad']).max() <= 1e-12
    assert (r['sel'].sum(1) == k).all() and ((g[key + '/grad'] != 0).any((2, 3)) <= r['sel']).all()
    if use_w:
        assert (wt == 0).any()                                   # the fixture has zero weights


def test_ohkm_ref_tie_rule_and_topk_range():
    rows = np.array([[1.0, 3.0, 3.0, 0.5, 3.0]])
    assert _ohkm_ref.select(rows, 2).tolist() == [[False, True, True, False, False]]     # lower index wins among equals
    assert _ohkm_ref.mask_words(_ohkm_ref.select(rows, 4)).tolist() == [0b10111]
    for k in (0, 6):
        with pytest.raises(ValueError):
            _ohkm_ref.select(rows, k)


def test_class_imports_and_keeps_the_reference_constructor():
    from fpd_amd.lib.core.loss import JointsOHKMMSELoss
    sig = inspect.signature(JointsOHKMMSELoss.__init__)
    assert list(sig.parameters) == ['self', 'use_target_weight', 'topk'] and sig.parameters['topk'].default == 8
    c = JointsOHKMMSELoss(True)
    assert c.use_target_weight is True and c.topk == 8 and JointsOHKMMSELoss(False, topk=3).topk == 3
    assert list(inspect.signature(c.forward).parameters) == ['output', 'target', 'target_weight']
    import torch
    from fpd_amd import runtime as R
    with pytest.raises(R.FpdError):                              # CPU tensors: an error, not a fallback
        c(torch.zeros(1, 16, 4, 4), torch.zeros(1, 16, 4, 4), torch.ones(1, 16, 1))


def test_struct_size_matches(runtime):
    R = runtime
    assert R.lib().fpd_abi_sizeof(b'fpd_loss_ohkm_t') == ctypes.sizeof(R.LossOhkmT) > ctypes.sizeof(R.LossT)
    assert R.LossOhkmT.base.offset == 0 and R.OP_LOSS_OHKM == 24
    assert R.lib().fpd_abi_version() == 2


def _args(R, J=16, S=2, topk=(8, 8), dtype=0, scratch=True):
    k = R.LossOhkmT()
    a = k.base
    a.B, a.J, a.H, a.W, a.S, a.dtype, a.target_nchw, a.alpha, a.grad_scale = 2, J, 8, 8, S, dtype, 1, 0.5, 1.0
    a.teacher = a.target = a.weight = a.losses = 64             # never dereferenced: every call below fails validation
    for s in range(min(S, R.MAX_STACKS)):
        a.out[s] = 64
    k.topk_pose, k.topk_kd = topk
    if scratch:
        k.scratch, k.scratch_bytes = 64, 1 << 30
    return k


def test_validation_errors_without_device(runtime):
    R, lib = runtime, runtime.lib()
    err = lambda: lib.fpd_last_error().decode()
    assert lib.fpd_loss_ohkm(None, None) != 0 and 'null' in err()
    assert lib.fpd_loss_ohkm(R.LossOhkmT(), None) != 0 and 'null' in err()
    for topk in ((0, 8), (17, 8), (8, 0), (8, 17), (-1, 8)):
        assert lib.fpd_loss_ohkm(_args(R, topk=topk), None) != 0 and 'topk' in err(), topk
    assert lib.fpd_loss_ohkm(_args(R, J=33, topk=(8, 8)), None) != 0 and 'J=33' in err()
    assert lib.fpd_loss_ohkm(_args(R, S=R.MAX_STACKS + 1), None) != 0 and 'S=%d' % (R.MAX_STACKS + 1) in err()
    assert lib.fpd_loss_ohkm(_args(R, S=0), None) != 0 and 'S=0' in err()
    assert lib.fpd_loss_ohkm(_args(R, dtype=7), None) != 0 and 'dtype' in err()
    assert lib.fpd_loss_ohkm(_args(R, scratch=False), None) != 0 and 'scratch' in err()
    k = _args(R)
    need = lib.fpd_loss_ohkm_scratch_bytes(k.base)
    assert need == 2 * 1 * 2 * 2 * 16 * 8                        # double [B][chunks = 1][S][2][J]
    k.scratch_bytes = need - 1
    assert lib.fpd_loss_ohkm(k, None) != 0 and 'scratch' in err() and str(need) in err()
    k.scratch, k.scratch_bytes = 68, need                        # misaligned
    assert lib.fpd_loss_ohkm(k, None) != 0 and 'aligned' in err()
    big = _args(R).base
    big.B, big.H, big.W = 32, 64, 64                             # the benchmark's maps: 32 tiles per image in 16 chunks of 2
    assert lib.fpd_loss_ohkm_scratch_bytes(big) == 32 * 16 * 2 * 2 * 16 * 8
    assert lib.fpd_loss_ohkm_scratch_bytes(_args(R, J=33).base) < 0 and lib.fpd_loss_ohkm_scratch_bytes(None) < 0
    # fpd_loss asks the same of its fpd_loss_t, before any launch
    assert lib.fpd_loss(None, None) != 0 and 'null' in err()
    assert lib.fpd_loss(_args(R, J=33).base, None) == -3 and 'loss: J=33 (<=32)' in err()
    a = _args(R).base
    a.out[1] = None
    assert lib.fpd_loss(a, None) == -2 and 'loss: null map of stack 1' in err()
    assert lib.fpd_loss(_args(R, dtype=7).base, None) == -2 and 'loss: bad dtype 7' in err()
    big = _args(R).base
    big.B, big.H, big.W = 2048, 256, 256                         # 2^31 elements
    assert lib.fpd_loss(big, None) == -2 and 'loss: tensor too large for 32-bit indexing' in err()


def test_plan_accepts_the_op_and_checks_its_args_size(runtime):
    R, lib = runtime, runtime.lib()
    k = _args(R)
    p = ctypes.c_void_p(lib.fpd_plan_create())
    assert lib.fpd_plan_add(p, R.OP_LOSS_OHKM, ctypes.byref(k), ctypes.sizeof(k)) == 0
    assert lib.fpd_plan_add(p, R.OP_LOSS_OHKM, ctypes.byref(k.base), ctypes.sizeof(k.base)) < 0 and b'expects' in lib.fpd_last_error()
    assert lib.fpd_plan_add(p, R.OP_LOSS, ctypes.byref(k), ctypes.sizeof(k)) < 0
    assert lib.fpd_plan_size(p) == 1
    lib.fpd_plan_destroy(p)


def test_check_supported_returns_the_topk_pair_and_still_refuses_other_criteria(runtime):
    import torch
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss, JointsOHKMMSELoss
    from fpd_amd.lib.utils.utils import FusedAdam
    opt = object.__new__(FusedAdam)                             # the check looks at the type only
    mse, mse0, hard = JointsMSELoss(True), JointsMSELoss(False), JointsOHKMMSELoss(False, topk=5)
    assert F._check_supported(opt, mse, mse0) == ((True, False), None)
    assert F._check_supported(opt, hard, mse) == ((False, True), (5, None))
    assert F._check_supported(opt, mse, hard) == ((True, False), (None, 5))
    assert F._check_supported(opt, hard, JointsOHKMMSELoss(True)) == ((False, True), (5, 8))
    with pytest.raises(runtime.FpdError):
        F._check_supported(opt, torch.nn.MSELoss(), mse)
    with pytest.raises(runtime.FpdError):
        F._check_supported(opt, hard, torch.nn.MSELoss())
    with pytest.raises(runtime.FpdError):
        F._check_supported(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), hard, hard)


def test_fpd_train_tool_builds_the_criterion_from_use_ohkm_and_topk(monkeypatch):
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', os.environ.get('GPU_MAX_HW_QUEUES', '4'))     # importing the tool must not change it
    monkeypatch.syspath_prepend(os.path.join(ROOT, 'tools'))
    import fpd_train
    from fpd_amd.lib.config import cfg
    from fpd_amd.lib.core.loss import JointsMSELoss, JointsOHKMMSELoss
    c = cfg.clone()
    assert c.LOSS.USE_OHKM is False and c.LOSS.TOPK == 8       # every yaml of the reference: nothing changes
    crit = fpd_train.make_criterion(c)
    assert type(crit) is JointsMSELoss and crit.use_target_weight is True
    c.defrost()
    c.LOSS.USE_OHKM, c.LOSS.TOPK, c.LOSS.USE_TARGET_WEIGHT = True, 5, False
    crit = fpd_train.make_criterion(c)
    assert type(crit) is JointsOHKMMSELoss and crit.topk == 5 and crit.use_target_weight is False
    src = open(os.path.join(ROOT, 'tools', 'fpd_train.py')).read()
    assert 'pose_criterion = make_criterion(cfg)' in src and 'kd_pose_criterion = make_criterion(tcfg)' in src
