"""Fused SGD without a GPU: the precondition of the bit-exact kernel test (float32 torch == float64 torch on the dyadic
trajectory), the C ABI of fpd_sgd (struct size, argument validation, plan op), the optimizer check of core.function,
FusedSGD's constructor and its checkpoint interop with torch.optim.SGD, utils.get_optimizer, and tools/train.py's wiring."""
import ctypes
import io
import os
import subprocess

import pytest
import torch

from tests import _sgd_ref
from tests.conftest import ROOT


class AD(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope='module')
def runtime():
    from fpd_amd import runtime as R
    if not os.path.exists(R.LIB_PATH):
        subprocess.check_call(['bash', os.path.join(os.path.dirname(R.LIB_PATH), 'build.sh')])
    R.lib()
    return R


@pytest.mark.parametrize('momentum,wd,nesterov', _sgd_ref.VARIANTS)
def test_dyadic_trajectory_is_exact_in_float32(momentum, wd, nesterov):
    """Three steps only: a fourth is no longer exact for Nesterov + weight decay."""
    p0, grads = _sgd_ref.dyadic_inputs(4099)
    assert p0.abs().max() == 2 and min(g.abs().max() for g in grads) == 1 and len(p0.unique()) == 33
    t32 = _sgd_ref.sgd_trajectory(p0, grads, _sgd_ref.LRS, momentum, wd, nesterov, torch.float32)
    t64 = _sgd_ref.sgd_trajectory(p0, grads, _sgd_ref.LRS, momentum, wd, nesterov, torch.float64)
    for k, ((p32, b32), (p64, b64)) in enumerate(zip(t32, t64)):
        assert p32.dtype == torch.float32 and torch.equal(p32.double(), p64), 'step %d' % (k + 1)
        assert (b32 is None) == (momentum == 0) and (b32 is None or torch.equal(b32.double(), b64))
    assert not torch.equal(t32[0][0], p0) and not torch.equal(t32[2][0], t32[1][0])


def test_struct_size_and_op_code(runtime):
    R = runtime
    assert R.lib().fpd_abi_sizeof(b'fpd_sgd_t') == ctypes.sizeof(R.SgdT) == 80
    assert R.OP_SGD == 25 == R.OP_LOSS_OHKM + 1 and R.OP_ADAM == 6
    assert R.lib().fpd_abi_version() == 2


def _args(R, **kw):
    a = R.SgdT()
    a.n, a.param, a.grad, a.buf = 16, 64, 128, 192           # never dereferenced: every call below fails validation
    a.lr, a.momentum, a.weight_decay, a.grad_scale = 0.1, 0.9, 1e-4, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_validation_errors_without_device(runtime):
    R, lib = runtime, runtime.lib()
    err = lambda: lib.fpd_last_error().decode()
    assert lib.fpd_sgd(None, None) != 0 and 'null' in err()
    assert lib.fpd_sgd(_args(R, param=None), None) != 0 and 'null' in err()
    assert lib.fpd_sgd(_args(R, grad=None), None) != 0 and 'null' in err()
    assert lib.fpd_sgd(_args(R, n=-1), None) != 0 and 'negative' in err()
    assert lib.fpd_sgd(_args(R, momentum=-0.5), None) != 0 and 'momentum' in err()
    assert lib.fpd_sgd(_args(R, momentum=float('nan')), None) != 0 and 'momentum' in err()
    assert lib.fpd_sgd(_args(R, weight_decay=-1e-4), None) != 0 and 'weight_decay' in err()
    assert lib.fpd_sgd(_args(R, buf=None), None) != 0 and 'buf' in err()
    assert lib.fpd_sgd(_args(R, momentum=0.0, nesterov=1), None) != 0 and 'nesterov' in err().lower()
    assert lib.fpd_sgd(_args(R, momentum=0.0, nesterov=1, buf=None), None) != 0 and 'nesterov' in err().lower()


def test_plan_accepts_the_op_and_checks_its_args_size(runtime):
    R, lib = runtime, runtime.lib()
    a, adam = _args(R), R.AdamT()
    p = ctypes.c_void_p(lib.fpd_plan_create())
    assert lib.fpd_plan_add(p, R.OP_SGD, ctypes.byref(a), ctypes.sizeof(a)) == 0
    assert lib.fpd_plan_add(p, R.OP_SGD, ctypes.byref(adam), ctypes.sizeof(adam)) < 0 and b'expects' in lib.fpd_last_error()
    assert lib.fpd_plan_add(p, R.OP_ADAM, ctypes.byref(a), ctypes.sizeof(a)) < 0
    assert lib.fpd_plan_size(p) == 1
    bad = _args(R, buf=None)                                     # the plan runs the op through fpd_sgd: refused before any launch
    assert lib.fpd_plan_add(p, R.OP_SGD, ctypes.byref(bad), ctypes.sizeof(bad)) == 1
    assert lib.fpd_plan_run_op(p, 1, None) != 0 and b'buf' in lib.fpd_last_error()
    lib.fpd_plan_destroy(p)


def test_check_supported_accepts_fused_sgd_and_still_refuses_torch_sgd(runtime):
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.utils.utils import FusedAdam, FusedSGD
    mse = JointsMSELoss(True)
    assert not issubclass(FusedSGD, FusedAdam) and not issubclass(FusedAdam, FusedSGD)      # fused_step_for tells them apart by type
    assert F._check_supported(object.__new__(FusedSGD), mse, mse) == ((True, True), None)  # the check looks at the type only
    assert F._check_supported(object.__new__(FusedAdam), mse, mse) == ((True, True), None)
    with pytest.raises(runtime.FpdError, match='FusedSGD'):
        F._check_supported(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1, momentum=0.9), mse, mse)
    with pytest.raises(runtime.FpdError, match='FusedAdam'):
        F._check_supported(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]), mse, mse)


def _model():
    from fpd_amd.lib.models import hourglass
    return hourglass.get_pose_net(AD(MODEL=AD(NUM_JOINTS=4, DTYPE='fp32', EXTRA=AD(NUM_FEATURES=32, NUM_STACKS=1, NUM_BLOCKS=1))),
                                  is_train=True)


def test_constructor_and_get_optimizer():
    from fpd_amd.lib.utils.utils import FusedSGD, get_optimizer
    m = _model()
    with pytest.raises(ValueError, match='Nesterov'):
        FusedSGD(m, lr=0.1, momentum=0, nesterov=True)
    with pytest.raises(ValueError, match='momentum'):
        FusedSGD(m, lr=0.1, momentum=-0.1)
    with pytest.raises(ValueError, match='weight_decay'):
        FusedSGD(m, lr=0.1, weight_decay=-0.1)
    plain = FusedSGD(m, lr=0.1)
    assert plain.buf is None                                     # no momentum: no buffer arena
    opt = get_optimizer(AD(TRAIN=AD(OPTIMIZER='sgd', LR=0.01, MOMENTUM=0.9, WD=1e-4, NESTEROV=True)), m)
    assert type(opt) is FusedSGD and isinstance(opt, torch.optim.Optimizer)
    g = opt.param_groups[0]
    assert (g['lr'], g['momentum'], g['weight_decay'], g['nesterov'], g['dampening'], g['maximize']) == (0.01, 0.9, 1e-4, True, 0, False)
    flat = m._flat['param']
    assert opt.buf.shape == flat.shape and opt.buf.dtype == torch.float32 and not opt.buf.any()
    assert float(opt.lr_dev) == pytest.approx(0.01) and int(opt.step_dev) == 0
    opt.param_groups[0]['lr'] = 0.5
    opt.sync_lr()
    assert float(opt.lr_dev) == 0.5
    with pytest.raises(ValueError):
        get_optimizer(AD(TRAIN=AD(OPTIMIZER='rmsprop', LR=0.01)), m)


def _roundtrip(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def test_fused_sgd_state_dict_interoperates_with_torch_sgd_and_resumes():
    """checkpoint['optimizer'] both ways, like the Adam resume test of tests/test_host_cpu.py: FusedSGD's state dict has
    torch.optim.SGD's layout -- one momentum_buffer per parameter in the reference's OIHW shapes, torch's param-group keys."""
    from fpd_amd.lib.utils.utils import FusedSGD
    m = _model()
    params = list(m.parameters())
    opt = FusedSGD(m, lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    sd0 = opt.state_dict()
    assert sd0['state'] == {}                                    # empty before the first step, like torch's
    ref0 = torch.optim.SGD(params, lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    assert sorted(sd0['param_groups'][0]) == sorted(ref0.state_dict()['param_groups'][0])
    assert sd0['param_groups'][0] == ref0.state_dict()['param_groups'][0]
    # FusedSGD checkpoint -> torch SGD: hand-set arena, one step taken
    opt.buf.copy_(torch.randn(opt.buf.shape, generator=torch.Generator().manual_seed(0)))
    opt.step_dev.fill_(1)
    opt.param_groups[0]['initial_lr'] = 0.05
    opt.param_groups[0]['lr'] = 0.005                            # a decayed lr, as a checkpoint written after a milestone has
    sd = _roundtrip(opt.state_dict())
    assert sorted(sd['state']) == list(range(len(params)))
    ref = torch.optim.SGD(params, lr=7.0, momentum=0.1)
    ref.load_state_dict(sd)
    g = ref.param_groups[0]
    assert (g['lr'], g['initial_lr'], g['momentum'], g['weight_decay'], g['nesterov'], g['dampening']) == (0.005, 0.05, 0.9, 1e-4, True, 0)
    views = opt._views(opt.buf)
    assert len(views) == len(params) and any(v.dim() == 4 and not v.is_contiguous() for v in views)      # OIHW views of K,R,S,C memory
    for p, v in zip(params, views):
        assert ref.state[p]['momentum_buffer'].shape == p.shape and torch.equal(ref.state[p]['momentum_buffer'], v)
    # torch SGD checkpoint -> a fresh FusedSGD (AUTO_RESUME): the arena comes back bit for bit
    opt2 = FusedSGD(m, lr=3.0, momentum=0.5)
    opt2.load_state_dict(_roundtrip(ref.state_dict()))
    assert torch.equal(opt2.buf, opt.buf)
    g2 = opt2.param_groups[0]
    assert (g2['lr'], g2['initial_lr'], g2['momentum'], g2['weight_decay'], g2['nesterov']) == (0.005, 0.05, 0.9, 1e-4, True)
    assert float(opt2.lr_dev) == pytest.approx(0.005)
    assert sorted(opt2.state_dict()['state']) == list(range(len(params)))      # a resumed optimizer writes its buffers again
    # a reference checkpoint whose momentum_buffer is None (a parameter that has not stepped): a zero buffer
    sd_none = ref.state_dict()
    sd_none['state'] = {i: {'momentum_buffer': None} for i in range(len(params))}
    opt2.load_state_dict(sd_none)
    assert not opt2.buf.any()
    # momentum arriving with the checkpoint allocates the arena
    opt3 = FusedSGD(m, lr=0.1)
    opt3.load_state_dict(_roundtrip(ref.state_dict()))
    assert opt3.buf is not None and torch.equal(opt3.buf, opt.buf) and opt3.param_groups[0]['momentum'] == 0.9
    # what the kernel does not implement is refused, not ignored
    for key, val in (('dampening', 0.1), ('maximize', True)):
        bad = ref.state_dict()
        bad['param_groups'][0][key] = val
        with pytest.raises(ValueError, match=key):
            opt2.load_state_dict(bad)
    short = ref.state_dict()
    del short['state'][0]
    with pytest.raises(ValueError, match='entries'):
        opt2.load_state_dict(short)


def test_train_tool_shares_the_loop_of_fpd_train(monkeypatch):
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', os.environ.get('GPU_MAX_HW_QUEUES', '4'))     # importing the tools must not change it
    monkeypatch.syspath_prepend(os.path.join(ROOT, 'tools'))
    monkeypatch.setattr('sys.argv', ['train.py', '--cfg', 'x.yaml', '--max-iters', '2', 'TRAIN.OPTIMIZER', 'sgd'])
    import fpd_train
    import train
    seen = []
    monkeypatch.setattr(fpd_train, 'run', lambda args, normal=False: seen.append((args, normal)))
    train.main()
    (args, normal), = seen
    assert normal is True and args.cfg == 'x.yaml' and args.max_iters == 2 and args.opts == ['TRAIN.OPTIMIZER', 'sgd']
    assert not hasattr(args, 'tcfg')
    with pytest.raises(SystemExit):                              # no --tcfg on this command line
        monkeypatch.setattr('sys.argv', ['train.py', '--cfg', 'x.yaml', '--tcfg', 't.yaml'])
        train.main()
    monkeypatch.setattr('sys.argv', ['fpd_train.py', '--cfg', 's.yaml', '--tcfg', 't.yaml'])
    fpd_train.main()
    assert seen[-1][1] is False and seen[-1][0].tcfg == 't.yaml'
    src = open(os.path.join(ROOT, 'tools', 'train.py')).read()
    assert 'for epoch' not in src and 'get_optimizer' not in src.split('"""')[2]      # no second copy of the loop
