"""Fused SGD on the MI355X: the flat kernel (csrc/loss_adam.hip sgd_kernel) bit for bit on dyadic inputs and within float32
torch's own error on general ones, FusedSGD through core.function.fpd_train / train and through the module API, and
tools/train.py as a subprocess.  The reference of every comparison is torch.optim.SGD on the CPU (tests/_sgd_ref.py)."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import _cases, _sgd_ref
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GRID_CAP = 4 * 4096 * 256          # elements one pass of the capped grid covers with 16-byte vectors: beyond it the loop iterates


class AD(dict):
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def _inputs(n):
    return _sgd_ref.dyadic_inputs(n)


@functools.lru_cache(maxsize=None)
def _reference(n, momentum, wd, nesterov, grad_scale):
    p0, grads = _inputs(n)
    return _sgd_ref.sgd_trajectory(p0, [g * grad_scale for g in grads], _sgd_ref.LRS, momentum, wd, nesterov)


def _run_kernel(p0, grads, lrs, momentum, wd, nesterov, grad_scale=1.0, offset=0, with_buf=True, with_lp=True):
    """Three fpd_sgd calls with the lr delivered through lr_dev only; every arena starts `offset` elements into its allocation.
    Returns (param, buf or None, param_lp or None, step) on the CPU."""
    from fpd_amd import runtime as R
    dev = torch.device('cuda:0')
    n = p0.numel()
    arena = lambda src=None, dtype=torch.float32: (torch.zeros(n + offset, dtype=dtype, device=dev) if src is None
                                                   else torch.cat([torch.zeros(offset), src]).to(dev))[offset:]
    p, buf = arena(p0), (arena() if with_buf else None)
    lp = arena(dtype=torch.bfloat16) if with_lp else None
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    lr = torch.zeros(1, device=dev)
    for g, l in zip(grads, lrs):
        gd = arena(g)
        lr.fill_(l)
        a = R.SgdT()
        a.n, a.param, a.grad = n, p.data_ptr(), gd.data_ptr()
        a.buf = buf.data_ptr() if buf is not None else None
        a.param_lp = lp.data_ptr() if lp is not None else None
        a.lr, a.momentum, a.weight_decay, a.grad_scale, a.nesterov = 0.0, momentum, wd, grad_scale, int(nesterov)
        a.lr_dev, a.step_dev = lr.data_ptr(), step.data_ptr()
        R.check(R.lib().fpd_sgd(a, R.current_stream()), 'fpd_sgd')
    torch.cuda.synchronize()
    return p.cpu(), (buf.cpu() if buf is not None else None), (lp.cpu() if lp is not None else None), int(step.item())


def _assert_exact(n, momentum, wd, nesterov, grad_scale=1.0, **kw):
    p0, grads = _inputs(n)
    ref_p, ref_b = _reference(n, momentum, wd, nesterov, grad_scale)[-1]
    p, buf, lp, step = _run_kernel(p0, grads, _sgd_ref.LRS, momentum, wd, nesterov, grad_scale, **kw)
    assert step == 3
    assert torch.equal(p, ref_p), 'parameters: %d of %d differ, max %.3e' % ((p != ref_p).sum(), n, (p - ref_p).abs().max())
    if momentum != 0:
        assert torch.equal(buf, ref_b), 'momentum buffer: max %.3e' % (buf - ref_b).abs().max()
    elif buf is not None:
        assert not buf.any()                                     # no momentum: the buffer is not touched
    if lp is not None:
        assert torch.equal(lp.view(torch.int16), p.bfloat16().view(torch.int16))      # round to nearest even
        if momentum != 0 or wd != 0:                             # (plain SGD keeps these inputs within bf16's 8 bits)
            assert not torch.equal(lp.float(), p)                # ... of values that do need rounding


@pytest.mark.parametrize('n', [1, 4099, 100003])
@pytest.mark.parametrize('momentum,wd,nesterov', _sgd_ref.VARIANTS)
def test_sgd_kernel_is_bit_exact_on_the_dyadic_trajectory(n, momentum, wd, nesterov):
    if n == 1:                                                   # one element: no claim about how many values need rounding
        p0, grads = _inputs(n)
        ref_p, ref_b = _reference(n, momentum, wd, nesterov, 1.0)[-1]
        p, buf, lp, step = _run_kernel(p0, grads, _sgd_ref.LRS, momentum, wd, nesterov)
        assert step == 3 and torch.equal(p, ref_p) and (momentum == 0 or torch.equal(buf, ref_b))
        assert torch.equal(lp.view(torch.int16), p.bfloat16().view(torch.int16))
        return
    _assert_exact(n, momentum, wd, nesterov)


def test_sgd_kernel_grad_scale_null_buffer_unaligned_arenas_and_capped_grid():
    _assert_exact(4099, 0.5, 0.25, True, grad_scale=0.5)         # the reference is fed g / 2
    _assert_exact(4099, 0.0, 0.25, False, with_buf=False)        # momentum 0 with buf = NULL succeeds
    _assert_exact(100003, 0.0, 0.0, False, with_buf=False, with_lp=False)
    _assert_exact(4099, 0.5, 0.25, True, offset=1)               # arenas 4 bytes off a 16-byte boundary: element by element
    _assert_exact(4099, 0.5, 0.25, False, offset=2)              # 8 bytes off
    _assert_exact(GRID_CAP + 4099, 0.5, 0.25, True)              # more vectors than the capped grid has threads: the loop iterates
    _assert_exact(4099, 0.0, 0.25, False, offset=1)              # the kernel without momentum on the same two paths
    _assert_exact(GRID_CAP + 4099, 0.0, 0.25, False)


@pytest.mark.parametrize('nesterov', [False, True])
def test_sgd_kernel_general_inputs_are_as_close_to_fp64_torch_as_fp32_torch_is(nesterov):
    n, lrs, hp = 100003, (0.1, 0.1, 0.1), (0.9, 1e-4, nesterov)
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=gen)
    grads = [0.01 * torch.randn(n, generator=gen) for _ in lrs]
    (r32, b32), (r64, b64) = (_sgd_ref.sgd_trajectory(p0, grads, lrs, *hp, dtype=dt)[-1] for dt in (torch.float32, torch.float64))
    p, buf, _, step = _run_kernel(p0, grads, lrs, *hp)
    assert step == 3
    ratio = _sgd_ref.assert_as_close_as_fp32(p, r32, r64, 'parameters, nesterov %s' % nesterov)
    _sgd_ref.assert_as_close_as_fp32(buf, b32, b64, 'momentum buffer, nesterov %s' % nesterov)
    print('sgd kernel, nesterov %s: max|ours - r64| / max|r32 - r64| = %.3f' % (nesterov, ratio))


def _models():
    from tests.test_model_gpu import build_models
    return build_models('tiny')


class _Loader:
    def __init__(self, step):
        self.b = [_cases.batch('tiny', step)]

    def __iter__(self):
        for x, t, w in self.b:
            yield x, t, w, {}

    def __len__(self):
        return len(self.b)


def _cfgnode(alpha):
    return AD(KD=AD(ALPHA=alpha), PRINT_FREQ=1, DEBUG=AD(DEBUG=False))


HP = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)


class _CpuSgd:
    """torch.optim.SGD restated on (parameters before, gradient) of every call, in float32 and float64, each carrying its own buffer."""

    def __init__(self):
        self.buf = {torch.float32: None, torch.float64: None}

    def check(self, before, grad, after, lr, label):
        r = {}
        for dt in self.buf:
            (r[dt], self.buf[dt]), = _sgd_ref.sgd_trajectory(before, [grad], [lr], HP['momentum'], HP['weight_decay'], HP['nesterov'],
                                                             dtype=dt, buf0=self.buf[dt])
        assert float(grad.abs().max()) > 0 and not torch.equal(before, after)
        return _sgd_ref.assert_as_close_as_fp32(after, r[torch.float32], r[torch.float64], label)


@pytest.mark.parametrize('kd', [True, False])
def test_fused_step_runs_sgd_through_fpd_train_and_train(kd):
    """Two one-iteration epochs on distinct batches through core.function.fpd_train (kd) / train (no teacher), then one at lr 0."""
    from fpd_amd import runtime as R
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.utils.utils import FusedSGD
    c, gold, student, teacher = _models()
    opt = FusedSGD(student, **HP)
    crit = JointsMSELoss(True).cuda()
    A = student.device_state().A
    param, grad = A.tensor('param'), A.tensor('grad')
    alpha = 0.5 if kd else 0.0

    def epoch(k):
        torch.cuda.synchronize()
        before = param.detach().cpu().clone()
        if kd:
            F.fpd_train(_cfgnode(alpha), _Loader(k), student, teacher, crit, crit, opt, k, '/tmp', '/tmp', None)
        else:
            F.train(_cfgnode(alpha), _Loader(k), student, crit, opt, k, '/tmp', '/tmp', None)
        torch.cuda.synchronize()
        step = F.fused_step_for(student, teacher if kd else None, opt, _cases.batch('tiny', 0)[0].shape, alpha, 1, (True, True))
        return before, grad.detach().cpu().clone(), param.detach().cpu().clone(), step
    ref = _CpuSgd()
    steps, grads = [], []
    for k in range(2):
        before, g, after, step = epoch(k)
        ratio = ref.check(before, g, after, HP['lr'], 'call %d' % k)
        print('fused step (kd %s) call %d: max|ours - r64| / max|r32 - r64| = %.3f' % (kd, k, ratio))
        steps.append(step); grads.append(g)
    assert int(opt.step_dev) == 2
    assert steps[0] is steps[1]                                  # the second call hit the step cache
    assert not torch.equal(grads[0], grads[1])                   # the batches really differ
    assert steps[0].buf is opt.buf and steps[0].m is None and steps[0].v is None      # shared buffer, no Adam moments
    assert steps[0].student.plan.op_type(steps[0].student.rng['adam'][0]) == R.OP_SGD
    assert steps[0].launches_per_step()['student_adam'] == 1
    _sgd_ref.assert_as_close_as_fp32(opt.buf.cpu(), ref.buf[torch.float32], ref.buf[torch.float64], 'momentum buffer after two calls')
    # lr 0 through param_groups: parameters stand still, the momentum buffer still moves
    buf_before = opt.buf.detach().cpu().clone()
    opt.param_groups[0]['lr'] = 0.0
    before, g, after, step = epoch(2)
    assert step is steps[0] and float(opt.lr_dev) == 0.0 and int(opt.step_dev) == 3
    assert torch.equal(before, after) and not torch.equal(buf_before, opt.buf.cpu())
    # a changed hyperparameter lives in the recorded op: a new step, not a stale replay
    opt.param_groups[0]['weight_decay'] = 0.0
    assert F.fused_step_for(student, teacher if kd else None, opt, _cases.batch('tiny', 0)[0].shape, alpha, 1, (True, True)) is not step


def test_sgd_step_has_the_launch_count_of_the_adam_step():
    from fpd_amd import executor as E
    from fpd_amd.lib.utils.utils import FusedSGD
    c, gold, student, teacher = _models()
    mk = lambda **kw: E.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, c['batch'],
                                     c['image'][1], c['image'][0], alpha=0.5, **kw)
    adam, sgd = mk().launches_per_step(), mk(sgd=FusedSGD(student, **HP)).launches_per_step()
    print('launches per step on the tiny pair: adam %r sgd %r' % (adam, sgd))
    assert adam == sgd
    from fpd_amd import runtime as R
    from fpd_amd.lib.utils.utils import FusedAdam
    with pytest.raises(R.FpdError, match='exclusive'):
        mk(sgd=FusedSGD(student, **HP), adam=FusedAdam(student))


def test_module_api_backward_then_fused_sgd_step():
    """loss.backward(); optimizer.step() (lib/core/function.py:119-146 of the reference) with FusedSGD, one step."""
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.utils.utils import FusedSGD
    c, gold, student, teacher = _models()
    opt = FusedSGD(student, **HP)
    crit = JointsMSELoss(True).cuda()
    x, tg, tw = (t.cuda() for t in _cases.batch('tiny', 0))
    student.train()
    A = student.device_state().A
    before = A.tensor('param').detach().cpu().clone()
    opt.zero_grad()
    outputs = student(x)
    loss = crit(outputs[0], tg, tw)
    for o in outputs[1:]:
        loss = loss + crit(o, tg, tw)
    loss.backward()
    torch.cuda.synchronize()
    g = A.tensor('grad').detach().cpu().clone()
    opt.step()
    torch.cuda.synchronize()
    ratio = _CpuSgd().check(before, g, A.tensor('param').detach().cpu(), HP['lr'], 'module API')
    print('module API: max|ours - r64| / max|r32 - r64| = %.3f' % ratio)
    assert int(opt.step_dev) == 1
    sd = opt.state_dict()                                        # one momentum_buffer per parameter, in the parameter's shape
    params = list(student.parameters())
    assert sorted(sd['state']) == list(range(len(params)))
    assert all(sd['state'][i]['momentum_buffer'].shape == p.shape for i, p in enumerate(params))


def test_tools_train_cli_sgd_and_auto_resume(tmp_path):
    """`python tools/train.py --cfg ... KEY VALUE` (the reference's tools/train.py) with TRAIN.OPTIMIZER sgd for one epoch of 2
    iterations, then a second launch that AUTO_RESUMEs from checkpoint.pth and runs epoch 1."""
    cfgd = os.path.join(ROOT, 'experiments', 'fpd_synthetic')
    base = [sys.executable, os.path.join(ROOT, 'tools', 'train.py'), '--cfg', os.path.join(cfgd, 'hg4x128_student.yaml'),
            '--max-iters', '2',
            'OUTPUT_DIR', str(tmp_path), 'MODEL.EXTRA.NUM_FEATURES', '32', 'MODEL.EXTRA.NUM_STACKS', '2', 'MODEL.IMAGE_SIZE', '128,128',
            'MODEL.HEATMAP_SIZE', '32,32', 'TRAIN.BATCH_SIZE_PER_GPU', '4', 'DATASET.NUM_SAMPLES', '32', 'PRINT_FREQ', '1',
            'TRAIN.LR_STEP', '[2,3]', 'AUTO_RESUME', 'True', 'MODEL.DTYPE', 'fp32',
            'TRAIN.OPTIMIZER', 'sgd', 'TRAIN.LR', '0.01', 'TRAIN.NESTEROV', 'True']
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(base + ['TRAIN.END_EPOCH', '1'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])      # nothing further is started when this launch fails
    log = r.stdout + r.stderr
    assert sum(1 for l in log.splitlines() if 'Epoch: [0][' in l and '\tLoss ' in l) == 2 and 'POSE_Loss' not in log and 'epoch 0 done' in log
    ckpts = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f == 'checkpoint.pth']
    assert len(ckpts) == 1
    ck = torch.load(ckpts[0], map_location='cpu', weights_only=False)
    g = ck['optimizer']['param_groups'][0]
    assert ck['epoch'] == 1 and (g['momentum'], g['nesterov'], g['weight_decay'], g['initial_lr']) == (0.9, True, 1e-4, 0.01)
    trainable = [k for k in ck['best_state_dict'] if 'running' not in k and 'tracked' not in k]
    st = ck['optimizer']['state']
    assert sorted(st) == list(range(len(trainable)))
    assert all(st[i]['momentum_buffer'].shape == ck['best_state_dict'][k].shape for i, k in enumerate(trainable))
    assert any(float(e['momentum_buffer'].abs().max()) > 0 for e in st.values())
    r2 = subprocess.run(base + ['TRAIN.END_EPOCH', '2'], env=env, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, (r2.stdout[-1500:], r2.stderr[-3000:])
    log2 = r2.stdout + r2.stderr
    assert 'loaded checkpoint' in log2 and 'epoch 1 done' in log2 and 'epoch 0 done' not in log2 and 'POSE_Loss' not in log2
    assert torch.load(ckpts[0], map_location='cpu', weights_only=False)['epoch'] == 2
    assert any(f == 'final_state.pth' for _, _, fs in os.walk(tmp_path) for f in fs)
