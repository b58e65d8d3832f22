"""fpd_adamw / FusedAdamW on the MI355X.  The kernel (csrc/adamw.hip) bit for bit against the numpy restatement of
csrc/adamw_math.h (tests/_adamw_ref.py; its preconditions in tests/test_adamw_cpu.py) on the vector and the element path, both
ways of passing the schedule, the exemption mask, the dyadic trajectory bit for bit against torch.optim.AdamW, zero gradients,
general inputs within twice float32 torch's own error, refusals; then FusedAdamW through core.function.fpd_train / train, the
module API and tools/train.py.  Every arena is sentinel-filled with guard elements on both sides, which have to stay intact,
and the gradient is never written."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _adamw_ref as W, _cases, _sgd_ref, _step_cases as SC
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

R = None
DEV = torch.device('cuda:0')
G = SC.GUARD
BIG = 4096 * 256 + 4099
GRID_CAP = 4 * 4096 * 256          # elements one pass of the capped grid covers with 16-byte vectors: beyond it the loop iterates


def setup_module(module):
    global R
    from fpd_amd import runtime
    R = runtime
    R.lib()


class Guarded:
    """n elements with G sentinel-filled guard elements on each side (and `offset` more in front: a start off the 16-byte grid)."""

    def __init__(self, n, dtype, src=None, offset=0):
        self.n, self.lo = n, G + offset
        self.full = torch.full((n + 2 * G + offset,), SC.SENTINEL, dtype=dtype, device=DEV)
        self.sent = self.full[:1].clone()
        self.t = self.full[self.lo:self.lo + n]
        if src is not None:
            self.t.copy_(src.reshape(-1).to(dtype))

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.full[:self.lo] == self.sent).all() and (self.full[self.lo + self.n:] == self.sent).all())

    def cpu(self):
        return self.t.cpu()


def run_adamw(p0, grads, lrs, betas=W.BETAS, eps=W.EPS, wd=0.01, amsgrad=False, grad_scale=1.0, host_schedule=False, with_lp=True,
              offset=0, exempt=None, expect_vec=None):
    """fpd_adamw once per gradient.  The schedule through step_dev + lr_dev, or -- host_schedule -- bias_corr1 / bias_corr2 / lr
    in the struct with both pointers NULL.  -> dict(p, m, v, vmax or None, lp or None: CPU tensors, step)"""
    n = p0.numel()
    zeros = torch.zeros(n)
    p, m, v = (Guarded(n, torch.float32, s, offset) for s in (p0, zeros, zeros))
    x = Guarded(n, torch.float32, zeros, offset) if amsgrad else None
    lp = Guarded(n, torch.bfloat16, None, offset) if with_lp else None
    mask = torch.from_numpy(W.mask_words(exempt).view(np.int32).copy()).to(DEV) if exempt is not None else None
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    lr = torch.zeros(1, device=DEV)
    for t, (g, l) in enumerate(zip(grads, lrs), start=1):
        gd = Guarded(n, torch.float32, g, offset)
        lr.fill_(l)
        a = R.AdamWT()
        a.n, a.param, a.grad, a.m, a.v = n, p.ptr(), gd.ptr(), m.ptr(), v.ptr()
        a.vmax = x.ptr() if x is not None else None
        a.param_lp = lp.ptr() if lp is not None else None
        a.no_decay_bits = mask.data_ptr() if mask is not None else None
        a.beta1, a.beta2, a.eps, a.grad_scale, a.weight_decay = betas[0], betas[1], eps, grad_scale, wd
        if host_schedule:
            bc1, bc2 = W.bias_corrections(t, betas)
            a.lr, a.bias_corr1, a.bias_corr2, a.lr_dev, a.step_dev = l, float(bc1), float(bc2), None, None
        else:
            a.lr, a.bias_corr1, a.bias_corr2, a.lr_dev, a.step_dev = 0.0, 1.0, 1.0, lr.data_ptr(), step.data_ptr()
        if expect_vec is not None:
            import ctypes as C
            blocks, vec = C.c_int32(), C.c_int64()
            R.check(R.lib().fpd_adamw_geometry(a, blocks, vec), 'fpd_adamw_geometry')
            assert vec.value == expect_vec, (vec.value, expect_vec)       # the path this case is there for, as launched
        R.check(R.lib().fpd_adamw(a, R.current_stream()), 'fpd_adamw')
        torch.cuda.synchronize()
        assert gd.intact() and torch.equal(SC.bits(gd.cpu()), SC.bits(g.float())), 'the gradient or its guard was written'
    assert all(z is None or z.intact() for z in (p, m, v, x, lp)), 'a guard element was written'
    return dict(p=p.cpu(), m=m.cpu(), v=v.cpu(), vmax=x.cpu() if x is not None else None, lp=lp.cpu() if lp is not None else None,
                step=int(step.item()))


def _assert_bits(got, want, keys, label):
    for k in keys:
        g, w = got[k], want[k]
        assert not bool(torch.isnan(w).any())
        assert torch.equal(SC.bits(g), SC.bits(w)), '%s: %s: %d of %d elements differ, max %.3e' % (
            label, k, int((SC.bits(g) != SC.bits(w)).sum()), g.numel(), float((g.float() - w.float()).abs().max()))


@functools.lru_cache(maxsize=None)
def _general(n, regime='small', kind='randn'):
    return W.start(kind, n), W.gradients(regime, n)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel against the restatement

@pytest.mark.parametrize('amsgrad', [False, True])
@pytest.mark.parametrize('wd', [0.0, 0.25])
@pytest.mark.parametrize('n,offset', [(1, 0), (4099, 0), (4099, 1), (4099, 2), (BIG, 0), (BIG, 1)])
def test_kernel_is_the_restatement_bit_for_bit(n, offset, wd, amsgrad):
    """Host schedule, grad_scale 0.5, with and without the bf16 copy; n = 4096 * 256 + 4099 is past the capped grid on the
    element path (offset 1), where a thread owns a second element."""
    p0, grads = _general(n)
    want = W.restated(p0, grads, W.LRS, W.BETAS, W.EPS, wd, amsgrad, grad_scale=0.5)
    keys = ('p', 'm', 'v') + (('vmax',) if amsgrad else ())
    vec = n // 4 * 4 if offset == 0 else 0
    for with_lp in (True, False):
        got = run_adamw(p0, grads, W.LRS, wd=wd, amsgrad=amsgrad, grad_scale=0.5, host_schedule=True, with_lp=with_lp, offset=offset,
                        expect_vec=vec)
        assert got['step'] == 0
        _assert_bits(got, want, keys, 'n %d offset %d wd %g amsgrad %s lp %s' % (n, offset, wd, amsgrad, with_lp))
        if with_lp:
            assert torch.equal(SC.bits(got['lp']), SC.bits(want['p'].bfloat16()))        # round to nearest even ...
            assert n == 1 or not torch.equal(got['lp'].float(), got['p'])                # ... of values that do need rounding
    if wd and n > 1:
        assert not torch.equal(want['p'], W.restated(p0, grads, W.LRS, W.BETAS, W.EPS, 0.0, amsgrad, grad_scale=0.5)['p'])


def test_vector_loop_iterates_past_the_capped_grid():
    """More 16-byte vectors than the capped grid has threads: a thread owns a second vector, with decay, AMSGrad and the mask
    (full), and with the decay alone."""
    n = GRID_CAP + 4099
    p0, grads = _general(n)
    for full in (True, False):
        exempt = W.exempt_of(n, W.mask_ranges(n) + [(GRID_CAP - 2, GRID_CAP + 3)]) if full else None
        got = run_adamw(p0, grads[:2], W.LRS[:2], wd=0.25, amsgrad=full, exempt=exempt, expect_vec=GRID_CAP + 4096)
        keys = ('p', 'm', 'v') + (('vmax',) if full else ())
        _assert_bits(got, W.restated(p0, grads[:2], W.LRS[:2], W.BETAS, W.EPS, 0.25, full, exempt=exempt), keys, 'past the cap')
        assert torch.equal(SC.bits(got['lp']), SC.bits(got['p'].bfloat16())) and got['step'] == 2


@pytest.mark.parametrize('offset', [0, 1])
def test_device_schedule_gives_the_bits_of_the_host_schedule_and_counts_three_steps(offset):
    p0, grads = _general(4099)
    lrs = (2.5e-4, 1e-3, 5e-4)
    for amsgrad in (False, True):
        dev = run_adamw(p0, grads, lrs, wd=0.25, amsgrad=amsgrad, offset=offset)
        host = run_adamw(p0, grads, lrs, wd=0.25, amsgrad=amsgrad, offset=offset, host_schedule=True)
        assert dev['step'] == 3 and host['step'] == 0
        _assert_bits(dev, host, ('p', 'm', 'v', 'lp') + (('vmax',) if amsgrad else ()), 'device against host schedule')
        _assert_bits(dev, W.restated(p0, grads, lrs, W.BETAS, W.EPS, 0.25, amsgrad), ('p', 'm', 'v'), 'device schedule')


@pytest.mark.parametrize('offset', [0, 1])
def test_mask_exempts_exactly_its_elements_on_the_vector_and_the_element_path(offset):
    # 4101: 1025 vectors and a one-element tail, which is exempt.  35: eight vectors and a three-element tail in the mask's second
    # word, with elements 31 and 32 (either side of the word boundary) and 34 (inside the tail) exempt
    for n, ranges in ((4101, W.mask_ranges(4101)), (35, [(31, 33), (34, 35)])):
        assert all(hi % 4 and (lo % 4 or lo == 0) for lo, hi in ranges)                    # none on a 4- (hence 32-) element boundary
        exempt = W.exempt_of(n, ranges)
        p0, grads = _general(n)
        run = lambda wd, ex: run_adamw(p0, grads, W.LRS, wd=wd, amsgrad=True, offset=offset, exempt=ex, expect_vec=n - n % 4 if offset == 0 else 0)
        masked, full, none = run(0.25, exempt), run(0.25, None), run(0.0, None)
        ex = torch.from_numpy(exempt)
        for k in ('p', 'lp'):
            assert torch.equal(SC.bits(masked[k])[ex], SC.bits(none[k])[ex]), k                # exempt: a run with weight_decay = 0
            assert torch.equal(SC.bits(masked[k])[~ex], SC.bits(full[k])[~ex]), k              # all others: a run with no mask
        assert not bool((masked['p'][ex] == full['p'][ex]).any())
        _assert_bits(masked, W.restated(p0, grads, W.LRS, W.BETAS, W.EPS, 0.25, True, exempt=exempt), ('p', 'm', 'v', 'vmax'), 'masked')
        _assert_bits(run(0.0, exempt), none, ('p', 'm', 'v', 'vmax', 'lp'), 'a mask without a decay')      # nobody reads it


@pytest.mark.parametrize('amsgrad', [False, True])
@pytest.mark.parametrize('n,offset', [(4099, 0), (4099, 1), (GRID_CAP // 4 + 4099, 0)])
def test_dyadic_trajectory_is_torchs_on_every_element(n, offset, amsgrad):
    p0, grads = W.dyadic_inputs(n)
    ref = W.dyadic_trajectory(p0, grads, amsgrad)
    got = run_adamw(p0, grads, W.DYADIC_LRS, (0.0, 0.0), 0.0, W.DYADIC_WD, amsgrad, offset=offset)
    assert got['step'] == 3
    for i, k in enumerate(('p', 'm', 'v') + (('vmax',) if amsgrad else ())):
        assert torch.equal(got[k], ref[i]) and not bool(torch.isnan(got[k]).any()), k


def test_zero_gradients_keep_the_moments_and_a_zero_parameter_with_decay_on():
    """What the arena's alignment gaps rely on: gradient 0 from the first step, parameter +-0."""
    n = 4099
    p0, grads = _general(n)
    p0, grads = p0.clone(), [g.clone() for g in grads]
    idle = torch.zeros(n, dtype=torch.bool)
    idle[[0, 1, 2, 3, 5, 70, 2048, 2049, n - 2, n - 1]] = True
    gaps = torch.zeros(n, dtype=torch.bool)
    gaps[[1, 2, 2048, n - 1]] = True                              # ... of which these have a zero parameter
    for g in grads:
        g[idle] = 0.0
    p0[gaps] = 0.0
    p0[[2, n - 1]] = -0.0
    for offset in (0, 1):
        for amsgrad in (False, True):
            got = run_adamw(p0, grads, W.LRS, wd=0.25, amsgrad=amsgrad, offset=offset)
            for k in ('m', 'v') + (('vmax',) if amsgrad else ()):
                assert not bool(got[k][idle].any()) and bool(got[k][~idle].all())
            assert torch.equal(SC.bits(got['p'])[gaps], SC.bits(p0)[gaps])              # +-0 keeps its bits
            rest = idle & ~gaps                                                         # a non-zero parameter only decays
            want = W.restated(p0, grads, W.LRS, W.BETAS, W.EPS, 0.25, amsgrad)
            assert torch.equal(SC.bits(got['p']), SC.bits(want['p'])) and bool((got['p'][rest].abs() < p0[rest].abs()).all())


B32 = tuple(float(np.float32(b)) for b in W.BETAS)


@pytest.mark.parametrize('kind', W.STARTS)
@pytest.mark.parametrize('regime', W.ALL_REGIMES)
def test_general_inputs_are_as_close_to_fp64_torch_as_fp32_torch_is(regime, kind):
    n, wd = 100003, 0.25
    p0, grads = _general(n, regime, kind)
    traj = lambda betas, dt: W.adamw_trajectory(p0, grads, W.LRS, betas, W.EPS, wd, True, dt)
    r32, r64, q32, q64 = traj(W.BETAS, torch.float32), traj(W.BETAS, torch.float64), traj(B32, torch.float32), traj(B32, torch.float64)
    got = run_adamw(p0, grads, W.LRS, wd=wd, amsgrad=True)
    assert got['step'] == 3
    rp = _sgd_ref.assert_as_close_as_fp32(got['p'], r32[0], r64[0], 'parameters, %s start, %s gradients' % (kind, regime))
    rs = [_sgd_ref.assert_as_close_as_fp32(got[k], q32[i], q64[i], '%s, %s start, %s gradients' % (k, kind, regime))
          for i, k in ((1, 'm'), (2, 'v'), (3, 'vmax'))]
    print('adamw %s start, %s gradients: ratio parameters %.3f, m %.3f, v %.3f, vmax %.3f' % ((kind, regime, rp) + tuple(rs)))
    _assert_bits(got, W.restated(p0, grads, W.LRS, W.BETAS, W.EPS, wd, True), ('p', 'm', 'v', 'vmax'), 'general inputs')


def test_refusals_launch_nothing_and_a_null_vmax_is_not_amsgrad():
    n = 4099
    p0, grads = _general(n)
    p, g, m, v, x = (Guarded(n, torch.float32, s) for s in (p0, grads[0], torch.zeros(n), torch.zeros(n), torch.zeros(n)))

    def args(**kw):
        a = R.AdamWT()
        a.n, a.param, a.grad, a.m, a.v, a.vmax = n, p.ptr(), g.ptr(), m.ptr(), v.ptr(), x.ptr()
        a.lr, a.beta1, a.beta2, a.eps, a.grad_scale, a.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 1.0, 0.25
        a.bias_corr1, a.bias_corr2 = (float(b) for b in W.bias_corrections(1))
        for k, val in kw.items():
            setattr(a, k, val)
        return a
    lib = R.lib()
    for word, kw in (('weight_decay', dict(weight_decay=-0.25)), ('overlaps', dict(m=p.ptr())), ('overlaps', dict(vmax=v.ptr() + 16)),
                     ('overlaps', dict(grad=m.ptr() + 4 * (n - 1))), ('overlaps', dict(param_lp=v.ptr())), ('null', dict(v=None))):
        rc = lib.fpd_adamw(args(**kw), R.current_stream())
        assert rc < 0 and word in lib.fpd_last_error().decode(), (kw, rc, lib.fpd_last_error())
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), p0) and not bool(m.cpu().any()) and not bool(v.cpu().any()) and not bool(x.cpu().any())
    # vmax == NULL is served, as plain AdamW: the same bits as the host-schedule run without AMSGrad, and no maximum is written
    R.check(lib.fpd_adamw(args(vmax=None), R.current_stream()), 'fpd_adamw')
    torch.cuda.synchronize()
    want = W.restated(p0, grads[:1], (1e-3,), W.BETAS, W.EPS, 0.25, False)
    assert torch.equal(SC.bits(p.cpu()), SC.bits(want['p'])) and torch.equal(SC.bits(v.cpu()), SC.bits(want['v'])) and not bool(x.cpu().any())
    assert all(z.intact() for z in (p, g, m, v, x))


# ---------------------------------------------------------------------------------------------------------------------
# FusedAdamW in the fused step, the module API and the tools

class AD(dict):
    __getattr__ = dict.__getitem__


def _models():
    from tests.test_model_gpu import build_models
    return build_models('tiny')


class _Loader:
    def __init__(self, *steps):
        self.b = [_cases.batch('tiny', s) for s in steps]

    def __iter__(self):
        for x, t, w in self.b:
            yield x, t, w, {}

    def __len__(self):
        return len(self.b)


def _cfgnode(alpha):
    return AD(KD=AD(ALPHA=alpha), PRINT_FREQ=1, DEBUG=AD(DEBUG=False))


HP = dict(lr=1e-3, weight_decay=0.05)


class _Restated:
    """The restatement applied to (parameters before, gradient arena) of every update, carrying its own moments."""

    def __init__(self, opt):
        self.opt, self.state, self.t = opt, None, 0
        n = opt.m.numel()
        self.exempt = W.exempt_of(n, opt.no_decay_ranges) if opt.no_decay_norm_bias else None

    def check(self, before, grad, after, lr, label):
        g = self.opt.param_groups[0]
        self.t += 1
        r = W.restated(before, [grad], [lr], g['betas'], g['eps'], g['weight_decay'], self.opt.amsgrad, exempt=self.exempt,
                       state=self.state, first_step=self.t)
        self.state = (r['m'], r['v'], r['vmax'])
        assert float(grad.abs().max()) > 0 and not torch.equal(before, after)
        got = dict(p=after, m=self.opt.m.cpu(), v=self.opt.v.cpu(), vmax=self.opt.vmax.cpu() if self.opt.amsgrad else None)
        _assert_bits(got, r, ('p', 'm', 'v') + (('vmax',) if self.opt.amsgrad else ()), label)
        return r


@pytest.mark.parametrize('variant', ['decay', 'decay+exemption', 'decay+amsgrad'])
@pytest.mark.parametrize('kd', [True, False])
def test_fused_step_runs_adamw_through_fpd_train_and_train(kd, variant):
    """Two one-iteration epochs on distinct batches through core.function.fpd_train (kd) / train (no teacher)."""
    from fpd_amd import executor as E
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.utils.utils import FusedAdamW
    c, gold, student, teacher = _models()
    opt = FusedAdamW(student, amsgrad='amsgrad' in variant, no_decay_norm_bias='exemption' in variant, **HP)
    crit = JointsMSELoss(True).cuda()
    A = student.device_state().A
    param, grad = A.tensor('param'), A.tensor('grad')
    alpha = 0.5 if kd else 0.0
    shape = _cases.batch('tiny', 0)[0].shape
    ref, steps = _Restated(opt), []
    for k in range(2):
        torch.cuda.synchronize()
        before = param.detach().cpu().clone()
        if kd:
            F.fpd_train(_cfgnode(alpha), _Loader(k), student, teacher, crit, crit, opt, k, '/tmp', '/tmp', None)
        else:
            F.train(_cfgnode(alpha), _Loader(k), student, crit, opt, k, '/tmp', '/tmp', None)
        torch.cuda.synchronize()
        ref.check(before, grad.detach().cpu().clone(), param.detach().cpu().clone(), HP['lr'], '%s call %d' % (variant, k))
        steps.append(F.fused_step_for(student, teacher if kd else None, opt, shape, alpha, 1, (True, True)))
    step = steps[0]
    assert int(opt.step_dev) == 2 and steps[1] is step                                      # the second call hit the step cache
    assert step.m is opt.m and step.v is opt.v and step.vmax is opt.vmax and step.step_dev is opt.step_dev and step.lr_dev is opt.lr_dev
    b, e = step.student.rng['adam']
    assert e - b == 1 and step.student.plan.op_type(b) == R.OP_ADAMW
    if opt.no_decay_norm_bias:                                                               # the exemption did something
        ex = torch.from_numpy(ref.exempt)
        assert bool(ex.any()) and not bool(ex.all()) and int(ex.sum()) == sum(hi - lo for lo, hi in opt.no_decay_ranges)
    if kd and variant == 'decay':
        plain = E.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, c['batch'], c['image'][1],
                               c['image'][0], alpha=0.5)
        print('launches per step on the tiny pair: adam %r adamw %r' % (plain.launches_per_step(), step.launches_per_step()))
        assert plain.launches_per_step() == step.launches_per_step() and step.launches_per_step()['student_adam'] == 1
        # a changed hyperparameter lives in the recorded op: a new step, not a stale replay
        opt.param_groups[0]['weight_decay'] = 0.0
        assert F.fused_step_for(student, teacher, opt, shape, alpha, 1, (True, True)) is not step


def test_fused_step_refuses_the_adamw_of_another_model():
    from fpd_amd import executor as E
    from fpd_amd.lib.utils.utils import FusedAdamW
    c, gold, student, teacher = _models()
    other = FusedAdamW(teacher, amsgrad=True, no_decay_norm_bias=True, **HP)      # its arenas have the teacher's size
    assert other.m.numel() != student.table.sizes['param']
    with pytest.raises(R.FpdError, match='another model'):
        E.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, c['batch'], c['image'][1],
                       c['image'][0], alpha=0.5, adam=other)


def test_fused_step_with_clip_and_ema_keeps_adamw_between_them():
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.utils.utils import FusedAdamW, GradClipper, ModelEma
    c, gold, student, teacher = _models()
    opt = FusedAdamW(student, amsgrad=True, no_decay_norm_bias=True, **HP)
    probe = GradClipper(student, float('inf'))
    crit = JointsMSELoss(True).cuda()
    A = student.device_state().A
    param, grad = A.tensor('param'), A.tensor('grad')
    ref = _Restated(opt)
    ema = ModelEma(student, decay=0.9, warmup=False)
    clip = None
    for k in range(2):
        torch.cuda.synchronize()
        before = param.detach().cpu().clone()
        if k == 1:                                                # clip the second update to a hundredth of the norm the first one had
            clip = GradClipper(student, 0.01 * norm)
        F.fpd_train(_cfgnode(0.5), _Loader(k), student, teacher, crit, crit, opt, k, '/tmp', '/tmp', None, ema=ema, clip=clip or probe)
        torch.cuda.synchronize()
        norm = probe.norm()
        # the clip scales the gradient arena in place, so the arena holds what the optimizer read
        ref.check(before, grad.detach().cpu().clone(), param.detach().cpu().clone(), HP['lr'], 'clip + ema, call %d' % k)
    step = F.fused_step_for(student, teacher, opt, _cases.batch('tiny', 0)[0].shape, 0.5, 1, (True, True), ema=ema, clip=clip)
    b, e = step.student.rng['adam']
    assert [step.student.plan.op_type(i) for i in range(b, e)] == [R.OP_GRAD_CLIP, R.OP_ADAMW, R.OP_EMA]
    assert clip.stats()['clipped'] == 1 and ema.updates == 2 and int(opt.step_dev) == 2


def test_window_of_two_identical_micro_batches_is_the_plain_update():
    from fpd_amd import executor as E
    from fpd_amd.lib.utils.utils import FusedAdamW
    out = []
    for accum in (1, 2):
        c, gold, student, teacher = _models()
        opt = FusedAdamW(student, amsgrad=True, no_decay_norm_bias=True, **HP)
        step = E.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, c['batch'], c['image'][1],
                              c['image'][0], alpha=0.5, adam=opt, accum=accum)
        for u in range(2):
            for _ in range(accum):
                b = _cases.batch('tiny', u)
                step.set_batch(*b)
                step.teacher_async(b[0])
                step.student_step(None)
        torch.cuda.synchronize()
        out.append((student.device_state().A.tensor('param').cpu().clone(), opt.m.cpu().clone(), opt.v.cpu().clone(), opt.vmax.cpu().clone(),
                    int(opt.step_dev)))
    assert out[0][4] == out[1][4] == 2
    for a, b, k in zip(out[0][:4], out[1][:4], ('p', 'm', 'v', 'vmax')):      # (g + g) * 0.5 = g exactly
        assert torch.equal(SC.bits(a), SC.bits(b)), k


def test_module_api_backward_then_fused_adamw_step():
    """loss.backward(); optimizer.step() with FusedAdamW, one step; the state dict it leaves loads into stock torch."""
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.utils.utils import FusedAdamW
    c, gold, student, teacher = _models()
    opt = FusedAdamW(student, amsgrad=True, no_decay_norm_bias=True, **HP)
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
    _Restated(opt).check(before, g, A.tensor('param').detach().cpu(), HP['lr'], 'module API')
    assert int(opt.step_dev) == 1
    sd = opt.state_dict()
    params = [p for grp in opt.param_groups for p in grp['params']]
    assert len(sd['param_groups']) == 2 and sorted(sd['state']) == list(range(len(params)))
    assert all(sd['state'][i]['max_exp_avg_sq'].shape == p.shape for i, p in enumerate(params))
    stock = torch.optim.AdamW([dict(params=[torch.nn.Parameter(torch.zeros_like(p)) for p in grp['params']], weight_decay=grp['weight_decay'])
                               for grp in opt.param_groups], lr=HP['lr'], amsgrad=True)
    stock.load_state_dict(sd)
    assert float(stock.state[stock.param_groups[1]['params'][0]]['step']) == 1


def test_tools_train_cli_adamw_amsgrad_exemption_and_auto_resume(tmp_path):
    """`python tools/train.py ... TRAIN.OPTIMIZER adamw TRAIN.AMSGRAD true TRAIN.NO_DECAY_NORM_BIAS true` for one epoch of 2
    iterations, then a second launch that AUTO_RESUMEs from checkpoint.pth and runs epoch 1."""
    cfgd = os.path.join(ROOT, 'experiments', 'fpd_synthetic')
    base = [sys.executable, os.path.join(ROOT, 'tools', 'train.py'), '--cfg', os.path.join(cfgd, 'hg4x128_student.yaml'),
            '--max-iters', '2',
            'OUTPUT_DIR', str(tmp_path), 'MODEL.EXTRA.NUM_FEATURES', '32', 'MODEL.EXTRA.NUM_STACKS', '2', 'MODEL.IMAGE_SIZE', '128,128',
            'MODEL.HEATMAP_SIZE', '32,32', 'TRAIN.BATCH_SIZE_PER_GPU', '4', 'DATASET.NUM_SAMPLES', '32', 'PRINT_FREQ', '1',
            'TRAIN.LR_STEP', '[2,3]', 'AUTO_RESUME', 'True', 'MODEL.DTYPE', 'fp32',
            'TRAIN.OPTIMIZER', 'adamw', 'TRAIN.AMSGRAD', 'true', 'TRAIN.NO_DECAY_NORM_BIAS', 'true', 'TRAIN.WD', '0.05', 'TRAIN.LR', '0.001']
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(base + ['TRAIN.END_EPOCH', '1'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])      # nothing further is started when this launch fails
    log = r.stdout + r.stderr
    assert sum(1 for l in log.splitlines() if 'Epoch: [0][' in l and '\tLoss ' in l) == 2 and 'epoch 0 done' in log
    ckpts = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f == 'checkpoint.pth']
    assert len(ckpts) == 1

    def look(path, epoch, steps):
        ck = torch.load(path, map_location='cpu', weights_only=False)
        groups, st = ck['optimizer']['param_groups'], ck['optimizer']['state']
        trainable = [k for k in ck['best_state_dict'] if 'running' not in k and 'tracked' not in k]
        assert ck['epoch'] == epoch and len(groups) == 2 and sorted(st) == list(range(len(trainable)))
        assert (groups[0]['weight_decay'], groups[1]['weight_decay'], groups[0]['amsgrad'], groups[0]['initial_lr']) == (0.05, 0, True, 0.001)
        k = len(groups[0]['params'])
        assert groups[0]['params'] == list(range(k)) and groups[1]['params'] == list(range(k, len(trainable))) and 0 < k < len(trainable)
        assert all(st[i]['exp_avg'].dim() >= 2 for i in range(k)) and all(st[i]['exp_avg'].dim() < 2 for i in range(k, len(trainable)))
        assert all(float(e['step']) == steps and bool((e['max_exp_avg_sq'] >= e['exp_avg_sq']).all()) for e in st.values())
        assert any(float(e['max_exp_avg_sq'].max()) > 0 for e in st.values())
    look(ckpts[0], 1, 2)
    r2 = subprocess.run(base + ['TRAIN.END_EPOCH', '2'], env=env, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, (r2.stdout[-1500:], r2.stderr[-3000:])
    log2 = r2.stdout + r2.stderr
    assert 'loaded checkpoint' in log2 and 'epoch 1 done' in log2 and 'epoch 0 done' not in log2
    look(ckpts[0], 2, 4)                                          # the resumed state carried on: four steps, still two groups
