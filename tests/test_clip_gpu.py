"""Global gradient-norm clipping on the MI355X: fpd_grad_clip (csrc/grad_clip.hip) against the numpy restatement
(tests/_clip_ref.py) -- the norm exactly on dyadic gradients over every path of its geometry, within the float64 summation
bound on random ones, non-finite values, repeatability, counters, the partials it writes -- then utils.GradClipper inside
the fused step (Adam, SGD, the deferred optimizer range, a captured graph, two shards) and tools/train.py as a child process."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _cases, _clip_ref as K
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

PAD = 8                      # guard elements on each side of a device array (a multiple of 4: the base stays 16-byte aligned)
POISON = np.float32(-12345.678)
CAP = 4 * 256 * 4096         # elements of an aligned arena that fill the capped grid exactly once
SENTINEL = -7.0              # a sum of squares is never negative


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """Bit equality, a NaN matching any NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


class Guarded:
    """A device float32 array of n elements `off` elements behind a 16-byte boundary, with PAD poisoned elements on both sides."""

    def __init__(self, values, off):
        values = np.ascontiguousarray(values, np.float32)
        self.n, self.lo = values.size, PAD + off
        host = np.full(self.lo + self.n + PAD, POISON, np.float32)
        host[self.lo:self.lo + self.n] = values
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    def put(self, values):
        self.buf[self.lo:self.lo + self.n].copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32)))

    def get(self):
        host = self.buf.cpu().numpy()
        guards = np.concatenate([host[:self.lo], host[self.lo + self.n:]])
        assert (guards == POISON).all(), 'a word outside the arena was written'
        return host[self.lo:self.lo + self.n].copy()


class Op:
    """One fpd_grad_clip_t over a Guarded arena with its own scratch (pre-filled with SENTINEL), result pair and counters."""

    def __init__(self, values, off=0, counters=True):
        from fpd_amd import runtime as R
        self.R, self.lib = R, R.lib()
        self.g = Guarded(values, off)
        self.partial = torch.full((4096 + PAD,), SENTINEL, dtype=torch.float64, device='cuda')
        self.out = torch.full((2 + PAD,), float(POISON), dtype=torch.float32, device='cuda')
        self.counters = torch.zeros(3 + PAD, dtype=torch.int64, device='cuda') if counters else None
        a = self.a = R.GradClipT()
        a.n, a.grad = self.g.n, (self.g.ptr() if self.g.n else None)
        a.partial, a.partial_bytes = self.partial.data_ptr(), 8 * 4096
        a.out, a.counters = self.out.data_ptr(), (self.counters.data_ptr() if counters else None)

    def geometry(self, max_norm=1.0):
        self.a.max_norm = max_norm
        blocks, vec = C.c_int32(), C.c_int64()
        self.R.check(self.lib.fpd_grad_clip_geometry(self.a, blocks, vec), 'fpd_grad_clip_geometry')
        return blocks.value, vec.value

    def run(self, max_norm):
        """One call; returns (norm, coef) as float32 and checks that nothing behind `out` and the counters was written."""
        self.a.max_norm = max_norm
        self.R.check(self.lib.fpd_grad_clip(self.a, self.R.current_stream()), 'fpd_grad_clip')
        torch.cuda.synchronize()
        out = self.out.cpu().numpy()
        assert (out[2:] == POISON).all() and (self.counters is None or int(self.counters[3:].abs().sum()) == 0)
        return np.float32(out[0]), np.float32(out[1])

    def stats(self):
        return self.counters[:3].tolist()


# ---- the kernels ----

@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('n', [1, 3, 255, 256, 257, 1027, CAP + 7])
def test_norm_of_dyadic_gradients_is_exact_and_the_scale_is_one_float32_product(n, off):
    """g = s * m * 2^-6, m in {0..3}: every partial sum is exact in float64 in any order, so there is no tolerance."""
    g0, m = K.dyadic(n, seed=n + off)
    if n <= 3:
        m[:] = np.arange(1, n + 1)                            # no all-zero arena
        g0 = (m * np.where(np.arange(n) % 2, -1, 1)).astype(np.float32) * np.float32(2.0 ** -6)
    want_norm = K.dyadic_norm(m)
    op = Op(g0, off)
    blocks, vec = op.geometry()
    assert vec == (n - n % 4 if off == 0 else 0)
    if n == CAP + 7:
        assert blocks == 4096 and (vec // 4 > blocks * 256 if off == 0 else n > blocks * 256)     # the grid-stride loop iterates
    # not clipped: max_norm = inf and a max_norm above the norm leave every bit where it was
    for max_norm in (float('inf'), float(want_norm) * 2.0 + 1.0):
        norm, coef = op.run(max_norm)
        assert _bits(norm) == _bits(want_norm), (float(norm), float(want_norm))
        assert coef == np.float32(1.0) and np.array_equal(_bits(op.g.get()), _bits(g0))
    # clipped: the device's own coefficient is the restatement's, and every element is float32(g * coef)
    max_norm = np.float32(want_norm * np.float32(0.37))
    norm, coef = op.run(float(max_norm))
    assert _bits(norm) == _bits(want_norm) and _bits(coef) == _bits(K.coef_of(want_norm, max_norm)) and coef < 1.0
    got = op.g.get()
    assert np.array_equal(_bits(got), _bits(K.scale(g0, coef))), '%d of %d elements differ' % ((_bits(got) != _bits(K.scale(g0, coef))).sum(), n)
    assert op.stats() == [3, 1, 0]


def _random_cases():
    out = []
    for n in (1027, 3287936):
        rng = np.random.RandomState(n % 1000)
        out.append(('normal', n, rng.standard_normal(n).astype(np.float32)))
        out.append(('scales', n, (rng.standard_normal(n) * 10.0 ** rng.uniform(-10, 0, n)).astype(np.float32)))
    return out


def test_norm_of_random_gradients_is_within_the_float64_summation_bound(tmp_path):
    """|norm - r64| <= r64 * (2^-24 + n * 2^-53): one float32 rounding, and the worst case of n float64 additions of
    non-negative terms, halved by the root.  r64 is the correctly rounded float64 root of the fsum of the exact squares."""
    lines, worst = [], 0.0
    for kind, n, g in _random_cases():
        r64 = math.sqrt(K.sumsq(g))
        for off in (0, 1):
            norm, coef = Op(g, off).run(float('inf'))
            bound = r64 * (2.0 ** -24 + n * 2.0 ** -53)
            ratio = abs(float(norm) - r64) / bound
            lines.append('%-7s n=%-8d off=%d  norm=%.9g  r64=%.17g  |diff|/bound=%.4f' % (kind, n, off, norm, r64, ratio))
            worst = max(worst, ratio)
            print(lines[-1])
            assert coef == np.float32(1.0)
            assert abs(float(norm) - r64) <= bound, lines[-1]
    lines.append('worst |norm - r64| / (r64 * (2^-24 + n * 2^-53)) = %.4f' % worst)
    path = os.environ.get('FPD_CLIP_GPU_PROFILE') or str(tmp_path / 'clip_gpu.txt')       # profiles/clip_gpu.txt is a copy of this file
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def test_large_elements_give_a_finite_norm_and_non_finite_ones_follow_the_restatement():
    n = 1027
    big = np.full(n, 1e30, np.float32) * np.where(np.arange(n) % 3, 1, -1).astype(np.float32)
    op = Op(big)
    norm, coef = op.run(1.0)
    r64 = math.sqrt(K.sumsq(big))
    assert np.isfinite(norm) and abs(float(norm) - r64) <= r64 * (2.0 ** -24 + n * 2.0 ** -53)     # no float32 square is formed
    assert _bits(coef) == _bits(K.coef_of(norm, 1.0)) and 0.0 < coef < 1e-30
    assert np.array_equal(_bits(op.g.get()), _bits(K.scale(big, coef))) and op.stats() == [1, 1, 0]
    base = np.random.RandomState(5).standard_normal(n).astype(np.float32)
    calls, clipped, nonfinite = 1, 1, 0
    for bad in (np.inf, -np.inf, np.nan):
        for max_norm in (1.0, float('inf')):
            g0 = base.copy()
            g0[517] = bad
            op.g.put(g0)
            norm, coef = op.run(max_norm)
            want_norm, want_coef, want = K.clip(g0, max_norm)
            assert _same(norm, want_norm) and _same(coef, want_coef) and _same(op.g.get(), want), (bad, max_norm)
            assert not np.isfinite(want_norm) and (np.isnan(want_coef) or want_coef == 0.0)
            if want_coef == 0.0:                               # torch's zeros: every finite element, and inf * 0 = NaN
                assert np.isnan(want[517]) and (np.delete(want, 517) == 0.0).all()
            else:
                assert np.isnan(want).all()
            # every call here has a non-finite norm; coef == 0 < 1 counts as clipped, a NaN coefficient compares false
            calls, clipped, nonfinite = calls + 1, clipped + int(want_coef == 0.0), nonfinite + 1
            assert op.stats() == [calls, clipped, nonfinite]
    assert op.stats() == [7, 3, 6]


def test_two_launches_give_the_same_bits_and_the_counters_advance_as_specified():
    g = _random_cases()[1][2]
    op = Op(g, 0)
    first = op.run(float('inf'))
    partial = op.partial.cpu().numpy().copy()
    second = op.run(float('inf'))
    assert _bits(first[0]) == _bits(second[0]) and _bits(first[1]) == _bits(second[1])
    assert np.array_equal(op.partial.cpu().numpy().view(np.uint64), partial.view(np.uint64))      # every partial, bit for bit
    assert op.stats() == [2, 0, 0]
    norm, coef = op.run(float(first[0]) * 0.5)
    assert coef < 1.0 and op.stats() == [3, 1, 0]
    g2 = op.g.get()
    g2[3] = np.nan
    op.g.put(g2)
    norm, coef = op.run(1.0)
    assert np.isnan(norm) and np.isnan(coef) and op.stats() == [4, 1, 1]
    quiet = Op(g, 1, counters=False)                           # the counters are optional
    assert _bits(quiet.run(float('inf'))[1]) == _bits(np.float32(1.0))


@pytest.mark.parametrize('n,off', [(0, 0), (1, 0), (257, 1), (4099, 0), (CAP + 7, 0)])
def test_partials_written_are_exactly_the_blocks_the_query_reports(n, off):
    g = K.dyadic(n, seed=1)[0] if n else np.zeros(0, np.float32)
    op = Op(g, off)
    blocks, vec = op.geometry()
    assert blocks == {0: 1, 1: 1, 257: 2, 4099: 4, CAP + 7: 4096}[n]
    norm, coef = op.run(float('inf'))
    partial = op.partial.cpu().numpy()
    assert (partial[:blocks] >= 0.0).all() and (partial[blocks:] == SENTINEL).all()
    assert _bits(K.norm_of(partial[:blocks].sum())) == _bits(norm)          # dyadic data: the partials add exactly in any order
    if n == 0:
        assert norm == 0.0 and coef == 1.0                     # legal: norm 0, coef 1


def test_refusals_return_an_error_with_a_message_and_launch_nothing():
    op = Op(K.dyadic(4099)[0], 0)
    R, lib = op.R, op.lib
    keep = {k: getattr(op.a, k) for k in ('n', 'grad', 'partial', 'partial_bytes', 'out', 'counters')}
    cases = [('negative', dict(n=-1)), ('too large', dict(n=1 << 60)), ('null', dict(grad=None)), ('null', dict(out=None)),
             ('null', dict(partial=None)), ('too small', dict(partial_bytes=8 * 17 - 1)), ('misaligned', dict(partial=keep['partial'] + 4)),
             ('max_norm', dict(max_norm=0.0)), ('max_norm', dict(max_norm=-1.0)), ('max_norm', dict(max_norm=float('nan'))),
             ('overlaps', dict(out=keep['grad'] + 4 * 4098)), ('overlaps', dict(counters=keep['grad'])),
             ('overlaps', dict(partial=keep['grad'] + 16)), ('overlaps', dict(out=keep['partial'] + 8)),
             ('overlaps', dict(counters=keep['partial'] + 8 * 4095)), ('overlaps', dict(counters=keep['out'] - 16))]
    for word, kw in cases:
        op.a.max_norm = 1.0
        for k, v in keep.items():
            setattr(op.a, k, v)
        for k, v in kw.items():
            setattr(op.a, k, v)
        rc = lib.fpd_grad_clip(op.a, R.current_stream())
        assert rc != 0 and word in lib.fpd_last_error().decode(), (word, kw, rc, lib.fpd_last_error())
    torch.cuda.synchronize()
    for k, v in keep.items():
        setattr(op.a, k, v)
    assert op.stats() == [0, 0, 0] and (op.partial.cpu().numpy() == SENTINEL).all() and (op.out.cpu().numpy() == POISON).all()
    assert np.array_equal(_bits(op.g.get()), _bits(K.dyadic(4099)[0]))
    assert op.run(1e-3)[1] < 1.0 and op.stats() == [1, 1, 0]           # the unmutated arguments are served


# ---- the fused step ----

HP = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
STEPS = 4
_identity = lambda flat, buckets=None: (lambda: None)      # stands in for the all-reduce hook: the optimizer range is deferred


def _models():
    from tests.test_model_gpu import build_models
    return build_models('tiny')


def _make_step(kind, max_norm, **kw):
    from fpd_amd import executor as EX
    from fpd_amd.lib.utils.utils import FusedSGD, GradClipper
    c, gold, student, teacher = _models()
    opt = FusedSGD(student, **HP) if kind == 'sgd' else None
    clip = GradClipper(student, max_norm) if max_norm is not None else None
    if opt is not None:
        kw['sgd'] = opt
    if clip is not None:
        kw['clip'] = clip
    step = EX.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, c['batch'],
                           c['image'][1], c['image'][0], alpha=0.5, **kw)
    return student, step, opt, clip


def _state(student, step, opt):
    torch.cuda.synchronize()
    A = student.device_state().A
    out = {n: A.tensor(n).detach().cpu().clone() for n in ('param', 'rstat', 'nbt', 'grad')}
    out['losses'] = step.student.A.tensor('losses')[:2].cpu().clone()
    if opt is None:
        out['m'], out['v'] = step.m.cpu().clone(), step.v.cpu().clone()
    elif opt.buf is not None:
        out['buf'] = opt.buf.cpu().clone()
    out['step'] = int(step.step_dev)
    return out


def _run_steps(student, step, opt, clip, first=0, last=STEPS):
    states = []
    for k in range(first, last):
        step.set_batch(*_cases.batch('tiny', k))
        step.step()
        st = _state(student, step, opt)
        if clip is not None:
            st['clip_out'] = clip.out.cpu().clone()
            st['clip_counters'] = clip.counters.cpu().clone()
        states.append(st)
    return states


@functools.lru_cache(maxsize=None)
def _trajectory(kind, max_norm):
    """Four eager steps on four batches from the golden initial state; max_norm None = the step of before (clip=None)."""
    student, step, opt, clip = _make_step(kind, max_norm)
    start = student.device_state().A.tensor('param').detach().cpu().clone()
    states = _run_steps(student, step, opt, clip)
    b, e = step.student.rng['adam']
    return dict(states=states, start=start, launches=step.launches_per_step(), ops=len(step.student.plan),
                adam_ops=[step.student.plan.op_type(k) for k in range(b, e)])


def _same_state(a, b, label, skip=()):
    assert sorted(k for k in a if k not in skip) == sorted(k for k in b if k not in skip)
    for k in a:
        if k in skip:
            continue
        same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]
        assert same, '%s: %s differs' % (label, k)


def _norm64_over_views(student, grad):
    """float64 L2 norm over the per-parameter views of a (host) flat gradient: what clip_grad_norm_ sees.  Alignment gaps of the
    arena are NOT part of it, so a device norm that agrees with it shows the gaps hold zeros."""
    from fpd_amd.lib.utils.utils import FusedAdam
    views = FusedAdam(student)._views(grad)
    assert sum(v.numel() for v in views) <= grad.numel()
    return math.sqrt(math.fsum(float((v.double() ** 2).sum()) for v in views)), sum(v.numel() for v in views)


CLIP_SKIP = ('clip_out', 'clip_counters')


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_fused_step_that_does_not_clip_trains_the_same_bits_with_one_more_launch(kind):
    from fpd_amd import runtime as R
    plain = _trajectory(kind, None)
    opt_op = R.OP_SGD if kind == 'sgd' else R.OP_ADAM
    assert plain['adam_ops'] == [opt_op] and plain['launches']['student_adam'] == 1         # clip=None: the plan of before
    observed = max(float(s['clip_out'][0]) for s in _trajectory(kind, float('inf'))['states'])
    for max_norm in (float('inf'), 1000.0 * observed):
        t = _trajectory(kind, max_norm)
        assert t['ops'] == plain['ops'] + 1 and t['adam_ops'] == [R.OP_GRAD_CLIP, opt_op]   # the FIRST op of the optimizer's range
        assert t['launches']['student_adam'] == 2 and t['launches']['total'] == plain['launches']['total'] + 1
        assert all(t['launches'][k] == v for k, v in plain['launches'].items() if k not in ('student_adam', 'total'))
        for k in range(STEPS):
            _same_state(t['states'][k], plain['states'][k], '%s max_norm %g step %d' % (kind, max_norm, k), skip=CLIP_SKIP)
            assert float(t['states'][k]['clip_out'][1]) == 1.0 and t['states'][k]['clip_counters'].tolist() == [k + 1, 0, 0]
        assert 0.0 < observed < float('inf')


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_fused_step_that_clips_scales_the_gradient_and_the_optimizer_sees_the_scaled_one(kind):
    from fpd_amd import runtime as R
    plain = _trajectory(kind, None)
    grad_plain = plain['states'][0]['grad']
    r64, covered = _norm64_over_views(_models()[2], grad_plain)
    student, step, opt, clip = _make_step(kind, float(np.float32(0.5 * r64)))
    n = student.table.sizes['param']
    assert covered <= n == grad_plain.numel()                   # (this model has no alignment gaps; the 17-joint test below has)
    start = student.device_state().A.tensor('param').detach().clone()
    assert torch.equal(start.cpu(), plain['start'])
    st = _run_steps(student, step, opt, clip, 0, 1)[0]
    norm, coef = (np.float32(v) for v in st['clip_out'].numpy())
    print('%s: device norm %.9g, float64 norm over the views %.17g, coef %.9g' % (kind, norm, r64, coef))
    assert abs(float(norm) - r64) <= r64 * (2.0 ** -24 + n * 2.0 ** -53)
    assert _bits(coef) == _bits(K.coef_of(norm, clip.max_norm)) and coef < 1.0 and st['clip_counters'].tolist() == [1, 1, 0]
    want_grad = K.scale(grad_plain.numpy(), coef)
    assert np.array_equal(_bits(st['grad'].numpy()), _bits(want_grad))
    assert torch.equal(st['losses'], plain['states'][0]['losses']) and torch.equal(st['rstat'], plain['states'][0]['rstat'])
    # the optimizer launch alone, on the scaled gradient from the same start state
    dev = start.device
    g = torch.from_numpy(want_grad).to(dev)
    lr_dev, step_dev = step.lr_dev.clone(), torch.zeros(1, dtype=torch.int64, device=dev)
    if kind == 'sgd':
        a = R.SgdT.from_buffer_copy(step._sgd_args)
        buf = torch.zeros_like(start)
        a.param, a.grad, a.buf, a.lr_dev, a.step_dev = start.data_ptr(), g.data_ptr(), buf.data_ptr(), lr_dev.data_ptr(), step_dev.data_ptr()
        R.check(R.lib().fpd_sgd(a, R.current_stream()), 'fpd_sgd')
        torch.cuda.synchronize()
        assert torch.equal(buf.cpu(), st['buf'])
    else:
        a = R.AdamT.from_buffer_copy(step._adam_args)
        m, v = torch.zeros_like(start), torch.zeros_like(start)
        a.param, a.grad, a.m, a.v, a.lr_dev, a.step_dev = start.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), lr_dev.data_ptr(), step_dev.data_ptr()
        R.check(R.lib().fpd_adam(a, R.current_stream()), 'fpd_adam')
        torch.cuda.synchronize()
        assert torch.equal(m.cpu(), st['m']) and torch.equal(v.cpu(), st['v'])
    assert torch.equal(start.cpu(), st['param']) and not torch.equal(st['param'], plain['states'][0]['param'])


def test_alignment_gaps_of_the_arena_hold_zeros_when_the_op_runs():
    """17 joints: the score biases and weights are no multiple of 4 elements, so the arena has alignment gaps, and the norm is
    taken over [0, n), gaps included.  The gradient arena is filled with a stale value first: the backward's memset covers
    the gaps, nothing writes them afterwards, and the device norm agrees with the float64 norm over the per-parameter views."""
    from fpd_amd import executor as EX
    from fpd_amd.lib.models import hourglass
    from fpd_amd.lib.utils.utils import FusedAdam, GradClipper
    from oracle import fpd_ref
    from tests.test_model_gpu import make_cfg
    torch.manual_seed(0)
    student = hourglass.get_pose_net(make_cfg(32, 2, 17), is_train=True).cuda()
    teacher = hourglass.get_pose_net(make_cfg(32, 2, 17), is_train=False).cuda()
    clip = GradClipper(student, float('inf'))
    step = EX.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, 2, 128, 128, alpha=0.5, clip=clip)
    table, grad = student.table, student.device_state().A.tensor('grad')
    n = table.sizes['param']
    gap = np.ones(n, bool)
    for key in table.trainable_keys():
        gap[table[key].off:table[key].off + table[key].numel] = False
    assert 0 < gap.sum() < n and grad.numel() == n
    grad.fill_(3.0)
    step.set_batch(*fpd_ref.synth_batch(100, 2, 17, (128, 128), (32, 32)))
    step.step()
    torch.cuda.synchronize()
    g = grad.cpu()
    assert (g.numpy()[gap] == 0.0).all() and (g.numpy()[~gap] != 0.0).any()
    views = FusedAdam(student)._views(g)
    assert sum(v.numel() for v in views) == n - gap.sum()
    r64 = math.sqrt(math.fsum(float((v.double() ** 2).sum()) for v in views))
    assert r64 > 0.0 and abs(clip.norm() - r64) <= r64 * (2.0 ** -24 + n * 2.0 ** -53), (clip.norm(), r64)
    assert clip.coef() == 1.0 and clip.stats() == {'calls': 1, 'clipped': 0, 'nonfinite': 0}


@functools.lru_cache(maxsize=None)
def _clipping_max_norm(kind):
    """Half the first step's gradient norm, from the measuring run."""
    return float(np.float32(0.5) * np.float32(_trajectory(kind, float('inf'))['states'][0]['clip_out'][0]))


def test_deferred_optimizer_range_clips_exactly_once_per_update():
    """allreduce= given (the identity hook): the optimizer range of step k runs at the start of step k + 1, the last one in
    flush().  Same bits as the eager clipped run, one call per update."""
    max_norm = _clipping_max_norm('adam')
    eager = _trajectory('adam', max_norm)['states']
    student, step, opt, clip = _make_step('adam', max_norm)
    for k in range(STEPS):
        step.set_batch(*_cases.batch('tiny', k))
        step.teacher_async(_cases.batch('tiny', k)[0])
        step.student_step(_identity)
        assert clip.stats()['calls'] == k                                         # step k's range is still pending
    step.flush()
    step.flush()                                                                  # nothing is pending any more: no second call
    st = _state(student, step, opt)
    _same_state(st, eager[-1], 'deferred', skip=CLIP_SKIP)
    assert clip.stats() == {'calls': STEPS, 'clipped': int(eager[-1]['clip_counters'][1]), 'nonfinite': 0}
    assert torch.equal(clip.out.cpu(), eager[-1]['clip_out']) and clip.stats()['clipped'] >= 1
    assert clip.norm() == float(eager[-1]['clip_out'][0]) and clip.coef() == float(eager[-1]['clip_out'][1])


def test_two_fresh_clipped_runs_are_bit_identical_and_graph_replay_matches_the_eager_run():
    max_norm = _clipping_max_norm('adam')
    eager = _trajectory('adam', max_norm)['states']
    assert int(eager[-1]['clip_counters'][1]) >= 1 and not torch.equal(eager[-1]['param'], _trajectory('adam', None)['states'][-1]['param'])
    student, step, opt, clip = _make_step('adam', max_norm)                       # (e) a second fresh run, three steps
    again = _run_steps(student, step, opt, clip, 0, 3)
    for k in range(3):
        _same_state(again[k], eager[k], 'fresh run, step %d' % k)
    student, step, opt, clip = _make_step('adam', max_norm)                       # (d) one eager step, then every phase as a hipGraph
    states = _run_steps(student, step, opt, clip, 0, 1)
    step.enable_graphs()
    states += _run_steps(student, step, opt, clip, 1, STEPS)
    for k in range(STEPS):
        _same_state(states[k], eager[k], 'graph replay, step %d' % k)


def test_step_cache_keys_on_the_clipper_and_its_max_norm_and_a_foreign_clipper_is_refused():
    from fpd_amd import executor as EX, runtime as R
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.utils.utils import FusedAdam, GradClipper
    c, gold, student, teacher = _models()
    opt = FusedAdam(student, lr=1e-3)
    shape = _cases.batch('tiny', 0)[0].shape
    clip = GradClipper(student, 1.0)
    plain = F.fused_step_for(student, teacher, opt, shape, 0.5)
    with_clip = F.fused_step_for(student, teacher, opt, shape, 0.5, clip=clip)
    assert plain is not with_clip and plain.clip is None and with_clip.clip is clip
    assert F.fused_step_for(student, teacher, opt, shape, 0.5, clip=clip) is with_clip and F.fused_step_for(student, teacher, opt, shape, 0.5) is plain
    assert F.fused_step_for(student, teacher, opt, shape, 0.5, clip=GradClipper(student, 1.0)) is not with_clip
    clip.max_norm = 2.0                                       # the value lives in the recorded op: a new step
    changed = F.fused_step_for(student, teacher, opt, shape, 0.5, clip=clip)
    assert changed is not with_clip and changed._clip_args.max_norm == 2.0 and with_clip._clip_args.max_norm == 1.0
    _, _, other, _ = _models()
    with pytest.raises(R.FpdError, match='another model'):
        EX.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, c['batch'], c['image'][1],
                        c['image'][0], alpha=0.5, clip=GradClipper(other, 1.0))


def test_module_api_path_clips_between_backward_and_step():
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.utils.utils import FusedAdam, GradClipper
    c, gold, student, teacher = _models()
    opt, crit = FusedAdam(student, lr=1e-3), JointsMSELoss(True).cuda()
    clip = GradClipper(student, 1e-3)
    x, tg, tw = (t.cuda() for t in _cases.batch('tiny', 0))
    student.train()
    opt.zero_grad()
    sum(crit(o, tg, tw) for o in student(x)).backward()
    flat = student.device_state().A.tensor('grad')
    before = flat.cpu().numpy().copy()
    norm_dev = clip()                                         # a device tensor: nothing waited
    assert torch.is_tensor(norm_dev) and norm_dev.is_cuda
    r64 = math.sqrt(K.sumsq(before))
    assert abs(clip.norm() - r64) <= r64 * (2.0 ** -24 + before.size * 2.0 ** -53) and float(norm_dev) == clip.norm()
    assert _bits(np.float32(clip.coef())) == _bits(K.coef_of(np.float32(clip.norm()), 1e-3)) and clip.coef() < 1.0
    assert np.array_equal(_bits(flat.cpu().numpy()), _bits(K.scale(before, np.float32(clip.coef()))))
    opt.step()
    assert clip.stats() == {'calls': 1, 'clipped': 1, 'nonfinite': 0}


# ---- two shards ----

def test_two_shards_on_one_gpu_compute_the_same_norm_and_keep_bit_equal_parameters():
    """The arrangement of tests/test_dist_gpu.py: two replicas with world_size = 2, each on its shard, the flat gradients
    summed on the device between the backward and the deferred optimizer range.  The loss kernel folds 1/world into the
    gradient, so both ranks clip the same reduced arena: same norm, same coefficient, no collective added."""
    from fpd_amd import dist as fdist, executor as EX
    from fpd_amd.lib.utils.utils import GradClipper
    from oracle import fpd_ref
    from tests.test_dist_gpu import _Replica
    c = _cases.CONFIGS['tiny']
    max_norm = _clipping_max_norm('adam') * 0.25
    reps, clips = [], []
    for r in range(2):
        _, _, student, teacher = _models()
        clips.append(GradClipper(student, max_norm))
        step = EX.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, 2, c['image'][1],
                               c['image'][0], alpha=0.5, lr=2.5e-4, world_size=2, clip=clips[-1])
        reps.append(_Replica(step, student))
    start = reps[0].model._flat['param'].clone()
    for k in range(3):
        x, tg, tw = fpd_ref.synth_batch(100 + k, 4, c['joints'], c['image'], c['heat'])
        for r, rep in enumerate(reps):
            xs, tgs, tws = fdist.shard([x, tg, tw], r, 2)
            rep.step.set_batch(xs, tgs, tws)
            rep.step.teacher_async(xs)
            rep.step.student_step(rep.hook)
        torch.cuda.synchronize()
        total = reps[0].grad + reps[1].grad
        for rep in reps:
            rep.grad.copy_(total)
            rep.step.flush()
        torch.cuda.synchronize()
        assert torch.equal(clips[0].out, clips[1].out), 'step %d: the ranks disagree on norm / coef' % k
        assert float(clips[0].out[1]) < 1.0                                        # max_norm is below the norm: every update clips
        assert torch.equal(reps[0].model._flat['param'], reps[1].model._flat['param'])
    assert clips[0].stats() == clips[1].stats() == {'calls': 3, 'clipped': 3, 'nonfinite': 0}
    assert not torch.equal(reps[0].model._flat['param'], start)


# ---- tools ----

def _run_train(out_dir, extra, timeout=300):
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'train.py'), '--cfg',
           os.path.join(ROOT, 'experiments', 'fpd_synthetic', 'hg4x128_student.yaml'), '--max-iters', '3',
           'OUTPUT_DIR', str(out_dir), 'MODEL.EXTRA.NUM_FEATURES', '32', 'MODEL.EXTRA.NUM_STACKS', '2', 'MODEL.IMAGE_SIZE', '128,128',
           'MODEL.HEATMAP_SIZE', '32,32', 'TRAIN.BATCH_SIZE_PER_GPU', '4', 'TEST.BATCH_SIZE_PER_GPU', '4', 'DATASET.NUM_SAMPLES', '32',
           'DATASET.NUM_VALID_SAMPLES', '8', 'PRINT_FREQ', '1', 'TRAIN.END_EPOCH', '1', 'MODEL.DTYPE', 'fp32', 'TRAIN.SHUFFLE', 'False',
           'TRAIN.LR', '0.001'] + extra
    return subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=timeout)


def test_tools_train_logs_the_norm_with_the_key_and_today_s_line_without_it(tmp_path):
    """tools/train.py for one epoch of three iterations, as child processes: with TRAIN.CLIP_GRAD_NORM the `Epoch:` line
    carries GradNorm and Clipped and a checkpoint is written; without the key the line has neither word.  Nothing further
    is started when a run fails."""
    r = _run_train(tmp_path / 'clip', ['TRAIN.CLIP_GRAD_NORM', '0.05'])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    log = r.stdout + r.stderr
    lines = [l for l in log.splitlines() if 'Epoch: [' in l]
    assert len(lines) == 3 and all('GradNorm ' in l and 'Clipped ' in l for l in lines), lines
    assert 'gradient clipping: global L2 norm 0.05' in log
    last = lines[-1].split('GradNorm ', 1)[1].split()
    assert float(last[0]) > 0.0 and last[1] == 'Clipped' and last[2].split('/')[1] == '3' and 0 <= int(last[2].split('/')[0]) <= 3
    hits = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / 'clip') for f in fs if f == 'checkpoint.pth']
    assert len(hits) == 1
    r2 = _run_train(tmp_path / 'plain', [])
    assert r2.returncode == 0, (r2.stdout[-1500:], r2.stderr[-3000:])
    lines2 = [l for l in (r2.stdout + r2.stderr).splitlines() if 'Epoch: [' in l]
    assert len(lines2) == 3 and not any('GradNorm' in l or 'Clipped' in l for l in lines2)
    assert 'gradient clipping' not in r2.stdout + r2.stderr
    strip = lambda l: l.split('Loss ', 1)[1].split('\t')[0]
    assert strip(lines[0]) == strip(lines2[0])                 # the first iteration's loss does not depend on the update
