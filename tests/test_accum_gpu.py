"""Gradient accumulation on the MI355X: fpd_grad_accum (csrc/grad_accum.hip) against the numpy restatement
(tests/_accum_ref.py) bit for bit in its three modes over every path of its geometry, then FusedFPDStep(accum=k): k = 1 is
the step of before, the plan's shape, windows of identical and of distinct micro-batches, counters, a partial window closed
by flush(), the deferred optimizer range, repeatability and graph replay, core.function.fpd_train and tools/train.py.

Denormals: the kernel's inputs come from tests/_accum_ref.py, which keeps every operand and result out of the subnormal range;
device denormal behaviour is not part of the op's contract."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _accum_ref as K, _cases
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

PAD = 64                     # guard elements on each side of a device array (a multiple of 4: the base stays 16-byte aligned)
POISON = np.float32(-12345.678)


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
        assert guards.size == 2 * PAD + (self.lo - PAD) and (guards == POISON).all(), 'a word outside the arena was written'
        return host[self.lo:self.lo + self.n].copy()


class Op:
    """One fpd_grad_accum_t over two Guarded arenas and a guarded device scale."""

    def __init__(self, grad, acc, off=0):
        from fpd_amd import runtime as R
        self.R, self.lib = R, R.lib()
        self.g, self.a, self.s = Guarded(grad, off), Guarded(acc, off), Guarded(np.ones(1, np.float32), 0)
        t = self.t = R.GradAccumT()
        t.n = self.g.n
        t.grad, t.acc = (self.g.ptr(), self.a.ptr()) if self.g.n else (None, None)
        t.scale_dev = self.s.ptr()

    def geometry(self, mode):
        self.t.mode = mode
        blocks, vec = C.c_int32(), C.c_int64()
        self.R.check(self.lib.fpd_grad_accum_geometry(self.t, blocks, vec), 'fpd_grad_accum_geometry')
        return blocks.value, vec.value

    def run(self, mode, s=None):
        """One call; returns (grad, acc) as the device holds them behind it (the guards of all three arrays are checked)."""
        self.t.mode = mode
        if s is not None:
            self.s.put(np.array([s], np.float32))
        self.R.check(self.lib.fpd_grad_accum(self.t, self.R.current_stream()), 'fpd_grad_accum')
        torch.cuda.synchronize()
        self.s.get()
        return self.g.get(), self.a.get()


def _values(n, seed):
    """(grad, acc) of n elements: normals, and from 1023 elements on every pair of special values in front."""
    g, a = K.normals(n, seed), K.normals(n, seed + 1000)
    if n >= 1023:
        sa, sb = K.special_pairs()
        g[:sa.size], a[:sb.size] = sa, sb
    return g, a


# ---- the kernel ----

@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('n', [0, 1, 3, 5, 255, 256, 257, 1023, 4099, 2 ** 20 + 1, 4 * 2 ** 20 + 23])
def test_three_modes_are_the_restatement_bit_for_bit(n, off):
    g0, a0 = _values(n, n + off)
    op = Op(g0, np.full(n, np.nan, np.float32), off)
    for mode in (K.FIRST, K.ADD, K.FIN):
        blocks, vec = op.geometry(mode)
        assert vec == (n - n % 4 if off == 0 else 0)              # off 0: the vector path and the scalar tail; off 1: element by element
        assert blocks == min(max(-(-max(vec // 4, n - vec) // 256), 1), 4096)
    if n == 2 ** 20 + 1 and off == 1:
        assert blocks * 256 < n                                   # the grid-stride loop iterates
    if n == 4 * 2 ** 20 + 23 and off == 0:
        assert blocks * 256 < vec // 4                            # ... and so does the loop over 16-byte vectors
    # FIRST over an accumulator full of NaN: acc is not read, the copy keeps every bit (NaN payloads, -0)
    for launch in range(2):
        g, a = op.run(K.FIRST)
        assert np.array_equal(K.bits(a), K.bits(g0)) and np.array_equal(K.bits(g), K.bits(g0)), 'FIRST, launch %d' % launch
    # ADD: one float32 addition, grad untouched; the same call on the same operands gives the same bits
    want = K.add(a0, g0)
    assert K.no_subnormal(g0, a0, want)
    seen = []
    for launch in range(2):
        op.a.put(a0)
        g, a = op.run(K.ADD)
        assert K.same(a, want) and np.array_equal(K.bits(g), K.bits(g0)), 'ADD, launch %d' % launch
        seen.append(K.bits(a).copy())
    assert np.array_equal(seen[0], seen[1])
    # FIN: one float32 multiplication by the device scalar, acc untouched
    op.a.put(a0)
    for m in (1, 3, 4):
        s = K.scale_of(m)
        want = K.fin(a0, s)
        assert K.no_subnormal(want)
        seen = []
        for launch in range(2):
            op.g.put(g0)
            g, a = op.run(K.FIN, s)
            assert K.same(g, want) and np.array_equal(K.bits(a), K.bits(a0)), 'FIN m=%d, launch %d' % (m, launch)
            seen.append(K.bits(g).copy())
        assert np.array_equal(seen[0], seen[1])


def test_a_window_on_the_device_is_the_restatements_window():
    n, m = 4099, 5
    grads = [K.normals(n, 50 + i) for i in range(m)]
    op = Op(grads[0], np.full(n, np.nan, np.float32), 0)
    op.run(K.FIRST)
    for g in grads[1:]:
        op.g.put(g)
        op.run(K.ADD)
    g, a = op.run(K.FIN, K.scale_of(m))
    assert np.array_equal(K.bits(g), K.bits(K.window(grads)))


def test_refusals_return_an_error_with_a_message_and_launch_nothing():
    g0, a0 = _values(4099, 7)
    op = Op(g0, a0, 0)
    R, lib = op.R, op.lib
    op.s.put(np.array([0.5], np.float32))
    keep = {k: getattr(op.t, k) for k in ('n', 'grad', 'acc', 'scale_dev')}
    cases = [('negative', dict(n=-1)), ('too large', dict(n=1 << 60)), ('null', dict(grad=None)), ('null', dict(acc=None)),
             ('misaligned', dict(grad=keep['grad'] + 2)), ('misaligned', dict(acc=keep['acc'] + 1)),
             ('misaligned', dict(scale_dev=keep['scale_dev'] + 2)),
             ('overlaps', dict(acc=keep['grad'])), ('overlaps', dict(acc=keep['grad'] + 4 * 4098)), ('overlaps', dict(grad=keep['acc'] + 16)),
             ('overlaps', dict(scale_dev=keep['grad'] + 4 * 100)), ('overlaps', dict(scale_dev=keep['acc'])),
             ('mode', dict(mode=3)), ('mode', dict(mode=-1)), ('scale_dev', dict(scale_dev=None, mode=K.FIN))]
    for word, kw in cases:
        for mode in ((kw['mode'],) if 'mode' in kw else (K.FIRST, K.ADD, K.FIN)):
            for k, v in keep.items():
                setattr(op.t, k, v)
            for k, v in kw.items():
                setattr(op.t, k, v)
            op.t.mode = mode
            rc = lib.fpd_grad_accum(op.t, R.current_stream())
            assert rc < 0 and word in lib.fpd_last_error().decode(), (word, kw, mode, rc, lib.fpd_last_error())
    torch.cuda.synchronize()
    for k, v in keep.items():
        setattr(op.t, k, v)
    assert np.array_equal(K.bits(op.g.get()), K.bits(g0)) and np.array_equal(K.bits(op.a.get()), K.bits(a0))
    assert op.s.get()[0] == np.float32(0.5)
    g, a = op.run(K.FIN)                                          # the unmutated arguments are served
    assert K.same(g, K.fin(a0, 0.5))


# ---- the fused step ----

HP = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
STAT_KEYS = ('rstat', 'nbt', 'ema_rstat', 'ema_nbt')      # the BatchNorm running statistics: they advance per micro-batch


def _models():
    from tests.test_model_gpu import build_models
    return build_models('tiny')


class Run:
    """A FusedFPDStep on the 'tiny' case from the golden initial state.  kind 'adam' | 'sgd'; clip: a max_norm or None;
    ema: a ModelEma of the student or none; accum and any further keyword go to the step."""

    def __init__(self, kind='adam', clip=None, ema=False, **kw):
        from fpd_amd import executor as EX
        from fpd_amd.lib.utils.utils import FusedSGD, GradClipper, ModelEma
        c, gold, self.student, teacher = _models()
        self.opt = FusedSGD(self.student, **HP) if kind == 'sgd' else None
        self.clip = GradClipper(self.student, clip) if clip is not None else None
        self.ema = ModelEma(self.student, decay=0.9, warmup=False) if ema else None
        if self.opt is not None:
            kw['sgd'] = self.opt
        self.step = EX.FusedFPDStep(self.student.device_state(), self.student.cfg_hg, teacher.device_state(), teacher.cfg_hg,
                                    c['batch'], c['image'][1], c['image'][0], alpha=0.5, clip=self.clip, ema=self.ema, **kw)
        self.A = self.student.device_state().A

    def micro(self, batch, allreduce=None):
        b = _cases.batch('tiny', batch)
        self.step.set_batch(*b)
        self.step.teacher_async(b[0])
        self.step.student_step(allreduce)

    def state(self):
        torch.cuda.synchronize()
        out = {n: self.A.tensor(n).detach().cpu().clone() for n in ('param', 'rstat', 'nbt', 'grad')}
        out['losses'] = self.step.student.A.tensor('losses')[:2].cpu().clone()
        if self.opt is None:
            out['m'], out['v'] = self.step.m.cpu().clone(), self.step.v.cpu().clone()
        elif self.opt.buf is not None:
            out['buf'] = self.opt.buf.cpu().clone()
        out['step'] = int(self.step.step_dev)
        if self.ema is not None:
            for n in ('param', 'rstat', 'nbt'):
                out['ema_' + n] = self.ema.flat[n].cpu().clone()
            out['ema_updates'] = self.ema.updates
        if self.clip is not None:
            out['clip_out'] = self.clip.out.cpu().clone()
            out['clip_counters'] = self.clip.counters.cpu().clone()
        return out

    def grad(self):
        torch.cuda.synchronize()
        return self.A.tensor('grad').detach().cpu().numpy().copy()


def _same_state(a, b, label, skip=()):
    assert sorted(k for k in a if k not in skip) == sorted(k for k in b if k not in skip)
    for k in a:
        if k in skip:
            continue
        same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]
        assert same, '%s: %s differs' % (label, k)


def _nbt_advanced(now, before, by):
    """Every num_batches_tracked counter of the arena moved by `by` (the arena keeps each counter on a 16-byte slot, so every
    second word is a gap that stays 0)."""
    d = (now.cpu() - before.cpu())
    used = d != 0
    return bool(used.any()) and int(used.sum()) * 2 >= d.numel() - 4 and bool((d[used] == by).all())


def _shape(run):
    s = run.step.student
    b, e = s.rng['adam']
    return dict(ops=len(s.plan), rng=dict(s.rng), launches=run.step.launches_per_step(),
                adam_ops=[s.plan.op_type(k) for k in range(b, e)])


def test_accum_one_is_the_step_of_before():
    """accum=1 and accum=None (and no keyword at all): the same plan, ranges and launch count, no accumulator, and a 4-step
    trajectory that is bit-equal in everything."""
    runs = [Run(), Run(accum=None), Run(accum=1)]
    shapes = [_shape(r) for r in runs]
    assert shapes[0] == shapes[1] == shapes[2]
    assert sorted(shapes[0]['rng']) == ['adam', 'bwd', 'fwd', 'mid', 'mid1', 'prep'] and 'student_acc' not in shapes[0]['launches']
    for r in runs:
        assert r.step.accum == 1 and not hasattr(r.step, 'acc') and not hasattr(r.step, 'scale_dev')
    for k in range(4):
        states = []
        for r in runs:
            r.micro(k)
            states.append(r.state())
        _same_state(states[1], states[0], 'accum=None, step %d' % k)
        _same_state(states[2], states[0], 'accum=1, step %d' % k)
        assert states[0]['step'] == k + 1
    assert [r.step.updates for r in runs] == [4, 4, 4]


def test_accum_argument_is_validated():
    from fpd_amd import executor as EX, runtime as R
    c, gold, student, teacher = _models()
    for bad in (0, -1, 1025, 2.0, '2', True):
        with pytest.raises(R.FpdError, match='accum'):
            EX.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, c['batch'], c['image'][1],
                            c['image'][0], alpha=0.5, accum=bad)


@pytest.mark.parametrize('kind,clip,ema', [('adam', None, False), ('sgd', None, False), ('adam', 1.0, False), ('adam', 1.0, True)])
def test_plan_gains_three_one_op_ranges_and_the_optimizer_range_keeps_its_contents(kind, clip, ema):
    from fpd_amd import runtime as R
    plain, acc = Run(kind, clip, ema), Run(kind, clip, ema, accum=3)
    sp, sa = _shape(plain), _shape(acc)
    want = ([R.OP_GRAD_CLIP] if clip else []) + [R.OP_SGD if kind == 'sgd' else R.OP_ADAM] + ([R.OP_EMA] if ema else [])
    assert sp['adam_ops'] == sa['adam_ops'] == want
    assert sa['ops'] == sp['ops'] + 3 and all(sa['rng'][k] == v for k, v in sp['rng'].items())
    s = acc.step.student
    for name in ('acc0', 'acc', 'accfin'):
        b, e = s.rng[name]
        assert e - b == 1 and s.plan.op_type(b) == R.OP_GRAD_ACCUM and b >= sp['ops']        # behind everything recorded before
    assert acc.step.acc.numel() == acc.step.n_param and acc.step.acc.dtype == torch.float32 and acc.step.scale_dev.numel() == 1
    assert sa['launches']['student_acc'] == 1 and sa['launches']['student_accfin'] == 1
    assert all(sa['launches'][k] == v for k, v in sp['launches'].items() if k != 'total')
    assert acc.step.grad_buckets() == [(0, acc.step.n_param, None)]


@functools.lru_cache(maxsize=None)
def _plain_updates(kind, extras):
    """Three k = 1 updates on batches 0, 1, 2; extras: clip (a max_norm that clips) and EMA on, or neither."""
    r = Run(kind, _clipping_max_norm(kind) if extras else None, extras)
    out = []
    for b in range(3):
        r.micro(b)
        out.append(r.state())
    return out


@functools.lru_cache(maxsize=None)
def _clipping_max_norm(kind):
    """Half the first update's gradient norm, from a measuring run."""
    r = Run(kind, float('inf'))
    r.micro(0)
    torch.cuda.synchronize()
    return float(np.float32(0.5) * np.float32(r.clip.norm()))


@pytest.mark.parametrize('extras', [False, True])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
@pytest.mark.parametrize('k', [2, 4])
def test_window_of_identical_micro_batches_is_one_plain_step_bit_for_bit(k, kind, extras):
    """((g + g) + g) + g = 4 g and 4 g * 0.25 = g are exact, so the window's mean is the micro-batch's gradient and everything
    behind it is the k = 1 update.  The BatchNorm running statistics are exempt: they advance once per micro-batch."""
    plain = _plain_updates(kind, extras)
    r = Run(kind, _clipping_max_norm(kind) if extras else None, extras, accum=k)
    nbt0 = r.A.tensor('nbt').cpu().clone()
    for u in range(3):
        for j in range(k):
            r.micro(u)
            if j < k - 1:
                assert r.step.updates == u
        st = r.state()
        _same_state(st, plain[u], '%s k=%d update %d' % (kind, k, u), skip=STAT_KEYS)
        assert _nbt_advanced(st['nbt'], nbt0, k * (u + 1)) and _nbt_advanced(plain[u]['nbt'], nbt0, u + 1)
        assert st['step'] == u + 1
        if extras:
            assert st['ema_updates'] == u + 1 and int(st['clip_counters'][0]) == u + 1
    if extras:
        assert int(st['clip_counters'][1]) >= 1                     # the max_norm did clip


def test_window_of_distinct_micro_batches_is_the_restatement_and_counters_advance_once_per_window():
    """k = 3: the per-micro-batch gradients g_i come from a twin k = 1 step at lr = 0 (same weights throughout, so the same
    gradients).  The clipper only measures (max_norm inf) and the EMA reads: neither writes the gradient arena."""
    k = 3
    twin = Run(lr=0.0)
    start = twin.A.tensor('param').detach().cpu().clone()
    g = []
    for b in range(k):
        twin.micro(b)
        g.append(twin.grad())
    assert torch.equal(twin.A.tensor('param').cpu(), start) and int(twin.step.step_dev) == k
    assert not np.array_equal(g[0], g[1]) and not np.array_equal(g[1], g[2])
    r = Run(clip=float('inf'), ema=True, accum=k)
    nbt0 = r.A.tensor('nbt').cpu().clone()
    r.micro(0)
    assert np.array_equal(K.bits(r.grad()), K.bits(g[0]))                   # 'acc0' reads the arena and leaves it
    assert int(r.step.step_dev) == 0 and r.ema.updates == 0 and r.clip.stats()['calls'] == 0
    r.micro(1)
    assert np.array_equal(K.bits(r.grad()), K.bits(g[1])) and int(r.step.step_dev) == 0
    r.micro(2)
    want = K.window(g)
    got = r.grad()
    assert np.array_equal(K.bits(got), K.bits(want)), '%d of %d elements differ' % ((K.bits(got) != K.bits(want)).sum(), want.size)
    assert not np.array_equal(K.bits(want), K.bits(g[2]))
    assert int(r.step.step_dev) == 1 and r.ema.updates == 1 and r.clip.stats() == {'calls': 1, 'clipped': 0, 'nonfinite': 0}
    assert _nbt_advanced(r.A.tensor('nbt'), nbt0, k) and r.step.updates == 1
    assert not torch.equal(r.A.tensor('param').cpu(), start)
    for b in range(3, 6):                                                    # a second window: every counter by one more
        r.micro(b)
    torch.cuda.synchronize()
    assert int(r.step.step_dev) == 2 and r.ema.updates == 2 and r.clip.stats()['calls'] == 2 and r.step.updates == 2
    assert _nbt_advanced(r.A.tensor('nbt'), nbt0, 2 * k)


def test_flush_closes_a_partial_window_and_the_next_one_starts_afresh():
    twin = Run(lr=0.0)
    g = []
    for b in range(2):
        twin.micro(b)
        g.append(twin.grad())
    r = Run(accum=3)
    r.micro(0)
    r.micro(1)
    assert int(r.step.step_dev) == 0
    r.step.flush()
    want = K.fin(K.add(g[0], g[1]), np.float32(0.5))
    assert np.array_equal(K.bits(r.grad()), K.bits(want)) and int(r.step.step_dev) == 1 and r.step.updates == 1
    assert float(r.step.scale_dev) == 0.5
    r.step.flush()                                                           # nothing is open or pending: no second update
    assert int(r.step.step_dev) == 1 and r.step.updates == 1
    r.step.acc.fill_(float('nan'))                                           # the next window starts with FIRST: acc is not read
    for b in range(2, 5):
        r.micro(b)
    st = r.state()
    assert st['step'] == 2 and float(r.step.scale_dev) == float(K.scale_of(3))
    for n in ('grad', 'param', 'm', 'v'):
        assert not torch.isnan(st[n]).any(), n
    assert not torch.isnan(r.step.acc).any()


def test_deferred_optimizer_range_runs_once_per_window_behind_one_whole_arena_bucket():
    """allreduce= given (a recording stand-in): the hook is called once per window with one bucket, sees the window's mean
    gradient, and the optimizer range of window w runs at the start of the next student_step, the last one in flush()."""
    k = 2
    eager = Run(accum=k)
    means, states = [], []
    for w in range(2):
        for j in range(k):
            eager.micro(k * w + j)
        means.append(eager.grad())
        states.append(eager.state())
    r = Run(accum=k)
    n = r.step.n_param
    calls, ran = [], []

    def hook(flat, buckets=None):
        calls.append((buckets, flat.clone()))                                # stream-ordered behind 'accfin'
        return lambda: ran.append(len(calls))
    for w in range(2):
        for j in range(k):
            r.micro(k * w + j, hook)
            torch.cuda.synchronize()
            assert len(calls) == (w + 1 if j == k - 1 else w)
            assert int(r.step.step_dev) == w          # window w - 1's range ran at this window's first micro-step, window w's is pending
        assert int(r.step.step_dev) == w and ran == list(range(1, w + 1))
    r.step.flush()
    r.step.flush()
    assert len(calls) == 2 and ran == [1, 2] and int(r.step.step_dev) == 2 and r.step.updates == 2
    for w, (buckets, flat) in enumerate(calls):
        assert buckets == [(0, n, None)]
        assert np.array_equal(K.bits(flat.cpu().numpy()), K.bits(means[w])), 'window %d' % w
    _same_state(r.state(), states[-1], 'deferred')


def test_two_fresh_runs_are_bit_identical_and_graph_replay_matches_the_eager_run():
    k = 2

    def windows(run, first, last):
        out = []
        for b in range(k * first, k * last):
            run.micro(b)
            out.append(run.state())
        return out
    eager = windows(Run(kind='adam', clip=_clipping_max_norm('adam'), ema=True, accum=k), 0, 3)
    again = windows(Run(kind='adam', clip=_clipping_max_norm('adam'), ema=True, accum=k), 0, 3)
    for i, (a, b) in enumerate(zip(again, eager)):
        _same_state(a, b, 'fresh run, micro-step %d' % i)
    assert eager[-1]['step'] == 3 and not torch.equal(eager[-1]['param'], eager[1]['param'])
    r = Run(kind='adam', clip=_clipping_max_norm('adam'), ema=True, accum=k)    # one eager window, then every range as a hipGraph
    states = windows(r, 0, 1)
    r.step.enable_graphs()
    assert all(r.step.student.graphs.get(n) is not None for n in ('acc0', 'acc', 'accfin', 'adam'))
    states += windows(r, 1, 3)
    for i, (a, b) in enumerate(zip(states, eager)):
        _same_state(a, b, 'graph replay, micro-step %d' % i)


# ---- the loop and the tools ----

class AD(dict):
    __getattr__ = dict.__getitem__


class _Loader:
    def __init__(self, n):
        self.b = [_cases.batch('tiny', i) for i in range(n)]

    def __iter__(self):
        for x, t, w in self.b:
            yield x, t, w, {}

    def __len__(self):
        return len(self.b)


def test_fpd_train_closes_the_trailing_window_and_reuses_the_cached_step(caplog):
    """Five batches with accum=2: windows of 2, 2 and 1 -- three updates an epoch; the second epoch gets the same step object."""
    import logging
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.utils.utils import FusedAdam
    c, gold, student, teacher = _models()
    opt, crit = FusedAdam(student, lr=2.5e-4), JointsMSELoss(True).cuda()
    cfg = AD(KD=AD(ALPHA=0.5), PRINT_FREQ=1, DEBUG=AD(DEBUG=False))
    shape = _cases.batch('tiny', 0)[0].shape
    nbt0 = student._flat['nbt'].cpu().clone()
    with caplog.at_level(logging.INFO):
        loss = F.fpd_train(cfg, _Loader(5), student, teacher, crit, crit, opt, 0, '/tmp', '/tmp', None, accum=2)
    step = F.fused_step_for(student, teacher, opt, shape, 0.5, 1, (True, True), accum=2)
    assert step.accum == 2 and int(opt.step_dev) == 3 and step.updates == 3 and step._acc_j == 0 and loss > 0.0
    assert float(step.scale_dev) == 1.0                                        # the trailing window held one micro-batch
    assert _nbt_advanced(student._flat['nbt'], nbt0, 5)
    lines = [rec.getMessage() for rec in caplog.records if 'Epoch: [' in rec.getMessage()]
    assert len(lines) == 5 and [int(l.rsplit('Updates ', 1)[1]) for l in lines] == [0, 1, 1, 2, 2]
    F.fpd_train(cfg, _Loader(5), student, teacher, crit, crit, opt, 1, '/tmp', '/tmp', None, accum=2)
    assert F.fused_step_for(student, teacher, opt, shape, 0.5, 1, (True, True), accum=2) is step
    assert int(opt.step_dev) == 6 and step.updates == 6


def _run_train(out_dir, extra, timeout=300):
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'train.py'), '--cfg',
           os.path.join(ROOT, 'experiments', 'fpd_synthetic', 'hg4x128_student.yaml'), '--max-iters', '3',
           'OUTPUT_DIR', str(out_dir), 'MODEL.EXTRA.NUM_FEATURES', '32', 'MODEL.EXTRA.NUM_STACKS', '2', 'MODEL.IMAGE_SIZE', '128,128',
           'MODEL.HEATMAP_SIZE', '32,32', 'TRAIN.BATCH_SIZE_PER_GPU', '4', 'TEST.BATCH_SIZE_PER_GPU', '4', 'DATASET.NUM_SAMPLES', '32',
           'DATASET.NUM_VALID_SAMPLES', '8', 'PRINT_FREQ', '1', 'TRAIN.END_EPOCH', '1', 'MODEL.DTYPE', 'fp32', 'TRAIN.SHUFFLE', 'False',
           'TRAIN.LR', '0.001'] + extra
    return subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=timeout)


def test_tools_train_logs_the_effective_batch_and_updates_with_the_key_and_today_s_line_without_it(tmp_path):
    """tools/train.py for one epoch of three iterations, as child processes: with TRAIN.ACCUM_STEPS 2 the log names the
    effective batch and the `Epoch:` line carries Updates (windows of 2 and 1); without the key the line has no such word.
    Nothing further is started when a run fails."""
    r = _run_train(tmp_path / 'accum', ['TRAIN.ACCUM_STEPS', '2'])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    log = r.stdout + r.stderr
    assert 'gradient accumulation: 2 micro-batches of 4 per update, effective batch 8' in log
    lines = [l for l in log.splitlines() if 'Epoch: [' in l]
    assert len(lines) == 3 and [int(l.rsplit('Updates ', 1)[1]) for l in lines] == [0, 1, 1], lines
    hits = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / 'accum') for f in fs if f == 'checkpoint.pth']
    assert len(hits) == 1
    r2 = _run_train(tmp_path / 'plain', [])
    assert r2.returncode == 0, (r2.stdout[-1500:], r2.stderr[-3000:])
    log2 = r2.stdout + r2.stderr
    lines2 = [l for l in log2.splitlines() if 'Epoch: [' in l]
    assert len(lines2) == 3 and not any('Updates' in l for l in lines2) and 'gradient accumulation' not in log2
    strip = lambda l: l.split('Loss ', 1)[1].split('\t')[0]
    assert strip(lines[0]) == strip(lines2[0])                 # the first iteration's loss does not depend on the update
