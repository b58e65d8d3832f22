"""The weight average on the MI355X: the flat kernel (csrc/ema.hip) bit for bit against the numpy restatement
(tests/_ema_ref.py) on every path of its geometry, its refusals, utils.ModelEma inside the fused step (Adam, SGD, the
deferred optimizer range, two shards), its `.module`, and tools/train.py / tools/test.py as child processes."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _cases, _ema_ref as E
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

PAD = 8                      # guard elements on each side of a destination (a multiple of 4: the base stays 16-byte aligned)
POISON_F, POISON_I = np.float32(-12345.678), np.int64(-0x0123456789abcdef)


class AD(dict):
    __getattr__ = dict.__getitem__


def _geometry(a):
    from fpd_amd import runtime as R
    blocks, vec = C.c_int32(), (C.c_int64 * R.EMA_MAX_SEG)()
    R.check(R.lib().fpd_ema_geometry(a, blocks, vec), 'fpd_ema_geometry')
    return blocks.value, list(vec)[:a.nseg]


@functools.lru_cache(maxsize=None)
def second_trip_n():
    """The smallest n of an aligned segment for which the launch's grid-stride loop over vectors makes a second trip, from the
    geometry query: the grid stops growing at its cap, and one more vector than the capped grid has threads is the answer."""
    from fpd_amd import runtime as R

    def geo(n):
        a = R.EmaT()
        a.nseg, a.decay = 1, 0.5
        a.seg[0].src, a.seg[0].dst, a.seg[0].n, a.updates_dev = 1 << 44, 1 << 45, n, 1 << 46      # never dereferenced
        b, v = _geometry(a)
        return b, v[0] // 4
    cap, _ = geo(1 << 34)
    n = 4 * (cap * 256 + 1)
    (b1, v1), (b0, v0) = geo(n), geo(n - 4)
    assert b1 == b0 == cap and v1 > cap * 256 >= v0
    return n


class Guarded:
    """A device array of n elements `off` elements behind a 16-byte boundary, with PAD poisoned elements on both sides."""

    def __init__(self, values, off, poison):
        values = np.ascontiguousarray(values)
        self.n, self.lo = values.size, PAD + off
        host = np.full(self.lo + self.n + PAD, poison, values.dtype)
        host[self.lo:self.lo + self.n] = values
        self.poison = poison
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + self.lo * self.buf.element_size()

    def put(self, values):
        self.buf[self.lo:self.lo + self.n].copy_(torch.from_numpy(np.ascontiguousarray(values)))

    def get(self):
        host = self.buf.cpu().numpy()
        guards = np.concatenate([host[:self.lo], host[self.lo + self.n:]])
        assert (guards == self.poison).all(), 'a word outside the range was written'
        return host[self.lo:self.lo + self.n].copy()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _sources(e, k):
    """The source of call k: every element within 5 % of the initial average (so within a factor 2 of it), new for every call."""
    rng = np.random.RandomState(1000 + k)
    return (e * (1.0 + 0.01 * rng.standard_normal(e.size))).astype(np.float32)


def _launch(segs, copy_n, decay, warmup, calls=3):
    """segs: [(n, src_off, dst_off)].  `calls` fpd_ema calls, each on fresh seeded sources.  Asserts bit equality with the
    restatement, untouched guards and sources, the copied integers and the counter; returns (geometry, e0, sources, result)."""
    from fpd_amd import runtime as R
    e0 = [E.seeded(n, seed=10 + s)[0] for s, (n, _, _) in enumerate(segs)]
    xs = [[_sources(e, k) for e in e0] for k in range(calls)]
    dst = [Guarded(e, d_off, POISON_F) for e, (_, _, d_off) in zip(e0, segs)]
    src = [Guarded(e, s_off, POISON_F) for e, (_, s_off, _) in zip(e0, segs)]
    cs = Guarded(np.arange(copy_n, dtype=np.int64) * 3 + 1, 0, POISON_I)
    cd = Guarded(np.zeros(copy_n, np.int64), 0, POISON_I)
    counter = Guarded(np.zeros(1, np.int64), 0, POISON_I)
    a = R.EmaT()
    a.nseg, a.warmup, a.decay = len(segs), int(warmup), decay
    for s, (n, _, _) in enumerate(segs):
        a.seg[s].src, a.seg[s].dst, a.seg[s].n = src[s].ptr(), dst[s].ptr(), n
    if copy_n:
        a.copy_src, a.copy_dst, a.copy_n = cs.ptr(), cd.ptr(), copy_n
    a.updates_dev = counter.ptr()
    geo = _geometry(a)
    for k in range(calls):
        for s in range(len(segs)):
            src[s].put(xs[k][s])
        cs.put(np.arange(copy_n, dtype=np.int64) * 3 + k)
        R.check(R.lib().fpd_ema(a, R.current_stream()), 'fpd_ema')
    torch.cuda.synchronize()
    want, updates = E.run(e0, xs, None, decay, warmup)
    for s in range(len(segs)):
        got = dst[s].get()
        assert np.array_equal(_bits(got), _bits(want[s])), 'segment %d: %d of %d elements differ' % (s, (_bits(got) != _bits(want[s])).sum(), got.size)
        assert np.array_equal(_bits(src[s].get()), _bits(xs[-1][s]))               # the source is only read
    assert np.array_equal(cd.get(), np.arange(copy_n, dtype=np.int64) * 3 + calls - 1) and np.array_equal(cs.get(), cd.get())
    assert int(counter.get()[0]) == calls == updates
    return geo, e0, xs, want


# ---- the kernel ----

@pytest.mark.parametrize('warmup', [False, True])
@pytest.mark.parametrize('n', [1, 3, 4099])
def test_kernel_is_the_restatement_bit_for_bit_over_three_updates(n, warmup):
    (blocks, vec), e0, xs, want = _launch([(n, 0, 0)], 7, 0.9998, warmup)
    assert vec == [n - n % 4] and blocks == max(1, -(-max(n // 4, n % 4, 7) // 256))
    assert not np.array_equal(_bits(want[0]), _bits(e0[0]))                        # the average really moved
    if warmup:                                                                     # ... and by the ramp's weights, not the decay's
        assert not np.array_equal(_bits(want[0]), _bits(E.run(e0, xs, None, 0.9998, False)[0][0]))


def test_kernel_makes_a_second_grid_stride_trip_exactly_where_the_geometry_says():
    n = second_trip_n() + 5
    (blocks, vec), _, _, _ = _launch([(n, 0, 0)], 0, 0.999, True)
    assert vec == [n - n % 4] and vec[0] // 4 > blocks * 256                       # more vectors than threads: the loop iterates


def test_two_segments_of_different_length_unaligned_bases_and_the_copied_integers():
    # two aligned segments in one launch, the grid sized by the longer one
    (blocks, vec), _, _, _ = _launch([(4099, 0, 0), (1031, 0, 0)], 1, 0.9998, True)
    assert vec == [4096, 1028] and blocks == 4
    # src one element off a 16-byte boundary with dst on it, and the reverse: element by element, same bits
    (blocks, vec), _, _, _ = _launch([(4099, 1, 0), (1031, 0, 1)], 7, 0.9998, True)
    assert vec == [0, 0] and blocks == -(-4099 // 256)
    (blocks, vec), _, _, _ = _launch([(4099, 0, 0), (1031, 3, 3), (5, 2, 0), (1, 0, 0)], 0, 0.5, False)      # four segments, mixed
    assert vec == [4096, 0, 0, 0]


def test_decay_zero_lands_on_the_source_and_the_update_is_not_contracted():
    """decay 0: w = 1 and e + (x - e) is x exactly wherever x - e is exact -- sources within a factor 2 of the average
    (Sterbenz), which the seeded pairs are.  The designed triple (tests/_ema_ref.DESIGNED), on which fma(w, x - e, e) and the
    three-rounding form differ, reaches the kernel through decay = 1 - w without warm-up."""
    _, e0, xs, want = _launch([(4099, 0, 0), (37, 1, 0)], 0, 0.0, False, calls=1)
    assert all(np.array_equal(_bits(w), _bits(x)) and not np.array_equal(_bits(x), _bits(e)) for w, x, e in zip(want, xs[0], e0))
    e, x, w = E.DESIGNED
    assert E.weight(5, 1.0 - float(w), False) == w and _bits(E.update(e, x, w)) != _bits(E.update_fused(e, x, w))
    for n, off in ((8, 0), (3, 1)):                                                # the vector path and the element path
        from fpd_amd import runtime as R
        dst, src = Guarded(np.full(n, e, np.float32), 0, POISON_F), Guarded(np.full(n, x, np.float32), off, POISON_F)
        counter = Guarded(np.zeros(1, np.int64), 0, POISON_I)
        a = R.EmaT()
        a.nseg, a.warmup, a.decay = 1, 0, 1.0 - float(w)
        a.seg[0].src, a.seg[0].dst, a.seg[0].n, a.updates_dev = src.ptr(), dst.ptr(), n, counter.ptr()
        R.check(R.lib().fpd_ema(a, R.current_stream()), 'fpd_ema')
        torch.cuda.synchronize()
        assert (_bits(dst.get()) == _bits(E.DESIGNED_UNFUSED)).all()


def test_special_values_follow_the_restatement_and_nan_stays_nan():
    from fpd_amd import runtime as R
    e0, x0 = E.special_values()
    dst, src, counter = Guarded(e0, 0, POISON_F), Guarded(x0, 0, POISON_F), Guarded(np.zeros(1, np.int64), 0, POISON_I)
    a = R.EmaT()
    a.nseg, a.warmup, a.decay = 1, 1, 0.9998
    a.seg[0].src, a.seg[0].dst, a.seg[0].n, a.updates_dev = src.ptr(), dst.ptr(), e0.size, counter.ptr()
    R.check(R.lib().fpd_ema(a, R.current_stream()), 'fpd_ema')
    torch.cuda.synchronize()
    got, want = dst.get(), E.update(e0, x0, E.weight(0, 0.9998, True))
    nan = np.isnan(want)
    assert nan.any() and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def test_every_refusal_returns_an_error_with_a_message_and_launches_nothing():
    from fpd_amd import runtime as R
    lib = R.lib()
    n = 4099
    e0, x0 = E.seeded(n)
    dst = [Guarded(e0, 0, POISON_F), Guarded(e0[:1000], 0, POISON_F)]
    src = [Guarded(x0, 0, POISON_F), Guarded(x0[:1000], 0, POISON_F)]
    cs, cd = Guarded(np.arange(7, dtype=np.int64), 0, POISON_I), Guarded(np.full(7, 5, np.int64), 0, POISON_I)
    counter = Guarded(np.full(1, 11, np.int64), 0, POISON_I)

    def args():
        a = R.EmaT()
        a.nseg, a.warmup, a.decay = 2, 1, 0.9998
        for s in range(2):
            a.seg[s].src, a.seg[s].dst, a.seg[s].n = src[s].ptr(), dst[s].ptr(), dst[s].n
        a.copy_src, a.copy_dst, a.copy_n, a.updates_dev = cs.ptr(), cd.ptr(), 7, counter.ptr()
        return a

    def seg(s, **kw):
        def f(a):
            for k, v in kw.items():
                setattr(a.seg[s], k, v)
        return f

    def top(**kw):
        return lambda a: [setattr(a, k, v) for k, v in kw.items()]
    cases = [('nseg', top(nseg=0)), ('nseg', top(nseg=5)), ('negative', seg(1, n=-1)), ('negative', top(copy_n=-2)),
             ('null', seg(0, src=None)), ('null', seg(1, dst=None)), ('null', top(copy_src=None)), ('null', top(copy_dst=None)),
             ('null', top(updates_dev=None)), ('decay', top(decay=1.0)), ('decay', top(decay=-0.1)), ('decay', top(decay=float('nan'))),
             ('overlaps', seg(0, dst=src[0].ptr())),                               # src == dst
             ('overlaps', seg(0, dst=src[0].ptr() + 4 * (n - 1))),                 # one element of overlap
             ('overlaps', seg(0, dst=src[1].ptr() - 4 * (n - 1))),                 # ... with the other segment's source
             ('overlaps', seg(1, dst=dst[0].ptr() + 16)),                          # two destinations
             ('overlaps', top(updates_dev=dst[0].ptr() + 8)),                      # the counter inside a destination
             ('overlaps', top(copy_dst=src[0].ptr()))]
    for word, mutate in cases:
        a = args()
        mutate(a)
        rc = lib.fpd_ema(a, R.current_stream())
        assert rc != 0 and word in lib.fpd_last_error().decode(), (word, rc, lib.fpd_last_error())
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(d.get()), _bits(e0[:d.n])) for d in dst)       # nothing was launched: no destination moved,
    assert (cd.get() == 5).all() and int(counter.get()[0]) == 11                    # no integer was copied, the counter did not tick
    R.check(lib.fpd_ema(args(), R.current_stream()), 'fpd_ema')                     # the unmutated arguments are served
    torch.cuda.synchronize()
    assert int(counter.get()[0]) == 12 and np.array_equal(cd.get(), np.arange(7))


def test_geometry_query_reports_the_grid_the_launch_uses(tmp_path):
    """A child process with the launch log on (it is read when the library is loaded): the query's blocks against the grid of
    the logged ema_kernel launch, for one block, several blocks, an unaligned segment and the capped grid."""
    log = tmp_path / 'launch.log'
    code = (
        "import ctypes as C, torch\n"
        "from fpd_amd import runtime as R\n"
        "for n, off, m in ((3, 0, 0), (4099, 0, 1031), (4099, 1, 5), (%d, 0, 0)):\n"
        "    src, dst = torch.zeros(n + 8, device='cuda'), torch.zeros(n + 8, device='cuda')\n"
        "    s2, d2, cnt = torch.zeros(m + 4, device='cuda'), torch.zeros(m + 4, device='cuda'), torch.zeros(1, dtype=torch.int64, device='cuda')\n"
        "    a = R.EmaT()\n"
        "    a.nseg, a.decay, a.updates_dev = 2, 0.5, cnt.data_ptr()\n"
        "    a.seg[0].src, a.seg[0].dst, a.seg[0].n = src.data_ptr() + 4 * off, dst.data_ptr(), n\n"
        "    a.seg[1].src, a.seg[1].dst, a.seg[1].n = s2.data_ptr(), d2.data_ptr(), m\n"
        "    b, v = C.c_int32(), (C.c_int64 * 4)()\n"
        "    R.check(R.lib().fpd_ema_geometry(a, b, v)); R.check(R.lib().fpd_ema(a, R.current_stream()))\n"
        "    torch.cuda.synchronize()\n"
        "    print('GEO', b.value, v[0], v[1], int(cnt))\n") % (second_trip_n() + 5)
    env = dict(os.environ, FPD_LAUNCH_LOG=str(log), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    geo = [[int(t) for t in l.split()[1:]] for l in out.stdout.splitlines() if l.startswith('GEO')]
    lines = [l.rstrip('\n').split('\t') for l in open(log)]
    grids = [int(f[1]) for f in lines if f[0] == 'ema_kernel']
    ticks = [int(f[1]) for f in lines if f[0] == 'tick_kernel']
    assert len(geo) == 4 and [g[0] for g in geo] == grids and ticks == [1] * 4 and len(lines) == 8      # two launches a call, nothing else
    assert all(int(f[2]) == 256 for f in lines if f[0] == 'ema_kernel') and all(g[3] == 1 for g in geo)
    assert geo[0][:3] == [1, 0, 0] and geo[1][:3] == [4, 4096, 1028] and geo[2][:3] == [17, 0, 4] and geo[3][1] // 4 > geo[3][0] * 256


# ---- the fused step ----

HP = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
STEPS = 4
_identity = lambda flat, buckets=None: (lambda: None)      # stands in for the all-reduce hook: the optimizer range is deferred


def _models():
    from tests.test_model_gpu import build_models
    return build_models('tiny')


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


def _make_step(kind, with_ema, **ema_kw):
    from fpd_amd import executor as EX
    from fpd_amd.lib.utils.utils import FusedSGD, ModelEma
    c, gold, student, teacher = _models()
    opt = FusedSGD(student, **HP) if kind == 'sgd' else None
    ema = ModelEma(student, **ema_kw) if with_ema else None
    kw = dict(sgd=opt) if opt is not None else {}
    if ema is not None:
        kw['ema'] = ema
    step = EX.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, c['batch'],
                           c['image'][1], c['image'][0], alpha=0.5, **kw)
    return student, step, opt, ema


@functools.lru_cache(maxsize=None)
def _plain_trajectory(kind):
    """The step of before (ema=None) from the golden initial state, four steps on four batches: the state after each."""
    student, step, opt, _ = _make_step(kind, False)
    states = []
    for k in range(STEPS):
        step.set_batch(*_cases.batch('tiny', k))
        step.step()
        states.append(_state(student, step, opt))
    return states, step.launches_per_step(), len(step.student.plan)


def _same_state(a, b, label):
    assert sorted(a) == sorted(b)
    for k in a:
        same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]
        assert same, '%s: %s differs between the step with the average and the step without' % (label, k)


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_fused_step_with_ema_trains_the_same_bits_and_averages_once_per_step(kind):
    from fpd_amd import runtime as R
    plain, plain_launches, plain_ops = _plain_trajectory(kind)
    decay, warmup = 0.9998, True
    student, step, opt, ema = _make_step(kind, True, decay=decay, warmup=warmup)
    # the plan: one op more, FPD_OP_EMA, the last of the optimizer's range; every other phase as it was
    b, e = step.student.rng['adam']
    assert len(step.student.plan) == plain_ops + 1 and e - b == 2 and e == len(step.student.plan)
    assert step.student.plan.op_type(b) == (R.OP_SGD if kind == 'sgd' else R.OP_ADAM) and step.student.plan.op_type(b + 1) == R.OP_EMA
    launches = step.launches_per_step()
    assert plain_launches['student_adam'] == 1 and launches['student_adam'] == 2 and launches['total'] == plain_launches['total'] + 1
    assert all(launches[k] == v for k, v in plain_launches.items() if k not in ('student_adam', 'total'))
    avg = [ema.flat[n].cpu().numpy().copy() for n in ('param', 'rstat')]
    for k in range(STEPS):
        step.set_batch(*_cases.batch('tiny', k))
        step.step()
        st = _state(student, step, opt)
        _same_state(st, plain[k], '%s step %d' % (kind, k))                       # the average only reads
        w = E.weight(k, decay, warmup)
        avg = [E.update(a, st[n].numpy(), w) for a, n in zip(avg, ('param', 'rstat'))]
        for a, n in zip(avg, ('param', 'rstat')):
            assert np.array_equal(_bits(ema.flat[n].cpu().numpy()), _bits(a)), '%s arena of the average after step %d' % (n, k)
        assert torch.equal(ema.flat['nbt'].cpu(), st['nbt']) and ema.updates == k + 1
    assert not np.array_equal(avg[0], plain[-1]['param'].numpy()) and int(plain[-1]['nbt'].max()) == STEPS


def test_deferred_optimizer_range_averages_exactly_once_per_step():
    """allreduce= given (the identity hook): the optimizer range of step k runs at the start of step k + 1, the last one in
    flush().  Same parameters as the plain run, the average of the restatement over those parameters, four updates."""
    plain, _, _ = _plain_trajectory('adam')
    student, step, opt, ema = _make_step('adam', True, decay=0.999, warmup=False)
    avg = [ema.flat[n].cpu().numpy().copy() for n in ('param', 'rstat')]
    for k in range(STEPS):
        step.set_batch(*_cases.batch('tiny', k))
        step.teacher_async(_cases.batch('tiny', k)[0])
        step.student_step(_identity)
        assert ema.updates == k                                                   # step k's range is still pending
    step.flush()
    step.flush()                                                                  # nothing is pending any more: no second update
    st = _state(student, step, opt)
    _same_state(st, plain[-1], 'deferred')
    assert ema.updates == STEPS
    # the deferred range runs in front of the next step's forward: update k sees the parameters and statistics of step k
    for k in range(STEPS):
        w = E.weight(k, 0.999, False)
        avg = [E.update(a, plain[k][n].numpy(), w) for a, n in zip(avg, ('param', 'rstat'))]
    assert np.array_equal(_bits(ema.flat['param'].cpu().numpy()), _bits(avg[0]))
    assert np.array_equal(_bits(ema.flat['rstat'].cpu().numpy()), _bits(avg[1]))


def test_step_cache_keys_on_the_ema_object_and_a_foreign_average_is_refused():
    from fpd_amd import executor as EX, runtime as R
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.utils.utils import FusedAdam, ModelEma
    c, gold, student, teacher = _models()
    opt = FusedAdam(student, lr=1e-3)
    shape = _cases.batch('tiny', 0)[0].shape
    ema = ModelEma(student)
    plain = F.fused_step_for(student, teacher, opt, shape, 0.5)
    with_ema = F.fused_step_for(student, teacher, opt, shape, 0.5, ema=ema)
    assert plain is not with_ema and plain.ema is None and with_ema.ema is ema
    assert F.fused_step_for(student, teacher, opt, shape, 0.5, ema=ema) is with_ema and F.fused_step_for(student, teacher, opt, shape, 0.5) is plain
    assert F.fused_step_for(student, teacher, opt, shape, 0.5, ema=ModelEma(student)) is not with_ema
    _, _, other, _ = _models()
    with pytest.raises(R.FpdError, match='another model'):
        EX.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, c['batch'], c['image'][1],
                        c['image'][0], alpha=0.5, ema=ModelEma(other))


# ---- ModelEma.module and update() ----

def test_module_is_the_averaged_model_evaluates_like_a_loaded_copy_and_refuses_training():
    from fpd_amd import runtime as R
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.models import hourglass
    from fpd_amd.lib.utils.utils import FusedAdam, ModelEma
    from tests.test_model_gpu import make_cfg
    c, gold, student, teacher = _models()
    opt, crit = FusedAdam(student, lr=1e-2), JointsMSELoss(True).cuda()
    ema = ModelEma(student, decay=0.9, warmup=False)
    x, tg, tw = (t.cuda() for t in _cases.batch('tiny', 0))
    avg = ema.flat['param'].cpu().numpy().copy()
    student.train()
    for k in range(2):                                       # the module-API path: loss.backward(); optimizer.step(); ema.update()
        opt.zero_grad()
        loss = sum(crit(o, tg, tw) for o in student(x))
        loss.backward()
        opt.step()
        ema.update()
        torch.cuda.synchronize()
        avg = E.update(avg, student._flat['param'].cpu().numpy(), E.weight(k, 0.9, False))
    assert ema.updates == 2 and np.array_equal(_bits(ema.flat['param'].cpu().numpy()), _bits(avg))
    assert not torch.equal(ema.flat['param'], student._flat['param']) and torch.equal(ema.flat['nbt'], student._flat['nbt'])
    sd = ema.state_dict()['state_dict']
    assert list(sd) == list(student.state_dict()) == list(ema.module.state_dict())
    assert all(sd[k].shape == v.shape for k, v in student.state_dict().items())
    fresh = hourglass.get_pose_net(make_cfg(c['s'][0], c['s'][1], c['joints']), is_train=False)
    fresh.load_state_dict(sd, strict=True)
    fresh = fresh.cuda().eval()
    assert not ema.module.training
    with torch.no_grad():
        a, b = ema.module(x), fresh(x)
        raw = student.eval()(x)
    assert len(a) == len(b) == c['s'][1] and all(torch.equal(u, v) for u, v in zip(a, b)) and not torch.equal(a[-1], raw[-1])
    with pytest.raises(R.FpdError, match='eval'):
        ema.module.train()
    out = ema.module(x)                                      # with autograd on: the same bits, and a backward that refuses
    assert all(torch.equal(u, v) for u, v in zip(out, a))
    with pytest.raises(R.FpdError, match='never trained'):
        out[-1].sum().backward()
    ema.set(student)
    assert ema.updates == 0 and torch.equal(ema.flat['param'], student._flat['param']) and torch.equal(ema.flat['rstat'], student._flat['rstat'])


# ---- two shards ----

def test_two_shards_on_one_gpu_keep_bit_equal_averaged_parameters():
    """The arrangement of tests/test_dist_gpu.py: two replicas with world_size = 2, each on its shard, the flat gradients
    summed on the device between the backward and the deferred optimizer range.  No collective is added for the average:
    every rank applies the same update to the same weights."""
    from fpd_amd import dist as fdist, executor as EX
    from fpd_amd.lib.utils.utils import ModelEma
    from oracle import fpd_ref
    from tests.test_dist_gpu import _Replica
    c = _cases.CONFIGS['tiny']
    reps, emas = [], []
    for r in range(2):
        _, _, student, teacher = _models()
        emas.append(ModelEma(student, decay=0.9998, warmup=True))
        step = EX.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, 2, c['image'][1],
                               c['image'][0], alpha=0.5, lr=2.5e-4, world_size=2, ema=emas[-1])
        reps.append(_Replica(step, student))
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
    assert emas[0].updates == emas[1].updates == 3
    assert torch.equal(emas[0].flat['param'], emas[1].flat['param'])
    assert torch.equal(reps[0].model._flat['param'], reps[1].model._flat['param'])
    assert not torch.equal(emas[0].flat['param'], reps[0].model._flat['param'])
    assert not torch.equal(emas[0].flat['rstat'], emas[1].flat['rstat'])            # running statistics are per rank


# ---- tools ----

def _run_tool(tool, out_dir, extra, timeout=300):
    cfgd = os.path.join(ROOT, 'experiments', 'fpd_synthetic')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', tool), '--cfg', os.path.join(cfgd, 'hg4x128_student_ema.yaml')]
    if tool == 'train.py':
        cmd += ['--max-iters', '2']
    cmd += ['OUTPUT_DIR', str(out_dir), 'MODEL.EXTRA.NUM_FEATURES', '32', 'MODEL.EXTRA.NUM_STACKS', '2', 'MODEL.IMAGE_SIZE', '128,128',
            'MODEL.HEATMAP_SIZE', '32,32', 'TRAIN.BATCH_SIZE_PER_GPU', '4', 'TEST.BATCH_SIZE_PER_GPU', '4', 'DATASET.NUM_SAMPLES', '32',
            'DATASET.NUM_VALID_SAMPLES', '8', 'PRINT_FREQ', '1', 'TRAIN.LR_STEP', '[2,3]', 'AUTO_RESUME', 'True', 'MODEL.DTYPE', 'fp32',
            'TRAIN.SHUFFLE', 'False', 'TRAIN.LR', '0.001', 'TRAIN.EMA_DECAY', '0.9'] + extra
    return subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=timeout)


def _find(root, name):
    hits = [os.path.join(dp, f) for dp, _, fs in os.walk(root) for f in fs if f == name]
    assert len(hits) == 1, (name, hits)
    return hits[0]


def _last_validation(log):
    tests = [l.split('Loss ', 1)[1] for l in log.splitlines() if 'Test: [' in l]
    rows = [l.split('| ', 1)[1] for l in log.splitlines() if '| hourglass' in l]
    return tests[-1], rows[-1]


def test_tools_train_with_ema_checkpoints_resumes_to_the_same_bits_and_test_py_evaluates_the_average(tmp_path):
    """tools/train.py with TRAIN.EMA for 2 epochs of 2 iterations, once in one go and once as 1 epoch + AUTO_RESUME; then
    tools/test.py on the average.  Every run is a child process of its own; nothing further is started when one fails."""
    load = lambda p: torch.load(p, map_location='cpu', weights_only=False)
    whole, parts = tmp_path / 'whole', tmp_path / 'parts'
    r = _run_tool('train.py', whole, ['TRAIN.END_EPOCH', '2'])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    r1 = _run_tool('train.py', parts, ['TRAIN.END_EPOCH', '1'])
    assert r1.returncode == 0, (r1.stdout[-1500:], r1.stderr[-3000:])
    ck1 = load(_find(parts, 'checkpoint.pth'))
    assert ck1['epoch'] == 1 and ck1['ema_updates'] == 2 and list(ck1['ema_state_dict']) == [k[7:] for k in ck1['state_dict']]
    best = load(_find(parts, 'model_best.pth'))              # the first epoch is always the best so far: the average of epoch 0
    assert all(torch.equal(best[k], v) for k, v in ck1['ema_state_dict'].items())
    assert any(not torch.equal(ck1['state_dict']['module.' + k], v) for k, v in ck1['ema_state_dict'].items() if k.endswith('.weight'))
    r2 = _run_tool('train.py', parts, ['TRAIN.END_EPOCH', '2'])
    assert r2.returncode == 0, (r2.stdout[-1500:], r2.stderr[-3000:])
    log2 = r2.stdout + r2.stderr
    assert 'loaded checkpoint' in log2 and 'epoch 1 done' in log2 and 'epoch 0 done' not in log2 and 'no ema_state_dict' not in log2
    a, b = load(_find(whole, 'checkpoint.pth')), load(_find(parts, 'checkpoint.pth'))
    assert a['epoch'] == b['epoch'] == 2 and a['ema_updates'] == b['ema_updates'] == 4
    for key in ('state_dict', 'ema_state_dict'):             # the step is bit-repeatable: a resumed run IS the uninterrupted one
        assert all(torch.equal(a[key][k], b[key][k]) for k in a[key]), key
    final = load(_find(parts, 'final_state.pth'))
    assert all(torch.equal(final[k], v) for k, v in b['ema_state_dict'].items())
    # tools/test.py on the average reproduces the validation the training run logged for its last epoch
    t = _run_tool('test.py', parts, ['TEST.USE_EMA', 'True', 'TEST.MODEL_FILE', _find(parts, 'checkpoint.pth')])
    assert t.returncode == 0, (t.stdout[-1500:], t.stderr[-3000:])
    assert 'averaged weights (4 updates)' in t.stdout + t.stderr
    assert _last_validation(t.stdout + t.stderr) == _last_validation(log2)
    # ... and a file without the average is an error, not a silent evaluation of something else
    t2 = _run_tool('test.py', parts, ['TEST.USE_EMA', 'True', 'TEST.MODEL_FILE', _find(parts, 'model_best.pth')])
    assert t2.returncode != 0 and 'ema_state_dict' in t2.stderr
