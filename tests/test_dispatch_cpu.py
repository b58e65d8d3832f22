"""The dispatch queries against the launches they answer for, without a device.  Two fusions are decided at lowering time by
asking the library (executor.Lowering): fpd_conv_fold_supported() / fpd_conv_pair_fold_supported() -- 1 means the launch
evaluates the BN-backward apply on its operand (fpd_conv_t.fold_x) and the stand-alone apply is lowered as a no-op -- and
fpd_conv_fused_wgrad_partials() / the pair form -- the weight-gradient slabs the launch writes, which size the workspace.  The
queries are asked on the descriptor BEFORE the fold and slab fields are filled in, and the launches are decided on the
descriptor AFTER; include/fpd_amd.h promises that the fold query looks at the dimensions, the epilogue and the prologue only.
A query that answers for another launch than the one made leaves a plan whose apply is gone and whose launch fails.

Properties, over a grid of data-gradient descriptors (N, square maps 4..128, C and K in {16, 32, 64, 128}, 1x1 and 3x3, with and
without a prologue BN, bf16; pairs of equal channel shape on two map sizes, as the hourglass pairs are) and under every
combination of the conv_c1 / conv_c3 / conv_pp modes {0, 1, 2} (1, 1, 1 = the default options):
  P1  the fold query answers the same with the fold fields NULL and set (pairs: on a, on b, on both);
  P2  the fold query answers the same with the slab fields (wg_partial, wg_stride, wg_count) NULL and set;
  P3  the slab query answers the same with the slab fields NULL and set;
  P4  where the fold query is 1 and the slab count n > 0, the slab count with the fold fields set is n as well (the executor
      asks for the slab count first, then fills the fold fields; the launch checks wg_count against its own geometry);
  P5  every conv / conv-pair struct the lowering of the benchmark student (and of an HRNet student) emits: folded -> the fold
      query says 1 on the struct as emitted; slabs -> the slab query gives wg_count on it.
Addresses are fake (16-byte aligned, distinct, never dereferenced): the predicates are pure host code."""
import contextlib
import ctypes
import itertools

import pytest

from oracle import hourglass_ref
from tests.test_lowering_cpu import FakeArenas

NS = (1, 2, 4, 8, 16, 32)
MAPS = (4, 8, 16, 32, 64, 128)
CHANNELS = (16, 32, 64, 128)
MODES = list(itertools.product((0, 1, 2), repeat=3))         # (conv_c1, conv_c3, conv_pp); (1, 1, 1) = the defaults

_addr = itertools.count(1)


def _fake():
    """A distinct 16-byte aligned address."""
    return (1 << 36) + 4096 * next(_addr)


@pytest.fixture(scope='module')
def R():
    from fpd_amd import runtime
    runtime.lib()
    return runtime


@contextlib.contextmanager
def _modes(R, c1, c3, pp):
    prev = {}
    try:
        for name, v in (('conv_c1', c1), ('conv_c3', c3), ('conv_pp', pp)):
            prev[name] = R.set_option(name, v)
        yield
    finally:
        for name, v in prev.items():
            R.set_option(name, v)


def _bn(R, s):
    s.mode, s.relu, s.eps = R.BN_TRAIN, 1, 1e-5
    s.gamma, s.beta, s.stats = _fake(), _fake(), _fake()


def _dgrad(R, N, H, C, K, r, bn):
    """BNRELU_BWD data-gradient descriptor (C input channels = the forward's K), fold and slab fields NULL."""
    a = R.ConvT()
    a.N, a.H, a.W, a.C, a.K, a.R, a.S, a.stride, a.pad, a.P, a.Q = N, H, H, C, K, r, r, 1, (r - 1) // 2, H, H
    a.dtype, a.epi = R.BF16, R.EPI_BNRELU_BWD
    a.x, a.w, a.y, a.epi_x, a.epi_stats = _fake(), _fake(), _fake(), _fake(), _fake()
    _bn(R, a.epi_bn)
    if bn:
        _bn(R, a.bn)
    return a


def _with_fold(R, a):
    f = R.ConvT.from_buffer_copy(a)
    f.fold_x, f.fold_out, f.fold_stats, f.fold_dgamma, f.fold_dbeta = _fake(), _fake(), _fake(), _fake(), _fake()
    _bn(R, f.fold_bn)
    return f


def _with_slabs(a, n):
    f = type(a).from_buffer_copy(a)
    f.wg_partial, f.wg_stride, f.wg_bias, f.wg_count = _fake(), (a.C * a.K + a.C + 63) // 64 * 64, 1, n
    return f


def _name(a):
    return 'N=%d %dx%d C=%d->K=%d %dx%d%s' % (a.N, a.H, a.W, a.C, a.K, a.R, a.S, ' +BN' if a.bn.mode else '')


class Queries:
    def __init__(self, R):
        self.R, self.l = R, R.lib()

    def fold(self, a):
        return self.l.fpd_conv_fold_supported(ctypes.byref(a))

    def slabs(self, a):
        return self.l.fpd_conv_fused_wgrad_partials(ctypes.byref(a))

    def pair(self, a, b):
        p = self.R.ConvPairT()
        p.a, p.b = a, b
        return p

    def pfold(self, a, b):
        return self.l.fpd_conv_pair_fold_supported(ctypes.byref(self.pair(a, b)))

    def pslabs(self, a, b):
        na, nb = ctypes.c_int32(-1), ctypes.c_int32(-1)
        assert self.l.fpd_conv_pair_fused_wgrad_partials(ctypes.byref(self.pair(a, b)), ctypes.byref(na), ctypes.byref(nb)) == 0
        return na.value, nb.value


_grid = {}


def _singles(R):
    if 'singles' not in _grid:
        out = []
        for N, H, C, K, r, bn in itertools.product(NS, MAPS, CHANNELS, CHANNELS, (1, 3), (False, True)):
            a = _dgrad(R, N, H, C, K, r, bn)
            out.append((a, _with_fold(R, a)))
        _grid['singles'] = out
    return _grid['singles']


def _pairs(R):
    """Up- / low-branch pairs of an hourglass level: equal channel shapes, the second half on the map of half the size."""
    if 'pairs' not in _grid:
        out = []
        for N, H, C, K, r, bn in itertools.product(NS, MAPS[1:], CHANNELS, CHANNELS, (1, 3), (False, True)):
            a, b = _dgrad(R, N, H, C, K, r, bn), _dgrad(R, N, H // 2, C, K, r, bn)
            out.append((a, b, _with_fold(R, a), _with_fold(R, b)))
        _grid['pairs'] = out
    return _grid['pairs']


def _report(fails, mode):
    assert not fails, '%d violations under conv_c1 / conv_c3 / conv_pp = %s:\n  %s' % (
        len(fails), mode, '\n  '.join(fails[:40] + (['...'] if len(fails) > 40 else [])))


@pytest.mark.parametrize('mode', MODES, ids=['c1=%d,c3=%d,pp=%d' % m for m in MODES])
def test_single_dgrad_queries_answer_for_the_launch(R, mode):
    q = Queries(R)
    fails = []
    with _modes(R, *mode):
        for a, fa in _singles(R):
            f0, n0 = q.fold(a), q.slabs(a)
            if q.fold(fa) != f0:
                fails.append('P1 %s: fold query %d with fold_x NULL, %d with it set' % (_name(a), f0, q.fold(fa)))
            if n0 <= 0:
                continue
            wa, wfa = _with_slabs(a, n0), _with_slabs(fa, n0)
            if q.fold(wa) != f0 or q.fold(wfa) != f0:
                fails.append('P2 %s: fold query %d without slab fields, %d / %d (unfolded / folded) with them' % (
                    _name(a), f0, q.fold(wa), q.fold(wfa)))
            if q.slabs(wa) != n0:
                fails.append('P3 %s: slab query %d without slab fields, %d with them' % (_name(a), n0, q.slabs(wa)))
            if f0 == 1 and (q.slabs(fa) != n0 or q.slabs(wfa) != n0):
                fails.append('P4 %s: %d slabs unfolded, %d / %d folded (without / with slab fields)' % (
                    _name(a), n0, q.slabs(fa), q.slabs(wfa)))
    _report(fails, mode)


@pytest.mark.parametrize('mode', MODES, ids=['c1=%d,c3=%d,pp=%d' % m for m in MODES])
def test_pair_dgrad_queries_answer_for_the_launch(R, mode):
    q = Queries(R)
    fails = []
    with _modes(R, *mode):
        for a, b, fa, fb in _pairs(R):
            name = 'pair %s + %dx%d' % (_name(a), b.H, b.W)
            f0, (na, nb) = q.pfold(a, b), q.pslabs(a, b)
            folded = (('a', fa, b), ('b', a, fb), ('both', fa, fb))
            for which, x, y in folded:
                if q.pfold(x, y) != f0:
                    fails.append('P1 %s: fold query %d with fold_x NULL, %d with it set on %s' % (name, f0, q.pfold(x, y), which))
            if na <= 0 or nb <= 0:
                continue
            wa, wb = _with_slabs(a, na), _with_slabs(b, nb)
            if q.pfold(wa, wb) != f0:
                fails.append('P2 %s: fold query %d without slab fields, %d with them' % (name, f0, q.pfold(wa, wb)))
            if q.pslabs(wa, wb) != (na, nb):
                fails.append('P3 %s: slab query %s without slab fields, %s with them' % (name, (na, nb), q.pslabs(wa, wb)))
            if f0 == 1:
                for which, x, y in folded:
                    got = (q.pslabs(x, y), q.pslabs(_with_slabs(x, na), _with_slabs(y, nb)))
                    if got != ((na, nb), (na, nb)):
                        fails.append('P4 %s: %s slabs unfolded, %s / %s with the fold on %s (without / with slab fields)' % (
                            name, (na, nb), got[0], got[1], which))
    _report(fails, mode)


def _check_lowered(q, low, ir_ops, lowered, finish):
    """P5 on the structs exactly as they go to the library (after finish_partials() patched the slab pointers)."""
    R = q.R
    finish()
    fails, n_fold, n_slab = [], 0, 0
    for op, (code, st) in zip(ir_ops, lowered):
        if code == R.OP_CONV:
            if st.fold_x:
                n_fold += 1
                if q.fold(st) != 1:
                    fails.append('%s: emitted folded, fold query %d' % (_name(st), q.fold(st)))
            if st.wg_partial:
                n_slab += 1
                if q.slabs(st) != st.wg_count:
                    fails.append('%s: emitted with %d slabs, slab query %d' % (_name(st), st.wg_count, q.slabs(st)))
        elif code == R.OP_CONV_PAIR:
            name = 'pair %s + %dx%d' % (_name(st.a), st.b.H, st.b.W)
            if st.a.fold_x or st.b.fold_x:
                n_fold += 1
                if q.pfold(st.a, st.b) != 1:
                    fails.append('%s: emitted folded, fold query %d' % (name, q.pfold(st.a, st.b)))
            if st.a.wg_partial or st.b.wg_partial:
                n_slab += 1
                got = q.pslabs(st.a, st.b)
                if got != (st.a.wg_count, st.b.wg_count):
                    fails.append('%s: emitted with %s slabs, slab query %s' % (name, (st.a.wg_count, st.b.wg_count), got))
    return fails, n_fold, n_slab


def _lower_backward(R, g):
    from fpd_amd import executor as E
    low = E.Lowering(FakeArenas(), R.BF16)
    low.use_partials = True
    bwd = [o for o in g.bwd if o.kind != 'seed']
    low.plan_folds(bwd)
    return low, bwd, [low.op(o) for o in bwd]


@pytest.mark.parametrize('size', [256, 128])
def test_lowered_student_structs_match_the_queries(R, monkeypatch, size):
    """The benchmark student (hg4x128, 4 stacks, 16 joints) at batch 1..32: every emitted data gradient is served as emitted."""
    from fpd_amd import graph as G
    monkeypatch.setenv('FPD_FOLD_APPLY', '1')
    q = Queries(R)
    fails, totals = [], []
    for B in NS:
        g = G.HourglassGraph(G.ParamTable(hourglass_ref.hourglass_keys(128, 4, 16)), 128, 4, 16, B, size, size, train=True)
        G.plan_memory(g.fwd + g.bwd, reuse_delay=400)
        low, bwd, lowered = _lower_backward(R, g)
        f, nf, ns = _check_lowered(q, low, bwd, lowered, low.finish_partials)
        fails += ['B=%d %d^2: %s' % (B, size, m) for m in f]
        totals.append((B, nf, ns))
    assert not fails, '\n'.join(fails[:40])
    # the check must see folded and slab-carrying launches (at batch 32 and 256^2: 118 folds, 102 fused weight gradients)
    assert all(nf > 0 for _, nf, _ in totals) and any(ns > 0 for _, _, ns in totals), totals


def test_lowered_hrnet_structs_match_the_queries(R, monkeypatch):
    """The HRNet product path (W32 topology, 256x192) at batch 2 and 32: same check on its emitted structs."""
    from fpd_amd import graph as G
    from oracle import hrnet_ref
    from tests._cases_hrnet import extra_cfg
    monkeypatch.setenv('FPD_FOLD_APPLY', '1')
    q = Queries(R)
    ex = extra_cfg(dict(widths=[32, 64, 128, 256], blocks=4, modules=(1, 4, 3)))
    table = G.ParamTable(hrnet_ref.hrnet_keys(ex, 17), bucket_of=G.hrnet_bucket_of)
    fails, totals = [], []
    for B in (2, 32):
        g = G.HRNetGraph(table, ex, 17, B, 256, 192, True, wlp_is_master=False)
        G.plan_memory(g.fwd + g.bwd, reuse_delay=4)
        low, bwd, lowered = _lower_backward(R, g)
        f, nf, ns = _check_lowered(q, low, bwd, lowered, low.finish_partials)
        fails += ['HRNet B=%d: %s' % (B, m) for m in f]
        totals.append((B, nf, ns))
    assert not fails, '\n'.join(fails[:40])
    assert any(nf > 0 for _, nf, _ in totals), totals


def test_launch_refuses_a_fusion_its_route_does_not_offer(R):
    """A launch whose fields ask for a fusion its route does not offer is refused by the dispatcher, naming the query that would
    have said so.  conv_c1 / conv_c3 / conv_pp are off, so the route is conv_tile's: no fused weight gradient at all, and no
    folded apply at four output tiles per block (128 output channels on 128 or more pixel tiles).  The refusal comes before any
    device call (api.hip launch_conv), so nothing is launched and the fake addresses are never dereferenced."""
    q = Queries(R)

    def refused(rc, query):
        err = q.l.fpd_last_error().decode()
        assert rc < 0 and query + '()' in err, (rc, err)

    with _modes(R, 0, 0, 0):
        a = _dgrad(R, 4, 64, 128, 64, 1, False)
        assert q.slabs(a) == 0
        refused(q.l.fpd_conv_forward(ctypes.byref(_with_slabs(a, 4)), None), 'fpd_conv_fused_wgrad_partials')
        a, b = _dgrad(R, 4, 64, 128, 128, 1, False), _dgrad(R, 4, 32, 128, 128, 1, False)
        assert q.fold(a) == 0 and q.pfold(a, b) == 0
        refused(q.l.fpd_conv_forward(ctypes.byref(_with_fold(R, a)), None), 'fpd_conv_fold_supported')
        refused(q.l.fpd_conv_forward_pair(ctypes.byref(q.pair(_with_fold(R, a), _with_fold(R, b))), None), 'fpd_conv_pair_fold_supported')
