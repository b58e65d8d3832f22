"""Host logic of the up-add formed on load by the frozen fused Bottleneck (fpd_bneck_t.x2, executor.Lowering.plan_upadd), without a
GPU (fake arena addresses as in tests/test_lowering_cpu.py).  Every hourglass level ends in `up1 + up(low)`; in an eval-mode graph
with fused Bottlenecks the sum's only reader is the single Bottleneck behind it (`low2` of the parent level, `res` behind the
outermost level), which then names both sources as its inputs while the up-add accesses nothing and its result is never allocated."""
import ctypes

import pytest

from oracle import hourglass_ref
from tests.test_lowering_cpu import FakeArenas


def _graph(feats, stacks, train, batch=2):
    from fpd_amd import graph as G
    return G.HourglassGraph(G.ParamTable(hourglass_ref.hourglass_keys(feats, stacks, 16)), feats, stacks, 16, batch, 256, 256, train=train,
                            wlp_is_master=False, fuse_bneck=not train)


def _upadds(g):
    return [o for o in g.fwd if o.kind == 'ew' and o.op == 'upadd_fwd']


def _lower(g, readers=None):
    from fpd_amd import executor as E, graph as G
    ops = g.fwd + g.bwd
    n = E.Lowering.plan_upadd(g.fwd, readers=ops if readers is None else readers)
    G.plan_memory(ops, reuse_delay=400 if g.train else 0)
    low = E.Lowering(FakeArenas(), 1)
    low.train = g.train
    if g.train:
        return n, low, None
    return n, low, [low.op(o) for o in g.fwd]


def _overlap(a, b):
    return a.arena == b.arena and a.off < b.off + b.numel and b.off < a.off + a.numel


@pytest.mark.parametrize('feats,stacks', [(128, 1), (256, 2)])
def test_eval_graph_absorbs_four_upadds_per_stack(monkeypatch, feats, stacks):
    from fpd_amd import runtime as R
    R.lib()
    monkeypatch.delenv('FPD_BNECK_UPADD', raising=False)
    g = _graph(feats, stacks, train=False)
    order = list(g.fwd)
    ups = _upadds(g)
    assert len(ups) == 4 * stacks
    sources = {id(u): (u.x, u.x2, u.y) for u in ups}
    n, low, lowered = _lower(g)
    assert n == 4 * stacks and all(a is b for a, b in zip(order, g.fwd)) and len(order) == len(g.fwd)      # the op list keeps every op
    pos = {id(o): i for i, o in enumerate(g.fwd)}
    pos.update({id(m): i for i, o in enumerate(g.fwd) if o.kind == 'bneck2' for m in (o.a, o.b)})      # (up1 comes out of a pair launch)
    consumers = [o for o in g.fwd if o.kind == 'bneck' and getattr(o, 'x2', None) is not None]
    assert len(consumers) == 4 * stacks
    assert sorted(o.dims[2] for o in consumers) == sorted([8, 16, 32, 64] * stacks)
    A = low.A
    for o in consumers:
        ua = o.upadd_op
        up1, lowb, summed = sources[id(ua)]
        assert ua.upadd_absorbed and o.x is up1 and o.x2 is lowb and pos[id(ua)] < pos[id(o)]
        assert ua.accesses() == ([], []) and ua.acts_in() == [] and ua.acts_out() == []
        assert summed.buf is None                          # the sum is never allocated
        rd, wr = o.accesses()
        assert up1.buf in rd and lowb.buf in rd and wr == [o.y.buf]
        assert any(t is up1 for t in o.acts_in()) and any(t is lowb for t in o.acts_in())
        assert lowb.shape == (up1.shape[0], up1.shape[1] // 2, up1.shape[2] // 2, up1.shape[3])
        # planned intervals: y, x and x2 are pairwise disjoint
        assert not _overlap(o.y.buf, up1.buf) and not _overlap(o.y.buf, lowb.buf) and not _overlap(up1.buf, lowb.buf)
        code, s = lowered[pos[id(o)]]
        assert code == R.OP_BNECK and s.x == A.ptr(up1.buf) and s.x2 == A.ptr(lowb.buf) and s.y == A.ptr(o.y.buf)
        assert lowered[pos[id(ua)]][0] == R.OP_NOP
        # both sources stay alive and unwritten up to the Bottleneck: a tensor that overlaps one is written before its producer or after
        for src in (up1, lowb):
            for j, r in enumerate(g.fwd):
                for t in r.acts_out():
                    if t is not src and t.buf is not None and _overlap(t.buf, src.buf):
                        assert j > pos[id(o)] or j < pos[id(src.producer)], 'a source of the up-add is overwritten before the Bottleneck reads it'
    # every other fused Bottleneck is lowered as before
    for o, (code, s) in zip(g.fwd, lowered):
        if o.kind == 'bneck' and o not in consumers:
            assert s.x2 is None
    assert sum(1 for c, _ in lowered if c != R.OP_NOP) == len(g.fwd) - 4 * stacks


def test_train_graph_absorbs_none(monkeypatch):
    from fpd_amd import runtime as R
    R.lib()
    monkeypatch.delenv('FPD_BNECK_UPADD', raising=False)
    g = _graph(128, 1, train=True)
    ups = _upadds(g)
    assert len(ups) == 4 and all(u.out_stats is not None for u in ups)      # the student's up-adds produce the statistics of the sum
    n, _, _ = _lower(g)
    assert n == 0 and not any(getattr(o, 'upadd_absorbed', False) for o in g.fwd)
    assert all(u.y.buf is not None for u in ups)


def test_knob_off_absorbs_none(monkeypatch):
    from fpd_amd import runtime as R
    R.lib()
    monkeypatch.setenv('FPD_BNECK_UPADD', '0')
    g = _graph(128, 1, train=False)
    n, _, lowered = _lower(g)
    assert n == 0 and sum(1 for c, _ in lowered if c != R.OP_NOP) == len(g.fwd)
    assert all(u.y.buf is not None and not getattr(u, 'upadd_absorbed', False) for u in _upadds(g))
    # the library's own switch: the query says no, the lowering follows it
    monkeypatch.delenv('FPD_BNECK_UPADD')
    prev = R.set_option('bneck_upadd', 0)
    try:
        g = _graph(128, 1, train=False)
        assert _lower(g)[0] == 0
    finally:
        R.set_option('bneck_upadd', prev)


def test_upadd_with_a_second_reader_is_kept(monkeypatch):
    from fpd_amd import graph as G, runtime as R
    R.lib()
    monkeypatch.delenv('FPD_BNECK_UPADD', raising=False)
    g = _graph(128, 1, train=False)
    ups = _upadds(g)
    shared = ups[1]
    extra = G.Op('ew', op='relu_mask', dims=shared.y.shape, x=shared.y, x2=None, dy=shared.y, add=None, y=G.Act(shared.y.shape, 'extra'),
                 out_stats=None, bstats=None, dgamma=None, dbeta=None, bn=None)
    n, low, lowered = _lower(g, readers=g.fwd + [extra])
    assert n == 3 and not getattr(shared, 'upadd_absorbed', False) and shared.y.buf is not None
    pos = {id(o): i for i, o in enumerate(g.fwd)}
    assert lowered[pos[id(shared)]][0] == R.OP_EW
    reader = next(o for o in g.fwd if o.kind == 'bneck' and o.x is shared.y)
    assert getattr(reader, 'x2', None) is None and lowered[pos[id(reader)]][1].x2 is None
    assert all(getattr(u, 'upadd_absorbed', False) for u in ups if u is not shared)


def test_query_domain():
    """Pure host calls: dimensions, dtype and the option decide; no pointer is read."""
    from fpd_amd import runtime as R
    l = R.lib()
    s = R.BneckT()

    def ask(N, H, W, C, P, dtype=R.BF16):
        (s.N, s.H, s.W, s.C, s.P, s.dtype) = (N, H, W, C, P, dtype)
        return l.fpd_bneck_upadd_supported(ctypes.byref(s))
    for W in (8, 16, 32, 64):
        assert ask(2, W, W, 256, 128) == 1 and ask(2, W, W, 128, 64) == 1
    assert ask(2, 4, 4, 256, 128) == 0                     # up-add results are never 4 wide
    assert ask(2, 1, 16, 256, 128) == 0                    # odd H
    assert ask(2, 128, 128, 256, 128) == 0 and ask(2, 16, 16, 256, 64) == 0 and ask(2, 16, 16, 64, 32) == 0
    assert ask(2, 16, 16, 256, 128, R.F32) == 0
    assert l.fpd_bneck_upadd_supported(None) == 0
    assert l.fpd_abi_sizeof(b'fpd_bneck_t') == ctypes.sizeof(R.BneckT) and l.fpd_abi_version() == 2
    prev = R.set_option('bneck_upadd', 0)
    try:
        assert ask(2, 16, 16, 256, 128) == 0
    finally:
        R.set_option('bneck_upadd', prev)
    assert ask(2, 16, 16, 256, 128) == 1
