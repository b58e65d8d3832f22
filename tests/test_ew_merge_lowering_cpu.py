"""Host logic of executor.Lowering.plan_ew_merge without a GPU (the library's query is pure host code): on the backward of
the benchmark student (hg4x128, batch 32, 256x256; lowered as tests/test_lowering_cpu.py does, the pass run after memory
planning) the BN-backward applies that carry a residual add are absorbed by the pool-backward op behind them -- 17 groups
in front of a max-pool backward, 16 in front of an up-sample backward, 33 launches fewer -- and hand-made lists that break
the aliasing or the single-reader condition are declined."""
import pytest

from oracle import hourglass_ref
from tests.test_lowering_cpu import FakeArenas


def _members(op):
    return [m for m in ((op.a, op.b) if op.kind in ('conv2', 'ew2') else (op,)) if m is not None]


def _lower(monkeypatch, merge):
    from fpd_amd import executor as E, graph as G, runtime as R
    R.lib()
    monkeypatch.setenv('FPD_FOLD_APPLY', '1')
    monkeypatch.setenv('FPD_EW_MERGE', '1' if merge else '0')
    g = G.HourglassGraph(G.ParamTable(hourglass_ref.hourglass_keys(128, 4, 16)), 128, 4, 16, 32, 256, 256, train=True)
    G.plan_memory(g.fwd + g.bwd, reuse_delay=400)
    low = E.Lowering(FakeArenas(), 1)
    low.use_partials = True
    bwd = [o for o in g.bwd if o.kind != 'seed']
    low.plan_folds(bwd)
    low.plan_ew_merge(bwd)
    lowered = [low.op(o) for o in bwd]
    return E, R, low, bwd, lowered


def test_benchmark_student_backward_merges_33_applies_into_their_pool_backward(monkeypatch):
    E, R, low, bwd, lowered = _lower(monkeypatch, merge=True)
    marked = [(i, o) for i, o in enumerate(bwd) if getattr(o, 'ewm_kind', None) is not None]
    assert sum(1 for _, o in marked if o.ewm_kind == 'maxpool_bwd') == 17
    assert sum(1 for _, o in marked if o.ewm_kind == 'sumpool') == 16
    # 16 apply pairs + the lone half-resolution apply in front of the 128x128 pool backward
    assert sum(1 for _, o in marked if o.ewm_kind == 'maxpool_bwd' and o.ewm_full is not None) == 16
    A = low.A
    iv = lambda b: (b.arena, b.off, b.off + b.numel)
    hit = lambda p, q: p[0] == q[0] and p[1] < q[2] and q[1] < p[2]
    pos = {id(m): i for i, o in enumerate(bwd) for m in _members(o)}
    absorbed = 0
    for i, op in marked:
        code, s = lowered[i]
        assert code == R.OP_EW_MERGE and R.lib().fpd_ew_merge_supported(R.C.byref(s)) == 1
        group = [m for m in (op.ewm_full, op.ewm_half) if m is not None]
        first = min(pos[id(m)] for m in group)
        assert len({pos[id(m)] for m in group}) == 1 and first < i
        # consecutive on lane 0: nothing of lane 0 between the absorbed op and the launch
        assert all((o.lane or 0) != 0 for o in bwd[first + 1:i])
        assert lowered[first][0] == R.OP_NOP and all(getattr(m, 'ewm_absorbed', False) for m in group)
        absorbed += len(group)
        # wiring of the descriptor
        if op.ewm_kind == 'maxpool_bwd':
            assert s.kind == R.EWM_MAXPOOL_BWD and s.pool.dy == s.half.y == A.ptr(op.ewm_half.y.buf)
            assert s.has_full == (1 if op.ewm_full is not None else 0)
            if op.ewm_full is not None:
                assert s.pool.add == s.full.y and s.pool.x == s.full.x
            hidden = [m.y for m in group]
            readers = [r for o in bwd for r in _members(o) if r is not op and any(t is y for t in r.acts_in() for y in hidden)]
            assert not readers
        else:
            assert s.kind == R.EWM_SUMPOOL and s.pool.x == s.full.y == A.ptr(op.ewm_full.y.buf)
            readers = [pos[id(r)] for o in bwd for r in _members(o) if r is not op and any(t is op.ewm_full.y for t in r.acts_in())]
            assert readers and all(j > i for j in readers)      # the data gradient and the residual path read dx AFTER the launch
        # the interval check, restated: no output of the launch overlaps an input of it, on physical arena intervals
        assert E.Lowering._ew_merge_intervals_ok(op, op.ewm_full, op.ewm_half, bwd[first + 1:i], iv, hit)
        rd, wr = op.accesses()
        outs = [b for b in wr if not any(b is m.bstats for m in group) and not (op.ewm_kind == 'maxpool_bwd' and any(b is m.y.buf for m in group))]
        ins = [b for b in rd if not any(b is o for o in outs) and not (op.ewm_kind == 'maxpool_bwd' and any(b is m.y.buf for m in group))]
        assert len(outs) >= 3 and not any(hit(iv(o), iv(b)) for o in outs for b in ins)
        # read and write sets are the union of the group's: the cross-lane waits of the schedule still hold
        for m in group:
            r, w = m.accesses()
            assert all(any(b is x for x in rd) for b in r) and all(any(b is x for x in wr) for b in w)
    assert absorbed == 49
    launches = sum(1 for c, _ in lowered if c != R.OP_NOP)
    _, R2, _, bwd2, lowered2 = _lower(monkeypatch, merge=False)
    assert not any(getattr(m, 'ewm_kind', None) is not None or getattr(m, 'ewm_absorbed', False) for o in bwd2 for m in _members(o))
    assert sum(1 for c, _ in lowered2 if c != R2.OP_NOP) - launches == 33
    assert not any(c == R2.OP_EW_MERGE for c, _ in lowered2)


def _hand_made(G, alias=None, second_reader=False, pattern=1):
    """[apply pair, maxpool_bwd] or [apply, sumpool] on 64-element-aligned offsets of one arena."""
    top = [0]

    def act(shape, name):
        a = G.Act(shape, name)
        n = shape[0] * shape[1] * shape[2] * shape[3]
        a.buf = G.Buf('act', top[0], shape, name)
        top[0] += (n + 63) // 64 * 64
        return a

    def buf(arena, n, name):
        b = G.Buf(arena, top[0], (n,), name)
        top[0] += 64
        return b

    def apply(dims, name):
        C = dims[3]
        bn = G.BN(name, 'train', C, buf('param', C, 'g'), buf('param', C, 'b'), buf('rstat', C, 'm'), buf('rstat', C, 'v'), buf('nbt', 1, 'n'),
                  stats=buf('stats', 8 * C, 's'))
        bn.count = dims[0] * dims[1] * dims[2]
        return G.Op('ew', op='bn_bwd_apply', dims=dims, x=act(dims, name + '.u'), x2=None, dy=act(dims, name + '.g'), add=act(dims, name + '.add'),
                    y=act(dims, name + '.y'), out_stats=None, bstats=buf('stats', 8 * C, 'bs'), dgamma=buf('grad', C, 'dg'), dbeta=buf('grad', C, 'db'), bn=bn)
    full, half = (2, 8, 8, 32), (2, 4, 4, 32)
    none = dict(x2=None, out_stats=None, bstats=None, dgamma=None, dbeta=None, bn=None)
    if pattern == 1:
        a, b = apply(full, 'a'), apply(half, 'b')
        y = act(full, 'y')
        if alias == 'half_input':          # the output starts inside the quarter-resolution gradient the launch reads
            y.buf = G.Buf('act', b.dy.buf.off, full, 'y')
        ops = [G.Op('ew2', a=a, b=b), G.Op('ew', op='maxpool_bwd', dims=full, x=a.x, dy=b.y, add=a.y, y=y, **none)]
        if second_reader:
            ops.append(G.Op('ew', op='add', dims=full, x=a.y, dy=None, add=None, y=act(full, 'z'), **dict(none, x2=y)))
    else:
        a = apply(full, 'a')
        y = act(half, 'ylow')
        if alias == 'half_input':
            low = act(half, 'low')
            y.buf = G.Buf('act', low.buf.off, half, 'ylow')
        else:
            low = act(half, 'low')
        ops = [a, G.Op('ew', op='sumpool', dims=full, x=a.y, dy=None, add=low, y=y, **none)]
    for o in ops:
        o.lane = 0
    return ops


@pytest.mark.parametrize('pattern', [1, 2])
def test_hand_made_groups_are_merged_or_declined(monkeypatch, pattern):
    from fpd_amd import executor as E, graph as G, runtime as R
    R.lib()
    monkeypatch.setenv('FPD_EW_MERGE', '1')

    def marked(ops):
        E.Lowering(FakeArenas(), 1).plan_ew_merge(ops)
        return sum(1 for o in ops if getattr(o, 'ewm_kind', None) is not None)
    assert marked(_hand_made(G, pattern=pattern)) == 1                               # the plain group is taken
    assert marked(_hand_made(G, alias='half_input', pattern=pattern)) == 0           # output over a quarter-resolution input: declined
    if pattern == 1:
        assert marked(_hand_made(G, second_reader=True)) == 0                        # a.y has a second reader: it must exist in memory
    monkeypatch.setenv('FPD_EW_MERGE', '0')
    assert marked(_hand_made(G, pattern=pattern)) == 0
