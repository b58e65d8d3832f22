"""The lowering-time fusion protocol between graph.Op and executor.Lowering, on hand-made ops: the declared per-op state and
its defaults, the one members rule, the one reader scan (both comparison keys) and the one absorbed-op rule."""
import pytest

from fpd_amd import executor as E, graph as G, runtime as R
from tests.test_lowering_cpu import FakeArenas

# graph.Op's table: field -> default
REFS = ('fold_apply', 'fold_wgrad', 'fused_wgrad', 'skip_conv', 'act_ew', 'w8', 'w8s', 'folded', 'ewm_kind', 'ewm_full', 'ewm_half',
        'upadd_op', 'x2')
FLAGS = ('fold_active', 'fold_other_readers', 'fused_active', 'skip_active', 'skip_fused', 'act_active', 'stem_fused', 'ewm_absorbed',
         'upadd_absorbed')
ABSORBING = ('skip_fused', 'ewm_absorbed', 'upadd_absorbed', 'folded', 'stem_fused')
SHAPE = (1, 2, 2, 4)


def _act(name, buf=None):
    a = G.Act(SHAPE, name)
    a.buf = buf
    return a


def _buf(arena, off, name=''):
    return G.Buf(arena, off, (16,), name)


def _ew(name='add', **kw):
    f = dict(op=name, dims=SHAPE, x=None, x2=None, dy=None, add=None, y=None, out_stats=None, bstats=None, dgamma=None, dbeta=None,
             bn=None)
    f.update(kw)
    return G.Op('ew', **f)


def _conv(**kw):
    f = dict(x=None, w=_buf('wlp', 0), wkey='c.weight', bias=None, bkey=None, residual=None, y=None, out_stats=None, bn=None,
             epi='plain', epi_x=None, epi_bn=None, epi_stats=None, dims=(1, 2, 2, 4, 4, 1, 1, 1, 0, 2, 2))
    f.update(kw)
    return G.Op('conv', **f)


def test_members_of_a_single_op_a_pair_and_a_half_filled_pair():
    a, b = _ew(), _ew()
    assert a.members() == [a]
    for kind in ('conv2', 'ew2', 'bneck2'):
        assert G.Op(kind, a=a, b=b).members() == [a, b]
        assert G.Op(kind, a=a, b=None).members() == [a]
        assert G.Op(kind, a=None, b=None).members() == []
    x, y = _act('x', _buf('act', 0)), _act('y', _buf('act', 64))
    half = G.Op('ew2', a=_ew(x=x, y=y), b=None)          # the container rules follow it
    assert half.acts_in() == [x] and half.acts_out() == [y] and half.accesses() == ([x.buf], [y.buf])


def test_reader_scan_by_act_before_any_buffer_is_assigned():
    t, u = _act('t'), _act('u')
    r0, r1, r3 = _ew(x=t), _ew(x=u), _ew(dy=t)
    pair = G.Op('ew2', a=_ew(x=u), b=_ew(add=t))
    ops = [r0, r1, None, r3, pair]                       # a None entry is skipped and still counted
    assert list(E._readers_of(ops, t, by_buf=False)) == [(0, r0), (3, r3), (4, pair.b)]
    assert list(E._readers_of(ops, t, exclude=(r3, pair.b), by_buf=False)) == [(0, r0)]
    assert list(E._readers_of(ops, t, exclude=(pair,), by_buf=False))[-1] == (4, pair.b)      # members are excluded, not containers
    # the Buf key cannot tell unplanned tensors apart (every buf is None): why a planner that runs first compares Acts
    assert [o for _, o in E._readers_of(ops, t)] == [r0, r1, r3, pair.a, pair.b]


def test_reader_scan_by_buf_sees_a_tensor_aliased_into_another_act():
    shared = _buf('act', 0)
    t, alias, other = _act('t', shared), _act('alias', shared), _act('o', _buf('act', 0))      # `other`: an equal Buf, not the same one
    r0, r1, r2 = _ew(x=alias), _ew(x=other), _ew(x2=t)
    ops = [r0, r1, r2]
    assert list(E._readers_of(ops, t)) == [(0, r0), (2, r2)]
    assert list(E._readers_of(ops, t, exclude=(r2,))) == [(0, r0)]
    assert list(E._readers_of(ops, t, by_buf=False)) == [(2, r2)]
    assert list(E._readers_of(ops, shared)) == [(0, r0), (2, r2)]       # a Buf may be asked for directly
    assert [j for j, _ in E._readers_of([None, r1, r0, r2], t) if 1 < j < 3] == [2]      # positions serve "between"


def _fresh_ops():
    """One op of every kind that carries fusion state, no relation marked and no decision taken, with the (reads, writes) it has
    always had."""
    B = lambda n: _buf('param', 16 * n, 'b%d' % n)
    x, x2, y, r = (_act(n, _buf('act', 64 * i, n)) for i, n in enumerate(('x', 'x2', 'y', 'r')))
    bn = G.BN('bn', 'eval', 4, B(0), B(1), B(2), B(3), B(4))
    st = _buf('stats', 0)
    conv = _conv(x=x, y=y, bias=B(5), residual=r, bn=bn, out_stats=st)
    ew = _ew('upadd_fwd', x=x, x2=x2, y=y, out_stats=st)
    stem = G.Op('stem_fwd', image=B(6), w=B(7), bias=B(8), y=y, out_stats=st, dims=(1, 8, 8, 4, 4, 4))
    w = dict(w1=B(9), b1=B(10), w2=B(11), b2=B(12), w3=B(13), b3=B(14))
    bneck = G.Op('bneck', x=x, y=y, dims=(1, 2, 2, 4, 2), bn1=bn, bn2=None, bn3=None, **w)
    hw = dict(w_fc=B(9), b_fc=B(10), w_score=B(11), b_score=B(12), w_fc2=None, b_fc2=None, w_score2=None, b_score2=None)
    head = G.Op('head', y0=x, x=None, score=y, next=None, dims=(1, 2, 2, 4, 4), bn=bn, **hw)
    bnb = [bn.gamma, bn.beta, bn.rmean, bn.rvar]
    return [(conv, ([x.buf, conv.w, conv.bias, r.buf] + bnb, [y.buf, st]), [x, r], [y]),
            (ew, ([x.buf, x2.buf], [y.buf, st]), [x, x2], [y]),
            (stem, ([stem.image, stem.w, stem.bias], [y.buf, st]), [], [y]),
            (bneck, ([x.buf] + list(w.values()) + bnb, [y.buf]), [x], [y]),
            (head, ([x.buf, hw['w_fc'], hw['b_fc'], hw['w_score'], hw['b_score']] + bnb, [y.buf]), [x], [y])]


def test_a_fresh_op_has_every_declared_field_at_its_default():
    assert len(set(REFS + FLAGS)) == 22
    for f in REFS:
        assert G.Op.__dict__[f] is None, f
    for f in FLAGS:
        assert G.Op.__dict__[f] is False, f
    for op, acc, ins, outs in _fresh_ops():
        for f in REFS + FLAGS:
            want = op.x2 if (f == 'x2' and op.kind == 'ew') else (None if f in REFS else False)      # an 'ew' states its x2
            assert getattr(op, f) is want, (op.kind, f)
        assert not op.absorbed() and op.members() == [op]
        assert op.accesses() == acc, op.kind
        assert op.acts_in() == ins and op.acts_out() == outs, op.kind
    with pytest.raises(AttributeError):
        _ew().fold_actve                                  # a misspelt field is an error, not "not fused"


def test_a_relation_alone_changes_no_access_and_a_decision_does():
    (conv, acc, _, _), _, (stem, sacc, _, _) = _fresh_ops()[:3]
    sc = _conv(x=_act('sx', _buf('act', 512)), w=_buf('wlp', 64), bias=_buf('param', 512))
    conv.skip_conv = sc
    assert conv.accesses() == acc and conv.acts_in()[-1] is sc.x          # (kept alive up to conv3 whatever is decided)
    conv.skip_active = True
    assert conv.accesses() == (acc[0] + [sc.x.buf, sc.w, sc.bias], acc[1])
    ae = _ew('bnrelu_fwd', x=stem.y, y=_act('a', _buf('act', 1024)), bn=G.BN('bn1', 'eval', 4, *(_buf('param', 600 + 16 * i) for i in range(5))))
    stem.act_ew = ae
    assert stem.accesses() == sacc and stem.acts_out() == [stem.y, ae.y]
    stem.act_active = True
    assert stem.accesses() == (sacc[0] + [ae.bn.gamma, ae.bn.beta, ae.bn.rmean, ae.bn.rvar], sacc[1] + [ae.y.buf])


def test_absorbed_is_true_for_exactly_the_five_flags():
    for f in REFS + FLAGS:
        op = _ew()
        setattr(op, f, True if f in FLAGS + ('folded',) else _ew())
        assert op.absorbed() == (f in ABSORBING), f
        assert op.absorbed(merged=False) == (f in ABSORBING and f != 'ewm_absorbed'), f
    for kind in ('bneck', 'head'):                         # there `folded` is the fold table, not a decision
        assert not G.Op(kind, folded=_buf('fold', 0)).absorbed()


def test_absorbed_ops_lower_to_the_one_nop_and_plain_keeps_its_meaning():
    low = E.Lowering(FakeArenas(), R.BF16)
    x, y = _act('x', _buf('act', 0)), _act('y', _buf('act', 64))
    assert E._nop()[0] == R.OP_NOP
    for f in ABSORBING:
        op = _ew(x=x, y=y)
        setattr(op, f, True)
        assert low.ew(op)[0] == R.OP_NOP, f
        assert low.ew(op, plain=True)[0] == (R.OP_EW if f == 'ewm_absorbed' else R.OP_NOP), f     # ew_merge builds the absorbed apply's struct
    pair = G.Op('ew2', a=_ew(x=x, y=y), b=_ew(x=y, y=x))
    assert low.op(pair)[0] == R.OP_EW_PAIR
    pair.a.folded = True
    assert low.op(pair)[0] == R.OP_EW                      # a folded member leaves the pair: the other goes out alone
    pair.b.folded = True
    assert low.op(pair)[0] == R.OP_NOP
    conv = _conv(x=x, y=y)
    conv.skip_fused = True
    assert low.conv(conv)[0] == R.OP_NOP and low.conv(conv, plain=True)[0] == R.OP_CONV      # plain ignores every decision
