"""Host logic of the two forward fusions, without a GPU (fake arena addresses as in tests/test_lowering_cpu.py): the downsample 1x1
of layer1 / layer2 formed inside conv3's launch (fpd_conv_t.x2) and the frozen stem's bn1 + ReLU applied in its epilogue
(fpd_stem_t.act), lowered for the benchmark teacher (hg8x256, eval) and student (hg4x128, train) at batch 32.  The teacher's
layer2 (K = 256) is outside the streaming kernel's channels and keeps its two launches: one fused skip there, two in the student."""
import ctypes

import pytest

from oracle import hourglass_ref
from tests._skip_cases import SKIP_CASES, served
from tests.test_lowering_cpu import FakeArenas


def _lower(monkeypatch, feats, stacks, train, skip='1', act='1'):
    from fpd_amd import executor as E, graph as G, runtime as R
    R.lib()
    monkeypatch.setenv('FPD_FUSE_SKIP', skip)
    monkeypatch.setenv('FPD_STEM_ACT', act)
    g = G.HourglassGraph(G.ParamTable(hourglass_ref.hourglass_keys(feats, stacks, 16)), feats, stacks, 16, 32, 256, 256, train=train,
                         wlp_is_master=False, fuse_bneck=not train, fuse_skip=True, fuse_stem_act=True)
    order = list(g.fwd)
    G.plan_memory(g.fwd + g.bwd, reuse_delay=400 if train else 0)
    low = E.Lowering(FakeArenas(), 1)
    low.train = train
    low.plan_skips(g.fwd, readers=g.fwd + g.bwd)
    low.plan_stem_act(g.fwd, readers=g.fwd + g.bwd)
    lowered = [low.op(o) for o in g.fwd]
    assert all(a is b for a, b in zip(order, g.fwd)) and len(order) == len(g.fwd)      # the IR order is unchanged
    return R, low, g, lowered


@pytest.mark.parametrize('net', [('teacher', 256, 8, False, 1), ('student', 128, 4, True, 2)])
def test_forward_lowering_fuses_the_downsample_and_the_frozen_stem(monkeypatch, net):
    name, feats, stacks, train, n_skips = net
    R, low, g, lowered = _lower(monkeypatch, feats, stacks, train)
    A = low.A
    pos = {id(o): i for i, o in enumerate(g.fwd)}
    cands = [o for o in g.fwd if o.kind == 'conv' and getattr(o, 'skip_conv', None) is not None]
    assert len(cands) == 2                                 # layer1 and layer2
    active = [o for o in cands if getattr(o, 'skip_active', False)]
    assert len(active) == n_skips
    assert sum(1 for o in g.fwd if getattr(o, 'skip_fused', False)) == n_skips
    for o in cands:
        sc, (code, s) = o.skip_conv, lowered[pos[id(o)]]
        assert pos[id(sc)] < pos[id(o)] and code == R.OP_CONV
        if o in active:
            assert lowered[pos[id(sc)]][0] == R.OP_NOP
            assert s.x2 == A.ptr(sc.x.buf) and s.w2 == A.ptr(sc.w) and s.bias2 == A.ptr(sc.bias) and s.C2 == sc.dims[3]
            assert s.residual is None
        else:
            assert lowered[pos[id(sc)]][0] == R.OP_CONV and s.x2 is None and s.residual == A.ptr(sc.y.buf)
        # x is kept alive and ordered up to conv3: every writer of a buffer that overlaps it comes after conv3 or before x's producer
        x = sc.x
        assert any(t is x for t in o.acts_in())
        lo, hi = x.buf.off, x.buf.off + x.numel
        for j, r in enumerate(g.fwd):
            for t in r.acts_out():
                if t is not x and t.buf.arena == x.buf.arena and t.buf.off < hi and lo < t.buf.off + t.numel:
                    assert j > pos[id(o)] or j < pos[id(x.producer)], 'a tensor that overlaps x is written while conv3 still reads it'
    stem = g.fwd[0]
    ew = g.fwd[1]
    assert stem.kind == 'stem_fwd' and ew.kind == 'ew' and ew.op == 'bnrelu_fwd'
    if train:                                              # train-mode bn1 needs the batch statistics first
        assert not getattr(stem, 'act_active', False) and lowered[1][0] == R.OP_EW
        assert lowered[0][1].y == A.ptr(stem.y.buf) and lowered[0][1].act.mode == R.BN_NONE
    else:
        assert getattr(stem, 'act_active', False) and lowered[1][0] == R.OP_NOP
        assert lowered[0][1].y == A.ptr(ew.y.buf) and lowered[0][1].act.mode == R.BN_EVAL and lowered[0][1].act.relu == 1
    # switched off: nothing is fused
    R2, low2, g2, lowered2 = _lower(monkeypatch, feats, stacks, train, skip='0', act='0')
    assert not any(getattr(o, 'skip_active', False) or getattr(o, 'skip_fused', False) or getattr(o, 'act_active', False) for o in g2.fwd)
    n_on, n_off = (sum(1 for c, _ in lw if c != R.OP_NOP) for lw in (lowered, lowered2))
    assert n_off - n_on == n_skips + (0 if train else 1)


@pytest.mark.parametrize('case', SKIP_CASES)
def test_skip_query_agrees_with_the_launch_route(case):
    """Pure host calls: the query for every case of the GPU test, and -- where it says no -- the launch refused before any device call."""
    from fpd_amd import runtime as R
    l = R.lib()
    N, H, W, C, K, bn_mode, use_stats, blocks = case
    s = R.ConvT()
    (s.N, s.H, s.W, s.C, s.K, s.R, s.S, s.stride, s.pad, s.P, s.Q) = (N, H, W, C, K, 1, 1, 1, 0, H, W)
    s.dtype, s.epi = R.BF16, R.EPI_PLAIN
    s.x, s.w, s.y, s.x2, s.w2, s.C2 = 1 << 40, 2 << 40, 3 << 40, 4 << 40, 5 << 40, C
    prev = R.set_option('conv_c1', 2)
    try:
        assert l.fpd_conv_skip_supported(ctypes.byref(s)) == (1 if served(case) else 0)
        if not served(case):
            assert l.fpd_conv_forward(ctypes.byref(s), None) < 0 and b'fpd_conv_skip_supported' in l.fpd_last_error()
        off = R.set_option('conv_skip', 0)
        try:
            assert l.fpd_conv_skip_supported(ctypes.byref(s)) == 0
            assert l.fpd_conv_forward(ctypes.byref(s), None) < 0 and b'fpd_conv_skip_supported' in l.fpd_last_error()
        finally:
            R.set_option('conv_skip', off)
        s.x2 = (4 << 40) + 8                               # a second source that is not 16-byte aligned
        assert l.fpd_conv_skip_supported(ctypes.byref(s)) == 0
    finally:
        R.set_option('conv_c1', prev)


def test_stem_act_query(monkeypatch):
    from fpd_amd import runtime as R
    l = R.lib()
    s = R.StemT()
    (s.N, s.H, s.W, s.K, s.P, s.Q, s.dtype) = (32, 256, 256, 64, 128, 128, R.BF16)
    s.x, s.w, s.bias, s.y = 1 << 40, 2 << 40, 3 << 40, 4 << 40
    assert l.fpd_stem_act_supported(ctypes.byref(s)) == 0                       # no act asked for
    s.act.mode, s.act.relu, s.act.eps = R.BN_EVAL, 1, 1e-5
    s.act.gamma, s.act.beta, s.act.running_mean, s.act.running_var = 5 << 40, 6 << 40, 7 << 40, 8 << 40
    assert l.fpd_stem_act_supported(ctypes.byref(s)) == 1
    s.out_stats = 9 << 40                                                       # statistics of the un-normalised map: not with act
    assert l.fpd_stem_act_supported(ctypes.byref(s)) == 0
    assert l.fpd_stem_forward(ctypes.byref(s), None) < 0 and b'fpd_stem_act_supported' in l.fpd_last_error()
    s.out_stats = None
    s.act.mode = R.BN_TRAIN
    assert l.fpd_stem_act_supported(ctypes.byref(s)) == 0
    s.act.mode, s.K = R.BN_EVAL, 128                                            # the im2col / plain stems decline
    assert l.fpd_stem_act_supported(ctypes.byref(s)) == 0
    s.K = 64
    prev = R.set_backend(R.BACKEND_NAIVE)
    try:
        assert l.fpd_stem_act_supported(ctypes.byref(s)) == 0
    finally:
        R.set_backend(prev)
    prev = R.set_option('stem_act', 0)
    try:
        assert l.fpd_stem_act_supported(ctypes.byref(s)) == 0
    finally:
        R.set_option('stem_act', prev)
