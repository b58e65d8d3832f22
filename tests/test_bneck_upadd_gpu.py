"""The frozen fused Bottleneck that forms the hourglass up-add on load (fpd_bneck_t.x2, csrc/bneck_fused.hip UPADD = true):
x'[p] = round_bf16(up1[p] + low[p / 2]) where the kernel reads its input, instead of a tensor a FPD_EW_UPADD_FWD launch wrote.

  bitwise      seeded random inputs: `ew upadd_fwd` + fpd_bottleneck_forward against the one launch with x2, as int16 views, no
               tolerance -- both round the sum once and feed the same bits to bn1 and to the residual.  Grid caps 1 and 3 make a
               block walk many tiles (ring reuse, image boundaries, the ragged last tile of (3, 8, 8));
  oracle       the dyadic inputs of tests/_teacher_cases.py (small() activations, sparse weights, unit BNs) with a small() low branch:
               the launch equals oracle/plan_interp's up-add followed by run_bneck bit for bit;
  refusals     W = 4, odd H, y aliasing x2, a pair with x2: an error before any launch;
  end to end   one teacher stack at B = 1, 256 x 256 with the option off and on: identical heat-map bytes, four launches fewer."""
import ctypes

import pytest
import torch

from oracle import plan_interp as PI
from tests import _teacher_cases as T
from tests.test_exact_gpu import exact_equal, small
from tests.test_kernels_gpu import Bench, rnd

pytestmark = pytest.mark.gpu

G = E = R = None


def setup_module(module):
    from tests import test_exact_gpu as X
    X.setup_module(X)
    global G, E, R
    from fpd_amd import executor, graph, runtime
    G, E, R = graph, executor, runtime


SHAPES = [(3, 8, 8),        # whole-image tiles, M = 192 is not a multiple of 128
          (3, 16, 16),      # two tiles per image, the ring across an image boundary
          (2, 32, 32),
          (1, 64, 64)]      # two rows per tile
_ids = lambda v: '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _clone(op, **kw):
    f = {k: v for k, v in op.__dict__.items() if k not in ('kind', 'lane')}
    f.update(kw)
    return G.Op('bneck', **f)


def _build(bt, shape, P, fold, exact):
    """-> (fold ops, up-add op, the Bottleneck reading its result, the Bottleneck with both sources, y of the two launches, y of the one)"""
    c = T.bneck_case(bt, shape, P, fold, exact)
    base = c.members[0]
    N, H, W = shape
    C = 2 * P
    gen = T.seed('tu', shape, P, exact)
    low = bt.act((N, H // 2, W // 2, C), small(gen, N, H // 2, W // 2, C) if exact else rnd(gen, N, H // 2, W // 2, C), 'low')
    xs = bt.act((N, H, W, C), torch.zeros(N, H, W, C), 'sum')
    y1 = bt.act((N, H, W, C), torch.zeros(N, H, W, C), 'y_fused')
    ua = G.Op('ew', op='upadd_fwd', dims=(N, H, W, C), x=base.x, x2=low, y=xs, out_stats=None, dy=None, add=None, bstats=None,
              dgamma=None, dbeta=None, bn=None)
    two = _clone(base, x=xs)
    one = _clone(base, y=y1, x2=low)
    return [o for o in c.ops if o.kind == 'bneck_fold'], ua, two, one, base.y, y1


def _run_gpu(bt, ops, cap=None):
    low = E.Lowering(bt.gpu, bt.dtype)
    plan = R.Plan()
    for op in ops:
        plan.add(*low.op(op))
    prev = R.set_option('bneck_blocks', cap) if cap is not None else None
    try:
        plan.run(0, len(plan))
        torch.cuda.synchronize()
    finally:
        if prev is not None:
            R.set_option('bneck_blocks', prev)


@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('P', [64, 128])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_upadd_on_load_equals_the_two_launches_bitwise(shape, P, fold):
    bt = Bench(1)
    folds, ua, two, one, y2, y1 = _build(bt, shape, P, fold, exact=False)
    bt.realise()
    _run_gpu(bt, folds)
    for cap in (1, 3):
        for y in (y2, y1, ua.y):
            bt.gpu.view(y.buf).fill_(float('nan'))           # an unwritten tile shows
        _run_gpu(bt, [ua, two], cap)
        _run_gpu(bt, [one], cap)
        a, b = bt.gpu.view(y2.buf).view(torch.int16), bt.gpu.view(y1.buf).view(torch.int16)
        assert torch.isfinite(bt.gpu.view(y2.buf).float()).all() and float(bt.gpu.view(y2.buf).float().abs().max()) > 0
        bad = torch.nonzero(a != b)
        assert bad.shape[0] == 0, 'bneck+upadd %r P=%d fold=%s cap=%d: %d/%d elements differ from the two launches, first at %s' % (
            shape, P, fold, cap, bad.shape[0], a.numel(), [int(i) for i in bad[0]])


@pytest.mark.parametrize('P', [64, 128])
@pytest.mark.parametrize('shape', [(3, 16, 16), (1, 64, 64)], ids=_ids)
def test_upadd_on_load_equals_the_specification_exactly(shape, P):
    bt = Bench(1)
    folds, ua, two, one, y2, y1 = _build(bt, shape, P, False, exact=True)
    bt.realise()
    PI.run(bt.cpu, [ua, _clone(two, y=y1)])                  # specification: the up-add, then run_bneck on its result
    bt.gpu.view(y1.buf).fill_(float('nan'))
    _run_gpu(bt, [one], 3)
    exact_equal(bt, y1, 'bneck+upadd %r P=%d' % (shape, P))


def _desc(keep, N, H, W, P=128):
    C = 2 * P
    a = R.BneckT()
    a.N, a.H, a.W, a.C, a.P, a.dtype = N, H, W, C, P, R.BF16
    t = lambda n: torch.zeros(n, dtype=torch.bfloat16, device='cuda')
    f = lambda n: torch.ones(n, dtype=torch.float32, device='cuda')
    bufs = dict(x=t(N * H * W * C), y=t(N * H * W * C), x2=t(max(1, N * (H // 2) * (W // 2) * C)), w1=t(P * C), w2=t(9 * P * P), w3=t(C * P))
    keep.append(bufs)
    for k, v in bufs.items():
        setattr(a, k, v.data_ptr())
    for bn, n in ((a.bn1, C), (a.bn2, P), (a.bn3, P)):
        v = f(n)
        keep.append(v)
        bn.mode, bn.relu, bn.eps = R.BN_EVAL, 1, 1e-5
        bn.gamma = bn.beta = bn.running_mean = bn.running_var = v.data_ptr()
    return a, bufs


def test_upadd_refusals_come_before_any_launch():
    l = R.lib()
    keep = []
    a, bufs = _desc(keep, 2, 16, 16)
    assert l.fpd_bneck_upadd_supported(ctypes.byref(a)) == 1
    bufs['y'].fill_(7.0)
    for dims, word in (((8, 4, 4), b'W must be'), ((8, 1, 16), b'H must be even')):
        b, bb = _desc(keep, *dims)
        bb['y'].fill_(7.0)
        assert l.fpd_bneck_upadd_supported(ctypes.byref(b)) == 0
        assert l.fpd_bottleneck_forward(ctypes.byref(b), R.current_stream()) < 0
        err = l.fpd_last_error()
        assert word in err and b'fpd_bneck_upadd_supported' in err, err
        torch.cuda.synchronize()
        assert bool((bb['y'].float() == 7.0).all())          # nothing was launched
    a.x2 = a.y                                               # y aliases the low branch
    assert l.fpd_bottleneck_forward(ctypes.byref(a), R.current_stream()) < 0 and b'alias x2' in l.fpd_last_error()
    a.x2 = bufs['x2'].data_ptr()
    prev = R.set_option('bneck_upadd', 0)                    # switched off: the query says no, the launch is refused
    try:
        assert l.fpd_bneck_upadd_supported(ctypes.byref(a)) == 0
        assert l.fpd_bottleneck_forward(ctypes.byref(a), R.current_stream()) < 0 and b'switched off' in l.fpd_last_error()
    finally:
        R.set_option('bneck_upadd', prev)
    p = R.BneckPairT()                                       # a pair launch takes no low branch
    p.a, p.b = a, _desc(keep, 2, 8, 8)[0]
    p.b.x2 = None
    assert l.fpd_bottleneck_forward_pair(ctypes.byref(p), R.current_stream()) < 0 and b'x2' in l.fpd_last_error()
    torch.cuda.synchronize()
    assert bool((bufs['y'].float() == 7.0).all())


def test_teacher_stack_is_unchanged_bit_for_bit(monkeypatch):
    from fpd_amd.lib.models import hourglass
    from oracle import fpd_ref, hourglass_ref
    from tests.test_fullsize_gpu import _cfg
    dev = torch.device('cuda', 0)
    J, H, W = 16, 256, 256
    teacher = hourglass.get_pose_net(_cfg(256, 1, J, 'bf16'), is_train=False)
    teacher.load_state_dict(fpd_ref.synth_state_dict(hourglass_ref.hourglass_keys(256, 1, J), 2), strict=True)
    teacher = teacher.to(dev)
    x = fpd_ref.synth_batch(100, 1, J, (W, H), (W // 4, H // 4))[0]

    def run(on):
        monkeypatch.setenv('FPD_BNECK_UPADD', '1' if on else '0')
        g = E.GraphInstance(teacher.device_state(), teacher.cfg_hg, 1, H, W, train=False).finalize()
        assert sum(1 for o in g.g.fwd if getattr(o, 'upadd_absorbed', False)) == (4 if on else 0)
        g.image().copy_(x)
        g.run('prep'); g.run('fwd')
        torch.cuda.synchronize()
        b, e = g.rng['fwd']
        return g.output_view(0).clone(), sum(1 for k in range(b, e) if g.plan.op_type(k) != R.OP_NOP)
    (m1, n1), (m0, n0) = run(True), run(False)
    assert torch.isfinite(m0.float()).all() and float(m0.float().abs().max()) > 0
    assert n0 - n1 == 4, (n0, n1)
    assert torch.equal(m1.contiguous().view(torch.int16), m0.contiguous().view(torch.int16)), 'the teacher heat-map moved'
