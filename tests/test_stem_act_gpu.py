"""The frozen stem with bn1 + ReLU applied in its epilogue (fpd_stem_t.act, csrc/stem_s2d.hip) on the MI355X: the bits of the stem
launch followed by the elementwise BNRELU_FWD launch it replaces (the rounding of the stem's own output is kept)."""
import numpy as np
import pytest
import torch

from tests import test_kernels_gpu as tk
from tests.test_kernels_gpu import Bench, make_bn, rnd, TOL

pytestmark = pytest.mark.gpu
G = R = None


def setup_module(module):
    global G, R
    tk.setup_module(tk)
    G, R = tk.G, tk.R


def _run(case, act_option):
    N, H, W, K = case
    gen = torch.Generator().manual_seed(501 + sum(case))
    bt = Bench(1)
    P, Q = H // 2, W // 2
    img = bt.buf('image', (N, 3, H, W), rnd(gen, N, 3, H, W))
    w = bt.buf('param', (K, 7, 7, 3), rnd(gen, K, 7, 7, 3, scale=1 / np.sqrt(147)))
    b = bt.buf('param', (K,), 0.1 * rnd(gen, K))
    s = bt.act((N, P, Q, K), None, 'stem')
    a = bt.act((N, P, Q, K), None, 'stem_act')
    bn = make_bn(bt, gen, K, 'eval')                      # running statistics, gamma and beta away from (0, 1, 1, 0)
    bn.count = N * P * Q
    stem = G.Op('stem_fwd', image=img, w=w, bias=b, y=s, out_stats=None, dims=(N, H, W, K, P, Q))
    ew = G.Op('ew', op='bnrelu_fwd', dims=(N, P, Q, K), y=a, out_stats=None, x=s, x2=None, dy=None, add=None, bstats=None,
              dgamma=None, dbeta=None, bn=bn)
    stem.act_ew = ew
    ops = [stem, ew]
    bt.realise()
    tk.PI.run(bt.cpu, ops)
    prev = R.set_option('stem_act', act_option)
    try:
        low = tk.E.Lowering(bt.gpu, 1)
        low.plan_stem_act(ops)
        lowered = [low.op(o) for o in ops]
        plan = R.Plan()
        for code, st in lowered:
            plan.add(code, st)
        plan.run(0, len(plan))
        torch.cuda.synchronize()
    finally:
        R.set_option('stem_act', prev)
    return bt, a, stem, sum(1 for code, _ in lowered if code != R.OP_NOP)


# N, H, W, K: 16 tiles of 128 pixels; 32 tiles; 384 tiles over the kernel's 256 blocks (a block owns several tiles, 128-wide rows)
@pytest.mark.parametrize('case', [(2, 64, 64, 64), (4, 64, 64, 64), (3, 256, 256, 64)])
def test_stem_act_equals_stem_then_bnrelu(case):
    fused, a1, stem1, n1 = _run(case, 1)
    assert getattr(stem1, 'act_active', False) and n1 == 1, 'the stem did not take bn1 + ReLU into its epilogue'
    plain, a0, stem0, n0 = _run(case, 0)
    assert not getattr(stem0, 'act_active', False) and n0 == 2      # stem_act = 0: two launches
    fused.compare(a1, label='stem act %s' % (case,), **TOL[1])
    got, ref = fused.gpu.view(a1.buf).cpu().view(torch.int16), plain.gpu.view(a0.buf).cpu().view(torch.int16)
    assert torch.equal(got, ref), 'differs from stem + bnrelu_fwd in %d elements' % int((got != ref).sum())
    assert (fused.gpu.view(a1.buf) == 0).any() and (fused.gpu.view(a1.buf) > 0).any()      # the ReLU cuts, and not everything
