"""conv3 of a downsample Bottleneck with the skip 1x1 as a second source of the same launch (fpd_conv_t.x2, csrc/conv_c1.hip) on
the MI355X: against the CPU specification of the two IR ops, and bit for bit against the two launches it replaces (every
rounding point is kept: skip = round(W2 x2 + bias2), y = round((W a(x) + skip) + bias))."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_kernels_gpu as tk
from tests._skip_cases import SKIP_CASES, served
from tests.test_kernels_gpu import Bench, make_bn, rnd, tensor_stats, RS, TOL

pytestmark = pytest.mark.gpu
G = R = None


def setup_module(module):
    global G, R
    tk.setup_module(tk)
    G, R = tk.G, tk.R


class SkipBench(Bench):
    """Bench whose lowering plans the forward fusion first, as GraphInstance.finalize() does (Bench.run plans only the folds)."""

    def run(self, ops, backend, partials=False):
        if backend != 0:
            return super().run(ops, backend, partials)      # sets the kernel options, then comes back here with backend 0
        tk.PI.run(self.cpu, ops)
        low = tk.E.Lowering(self.gpu, self.dtype)
        low.plan_skips(ops)
        lowered = [low.op(op) for op in ops]
        self.n_launches = sum(1 for code, _ in lowered if code != R.OP_NOP)
        plan = R.Plan()
        for code, st in lowered:
            plan.add(code, st)
        plan.run(0, len(plan))
        torch.cuda.synchronize()


def _ops(bt, case):
    N, H, W, C, K, bn_mode, use_stats, blocks = case
    gen = torch.Generator().manual_seed(401 + sum(v for v in case if isinstance(v, int) and not isinstance(v, bool)))
    x = bt.act((N, H, W, C), rnd(gen, N, H, W, C) + 0.2, 'x')               # the Bottleneck's input: operand of the skip 1x1
    t_val = rnd(gen, N, H, W, C) + 0.3
    t = bt.act((N, H, W, C), t_val, 't')                                    # conv2's output: operand of conv3 behind bn3 + ReLU
    w2 = bt.buf('wlp', (K, 1, 1, C), rnd(gen, K, 1, 1, C, scale=1.0 / np.sqrt(C)))
    b2 = bt.buf('param', (K,), 0.1 * rnd(gen, K))
    w3 = bt.buf('wlp', (K, 1, 1, C), rnd(gen, K, 1, 1, C, scale=1.0 / np.sqrt(C)))
    b3 = bt.buf('param', (K,), 0.1 * rnd(gen, K))
    skip = bt.act((N, H, W, K), None, 'skip')
    y = bt.act((N, H, W, K), None, 'y')
    bn = make_bn(bt, gen, C, bn_mode)
    bn.count = N * H * W
    if bn_mode == 'train':
        bn.stats = bt.buf('stats', (RS, 2, C), tensor_stats(t_val.to(torch.bfloat16).float()))
    ostats = bt.buf('stats', (RS, 2, K), torch.zeros(RS, 2, K, dtype=torch.float64)) if use_stats else None
    dims = (N, H, W, C, K, 1, 1, 1, 0, H, W)
    sc = G.Op('conv', x=x, w=w2, wkey='w2', bias=b2, bkey='b2', residual=None, y=skip, out_stats=None, bn=None, epi='plain',
              epi_x=None, epi_bn=None, epi_stats=None, dims=dims)
    c3 = G.Op('conv', x=t, w=w3, wkey='w3', bias=b3, bkey='b3', residual=skip, y=y, out_stats=ostats, bn=bn, epi='plain',
              epi_x=None, epi_bn=None, epi_stats=None, dims=dims)
    c3.skip_conv = sc
    return [sc, c3], y, ostats


def _run(case, skip_option):
    bt = SkipBench(1)
    ops, y, ostats = _ops(bt, case)
    prev = R.set_option('conv_skip', skip_option)
    try:
        bt.realise().run(ops, ('c1', case[7]))
    finally:
        R.set_option('conv_skip', prev)
    return bt, ops, y, ostats


@pytest.mark.parametrize('case', SKIP_CASES)
def test_skip_fused_into_conv3(case):
    N, H, W, C, K, bn_mode, use_stats, blocks = case
    bt, ops, y, ostats = _run(case, 1)
    if served(case):
        # (d) one launch of the streaming kernel where there were two
        assert getattr(ops[1], 'skip_active', False) and getattr(ops[0], 'skip_fused', False)
        assert bt.n_launches == 1 and bt.n_c1 == 1
    else:
        # K = 256 is outside the streaming kernel's channels: the query says no and the two launches stay (on conv_tile)
        assert not getattr(ops[1], 'skip_active', False) and bt.n_launches == 2 and bt.n_c1 == 0
    # (a) against the interpreter's result of the two IR ops
    bt.compare(y, label='skip y %s' % (case,), **TOL[1])
    if use_stats:
        bt.compare(ostats, atol=TOL[1]['atol'] * N * H * W, rtol=TOL[1]['rtol'], label='skip out_stats')
    # (b) / (c) against the two launches with the fusion switched off: conv_c1 forced for C <= 64, conv_tile for K = 256
    b2, ops2, y2, ostats2 = _run(case, 0)
    assert not getattr(ops2[1], 'skip_active', False) and b2.n_launches == 2
    assert b2.n_c1 == (2 if served(case) else 0)
    got, ref = bt.gpu.view(y.buf).cpu().view(torch.int16), b2.gpu.view(y2.buf).cpu().view(torch.int16)
    assert torch.equal(got, ref), 'y differs from the two launches in %d elements' % int((got != ref).sum())
    if use_stats:
        s1, s0 = bt.gpu.stats_read(ostats).cpu().sum(0), b2.gpu.stats_read(ostats2).cpu().sum(0)
        scale = s0.abs().max(1, keepdim=True).values
        assert ((s1 - s0).abs() <= 2e-6 * scale + 1e-9).all(), float(((s1 - s0).abs() / scale).max())


def test_skip_refusals():
    """Descriptors that ask for the second source where it is not offered are refused before any kernel runs."""
    bt = SkipBench(1)
    case = (2, 32, 32, 64, 128, 'train', True, 3)
    ops, y, ostats = _ops(bt, case)
    other = bt.act((2, 32, 32, 128), torch.zeros(2, 32, 32, 128), 'other')
    bt.realise()
    low = tk.E.Lowering(bt.gpu, 1)
    l = R.lib()

    def desc():
        s = low.conv(ops[1], plain=True)[1]
        low._fill_skip(ops[1], s)
        return s
    cm = R.set_option('conv_c1', 2)
    n0 = R.set_option('conv_c1_launches', 0)
    try:
        good = desc()
        assert l.fpd_conv_skip_supported(ctypes.byref(good)) == 1
        both = desc()
        both.residual = bt.gpu.ptr(other.buf)
        c2 = desc()
        c2.C2 = 32
        bwd = desc()
        bwd.epi, bwd.bias, bwd.out_stats = R.EPI_BNRELU_BWD, None, None
        bwd.epi_x, bwd.epi_bn, bwd.epi_stats = bt.gpu.ptr(other.buf), low.bn(ops[1].bn), bt.gpu.ptr(ostats)
        bwd.bn = low.bn(None)
        for what, s in (('x2 + residual', both), ('C2 != C', c2), ('BNRELU_BWD', bwd)):
            assert l.fpd_conv_skip_supported(ctypes.byref(s)) == 0, what
            assert l.fpd_conv_forward(ctypes.byref(s), None) < 0, what
            assert b'x2' in l.fpd_last_error(), (what, l.fpd_last_error())
        pair = R.ConvPairT()
        pair.a, pair.b = desc(), desc()
        assert l.fpd_conv_forward_pair(ctypes.byref(pair), None) < 0 and b'x2' in l.fpd_last_error()
        off = R.set_option('conv_skip', 0)
        try:
            assert l.fpd_conv_skip_supported(ctypes.byref(good)) == 0
            assert l.fpd_conv_forward(ctypes.byref(good), None) < 0 and b'x2' in l.fpd_last_error()
        finally:
            R.set_option('conv_skip', off)
        torch.cuda.synchronize()
        assert R.set_option('conv_c1_launches', 0) == n0, 'a refused launch ran a kernel'
    finally:
        R.set_option('conv_c1', cm)
