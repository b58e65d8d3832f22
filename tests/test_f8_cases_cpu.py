"""The bit-exact fp8 convolution tests (tests/test_exact_f8_gpu.py) without a device: which instantiation of
csrc/conv_tile_f8.hip every case of tests/_f8_cases.py F8_EXACT launches -- asked of the library, fpd_conv_f8_variant() answers
through the route function the launch walks -- and the preconditions that make a bit-for-bit comparison legitimate AND
worth having (check_f8(): exact weight quantisation under power-of-two scales, headroom of the accumulator and of both
statistics sums; here: the e4m3 rounding is live, ties go both ways, the result is not the bf16 convolution's).

A list that stops reaching one of the six compiled (TN, BK), or an operand draw that the e4m3 rounding leaves alone, fails here by
name before any device is involved."""
import ctypes
import itertools

import pytest
import torch

from tests import _exact_inputs as X
from tests import _f8_cases as F8


@pytest.fixture(scope='module')
def R():
    from fpd_amd import runtime
    runtime.lib()
    return runtime


def _variant(R, *dims, **kw):
    return R.lib().fpd_conv_f8_variant(ctypes.byref(F8.conv_struct(R, *dims, **kw)))


def test_cases_reach_every_compiled_variant(R):
    got = {}
    for c in F8.F8_EXACT:
        v = _variant(R, *c[:6])
        assert v >= 0, 'the fp8 kernel declines %s' % (c,)
        assert v == F8.route(*c[:6]), '%s: the library says %s, the restatement %s' % (c, F8.variant_name(v), F8.variant_name(F8.route(*c[:6])))
        got.setdefault(v, []).append(c)
    assert set(got) == F8.VARIANTS, 'no exact case launches: ' + '; '.join(F8.variant_name(v) for v in sorted(F8.VARIANTS - set(got)))
    for v, cases in got.items():
        assert any((c, 'dense') not in F8.NO_STATS for c in cases), '%s: no dense case compares the output statistics' % F8.variant_name(v)
        assert {c[5] for c in cases} == {1, 3}, '%s: 1x1 and 3x3' % F8.variant_name(v)
    for c in F8.F8_EXACT:
        assert any((c, m) not in F8.NO_STATS for m in F8.WMODES), '%s never compares its statistics' % (c,)
    # what the list varies
    assert {c[6] for c in F8.F8_EXACT} == {'train', 'eval', None} and {c[7] for c in F8.F8_EXACT} == {True, False} == {c[8] for c in F8.F8_EXACT}
    assert {v >> 4 for v, cs in got.items() if any(c[9] for c in cs)} == {32, 64}, 'operands beyond 448 on both chunk widths'
    rows = lambda c: max(1, 128 // c[2])
    assert any(c[0] * c[1] % rows(c) for c in F8.F8_EXACT), 'no case whose last tile ends inside the tensor'
    assert any(c[1] % rows(c) and c[0] > 1 for c in F8.F8_EXACT), 'no case whose tiles span images'


def test_sweep_shapes_are_one_chunk_of_each_width(R):
    assert [_variant(R, n, h, w, c, c, 1) >> 4 for n, h, w, c in F8.SWEEP] == [32, 64]
    assert all(n * h * w * c == 65536 for n, h, w, c in F8.SWEEP)


def test_restated_route_equals_the_library(R):
    """... around the switch points of TN (K = 32 / 64 and the 128-block rule), on every map width class, both chunk widths, and
    outside the domain: the query is -1 exactly where fpd_conv_f8_in_domain() is 0."""
    lib, seen = R.lib(), set()
    maps = [(1, 1), (7, 1), (8, 6), (16, 16), (32, 24), (43, 128), (64, 48), (64, 64), (96, 72), (127, 2), (128, 128), (31, 43), (3, 129), (16, 96)]
    rows = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    chans = (16, 32, 64, 96, 128, 512, 544)
    outs = (4, 8, 24, 32, 40, 64, 72, 96, 128, 136, 256, 264, 488, 512)
    for (H, W), C, K, r, stride in itertools.product(maps, chans, outs, (1, 3, 5), (1, 2)):
        for N in sorted({1, 2, 5} | {max(1, -(-g * max(1, 128 // W) // H)) for g in rows}):
            a = F8.conv_struct(R, N, H, W, C, K, r, stride)
            v = lib.fpd_conv_f8_variant(ctypes.byref(a))
            assert v == F8.route(N, H, W, C, K, r, stride), ((N, H, W, C, K, r, stride), F8.variant_name(v))
            assert (v == -1) == (lib.fpd_conv_f8_in_domain(ctypes.byref(a)) == 0)
            seen.add(v)
    assert seen == F8.VARIANTS | {-1}
    a = F8.conv_struct(R, 2, 16, 16, 64, 64, 3)
    a.dtype = R.F32
    assert lib.fpd_conv_f8_variant(ctypes.byref(a)) == -1 and lib.fpd_conv_f8_in_domain(ctypes.byref(a)) == 0
    a.dtype, a.epi = R.BF16, R.EPI_BNRELU_BWD
    assert lib.fpd_conv_f8_variant(ctypes.byref(a)) == -1 and lib.fpd_conv_f8_in_domain(ctypes.byref(a)) == 0


@pytest.mark.parametrize('wmode', F8.WMODES)
@pytest.mark.parametrize('case', F8.F8_EXACT, ids=lambda c: '-'.join(str(v) for v in c))
def test_case_is_exact_and_worth_running(case, wmode):
    bt = X.CpuBench(1)
    b = F8.f8_forward(bt, case, wmode)
    bt.realise().run(b.ops)
    m = F8.check_f8(bt.cpu, b, 'f8_forward %s %s' % (case, wmode))
    assert (b.h['op'].out_stats is None) == ((case, wmode) in F8.NO_STATS)
    assert m['changed'] >= 0.01, 'the e4m3 rounding changes only %.2f %% of the operand' % (100 * m['changed'])
    assert m['down'] > 0 and m['up'] > 0, 'ties to even: %d down, %d up' % (m['down'], m['up'])
    assert (m['big'] > 0) == case[9], '%d operands beyond 448' % m['big']
    y8 = bt.cpu.view(b.h['op'].y.buf).float().clone()
    differ = float((F8.bf16_output(bt, b) != y8).float().mean())
    assert differ >= 0.01, 'only %.2f %% of y differs from the bf16 convolution' % (100 * differ)
    assert torch.equal(bt.cpu.view(b.h['op'].y.buf).float(), y8)


def test_plain_draw_would_not_tell_fp8_from_bf16():
    """The draws of tests/_exact_inputs.py alone -- small() behind exact_bn() -- have only e4m3-representable operands (this is
    what the sprinkled values of f8_operand() are for)."""
    bt = X.CpuBench(1)
    gen = X.seed('plain')
    b = X.Built()
    bn = b.bn(bt, gen, 64, 512)
    x = bt.act((2, 16, 16, 64), F8.small(gen, 2, 16, 16, 64), 'x')
    op = X.G.Op('conv', x=x, bn=bn)
    bt.realise()
    v, vq = F8.operand(bt.cpu, op)
    assert torch.equal(v, vq) and float(v.max()) <= 4.0


@pytest.mark.parametrize('shape', F8.SWEEP, ids=str)
@pytest.mark.parametrize('prologue', F8.SWEEP_PROLOGUES, ids=str)
def test_sweep_reference(shape, prologue):
    """y == e4m3(prologue(x)) * 7/16 exactly, in bf16, for every bit pattern; +-inf saturate; 253 distinct grid values."""
    from oracle import fp8_ref
    bt = X.CpuBench(1)
    b = F8.f8_sweep(bt, shape, prologue)
    bt.realise().run(b.ops)
    x = F8.sweep_patterns()
    if prologue and prologue.endswith('relu'):
        x = x.clamp_min(0)
    want = fp8_ref.quant_e4m3(x) * 0.4375
    y = bt.cpu.view(b.h['op'].y.buf).float().reshape(-1)
    assert torch.equal(y, want) and torch.equal(want.bfloat16().float(), want)
    assert int(torch.unique(want).numel()) == (127 if prologue and prologue.endswith('relu') else 253)
    assert float(want.max()) == 196.0 and (prologue and prologue.endswith('relu') or float(want.min()) == -196.0)
    q, scale = fp8_ref.quant_weights(bt.cpu.view(b.h['wm']).float())
    assert bool((scale == 2.0 ** -10).all()) and float(q.abs().max()) == 448.0
    xo, xq = F8.operand(bt.cpu, b.h['op'])
    down, up = F8.ties(xo, xq)
    assert down >= 32 and up >= 32          # (four midpoints each way per binade and sign)
    # any two of the eight positions of a packed vector hold different e4m3 values in more than a tenth of the 8192 vectors (most
    # patterns are below the e4m3 range or beyond it): bytes that change places show
    v8 = xq.reshape(-1, 8)
    for i, j in itertools.combinations(range(8), 2):
        assert float((v8[:, i] != v8[:, j]).float().mean()) > 0.1, (i, j)
