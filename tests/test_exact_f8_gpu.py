"""Bit-exact parity of the fp8 forward convolution (csrc/conv_tile_f8.hip, BASELINE configs[4] "HRNet-W32 student fp8 weights")
with its specification (oracle/fp8_ref.py through oracle/plan_interp.py) on the inputs of tests/_f8_cases.py, in every one of
the six compiled instantiations TN {1, 2, 4} x BK {32, 64}.  tests/test_fp8_gpu.py compares N(0.3, 1) inputs at 6e-3 + 6e-3:
it launches TN4 and (TN2, BK32) never, its operands neither saturate nor sit on a rounding tie, and a fall-back to the bf16
kernel shows there only as a statistic.  Here

  * the operand quantiser alone: all 65536 bf16 bit patterns (NaN aside) through clamp + cvt on the way into LDS, on both chunk
    widths, without a prologue and behind an identity BatchNorm without and with ReLU -- saturation (+-inf included), every
    tie, the subnormal range, the sign and each of the eight positions of a packed vector;
  * F8_EXACT through the plan path of test_conv_forward_f8 (wprep + wquant + OP_CONV_F8), 'sparse' and 'dense' filters with a
    different power-of-two scale per output channel: y and the output statistics BIT FOR BIT, the device-quantised weights
    and scales equal to the specification's.  Operands that the e4m3 rounding changes make the result differ from the bf16
    convolution's in more than 1 % of the elements (tests/test_f8_cases_cpu.py asserts it), so a silent fall-back fails here;
  * one case per instantiation twice: identical bytes.

Which instantiation a case launches is the library's answer (fpd_conv_f8_variant, the route function of the launch); that the
list reaches all six, and the preconditions of exactness, are checked without a device by tests/test_f8_cases_cpu.py and, on
the interpreter's result, by check_f8() here."""
import ctypes

import pytest
import torch

from oracle import fp8_ref, plan_interp as PI
from tests import _f8_cases as F8
from tests import test_kernels_gpu as tk
from tests.test_exact_gpu import exact_equal
from tests.test_kernels_gpu import Bench

pytestmark = pytest.mark.gpu
wmode = pytest.mark.parametrize('wmode', F8.WMODES)


def setup_module(module):
    tk.setup_module(tk)


def _ids(c):
    return '-'.join(str(int(v) if isinstance(v, bool) else v) for v in c)


def _run(build, *params):
    """Quantise the master weights on the device, then the convolution as OP_CONV_F8; the interpreter quantises on the fly."""
    bt = Bench(1)
    b = build(bt, *params)
    bt.sizes['w8'] = (bt.sizes['w8'] + 15) // 16 * 16
    bt.realise()
    low = tk.E.Lowering(bt.gpu, 1)
    plan = tk.R.Plan()
    plan.add(*low.wprep([(b.h['wm'], b.h['w'], None)]))
    plan.add(*low.wquant([(b.h['wm'], b.h['w8'], b.h['w8s'])]))
    code, st = low.op(b.h['op'])
    assert code == tk.R.OP_CONV_F8
    v = tk.R.lib().fpd_conv_f8_variant(ctypes.byref(st.c))
    assert v >= 0 and tk.R.lib().fpd_conv_f8_in_domain(ctypes.byref(st.c)) == 1, 'the fp8 kernel declines the launch'
    plan.add(code, st)
    plan.run(0, len(plan))
    torch.cuda.synchronize()
    PI.run(bt.cpu, b.ops)
    return bt, b, v


def _weights_equal(bt, b, label):
    """The e4m3 bytes and scales the device wrote are the specification's (tests/test_fp8_gpu.py test_weight_quantisation_is_exact)."""
    wm = bt.cpu.view(b.h['wm']).float()
    q, scale = fp8_ref.quant_weights(wm)
    assert torch.equal(bt.gpu.view(b.h['w8s']).cpu(), scale), label + ': weight scales'
    got = bt.gpu.view(b.h['w8']).cpu().view(torch.float8_e4m3fn).float().reshape(wm.shape)
    assert torch.equal(got, q), '%s: %d e4m3 weights differ' % (label, int((got != q).sum()))


@pytest.mark.parametrize('prologue', F8.SWEEP_PROLOGUES, ids=str)
@pytest.mark.parametrize('shape', F8.SWEEP, ids=_ids)
def test_operand_quantiser_on_every_bf16_pattern(shape, prologue):
    bt, b, v = _run(F8.f8_sweep, shape, prologue)
    assert v >> 4 == shape[3], F8.variant_name(v)
    _weights_equal(bt, b, 'sweep')
    want = bt.cpu.view(b.h['op'].y.buf).float().reshape(-1)
    got = bt.gpu.view(b.h['op'].y.buf).float().cpu().reshape(-1)
    bad = torch.nonzero(got != want).reshape(-1)          # (values: -0 equals +0)
    x = F8.sweep_patterns()
    assert bad.numel() == 0, 'sweep %s %s (%s): %d patterns differ, first 0x%04x (x = %r): y = %r, specification %r' % (
        shape, prologue, F8.variant_name(v), bad.numel(), int(F8.sweep_bits()[bad[0]]), float(x[bad[0]]), float(got[bad[0]]), float(want[bad[0]]))
    assert float(want.max()) == 196.0


@wmode
@pytest.mark.parametrize('case', F8.F8_EXACT, ids=_ids)
def test_conv_f8_exact(case, wmode):
    bt, b, v = _run(F8.f8_forward, case, wmode)
    label = 'conv_f8 %s %s %s' % (case, wmode, F8.variant_name(v))
    m = F8.check_f8(bt.cpu, b, label)
    assert m['changed'] >= 0.01 and m['down'] > 0 and m['up'] > 0, m
    _weights_equal(bt, b, label)
    for name, buf in b.compare:
        exact_equal(bt, buf, '%s %s' % (name, label))


def _one_case_per_variant():
    seen = {}
    for c in F8.F8_EXACT:
        if all((c, m) not in F8.NO_STATS for m in F8.WMODES):
            seen.setdefault(F8.route(*c[:6]), c)
    assert set(seen) == F8.VARIANTS
    return [seen[v] for v in sorted(seen)]


@pytest.mark.parametrize('case', _one_case_per_variant(), ids=_ids)
def test_conv_f8_is_repeatable(case):
    """The same launch twice (fresh arenas): identical bytes in y and in the statistics limbs."""
    runs = []
    for _ in range(2):
        bt, b, v = _run(F8.f8_forward, case, 'dense')
        runs.append([bt.gpu.view(buf.buf if hasattr(buf, 'buf') else buf).cpu().clone() for _, buf in b.compare])
    assert len(runs[0]) == 2, 'y and out_stats'
    for (name, _), t0, t1 in zip(b.compare, *runs):
        assert torch.equal(t0.view(torch.uint8), t1.view(torch.uint8)), '%s of %s (%s) differs between two runs' % (name, case, F8.variant_name(v))

