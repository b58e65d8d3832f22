"""Bit-exact parity of the stem -- Conv2d(3, K, 7, stride 2, pad 3) on the fp32 NCHW image, the only op with three hand-written
back ends for one arithmetic (csrc/stem_s2d.hip, csrc/stem_mfma.hip, csrc/stem.hip) -- on the dyadic inputs of
tests/_exact_inputs.py: every compared buffer equals the CPU specification (oracle/plan_interp.py) BIT FOR BIT.

The random-input tests (test_kernels_gpu.py test_stem, test_stem_act_gpu.py) build P, Q = H // 2, W // 2 from even sizes, so
the space-to-depth kernels take every bf16 shape the im2col kernels would: stem_fwd_mfma_kernel<1> / <2> and
stem_wgrad_mfma_kernel<32> are never launched there, nor is stem_s2d_fwd_kernel<1, true>; their persistent forward owns one
tile per block except in one case judged at 3e-2, and their dw tolerance (2e-2 + 2e-5 * N*P*Q on gradients of scale 0.1) passes
a dropped halo row, a live tap in the tap-less slot of the 4x4x16 phase table, a column over-read in the weight gradient's
funnel shift or a missing tile.  Here

  * the "stem_blocks" option caps the grids, so that a block owns several tiles on a 256..768-pixel tensor: ring continuation
    and wrap, the full reload at an image change, a block that starts in the middle of an image, uneven tile ranges;
  * odd H or W sends the same (P, Q) to the im2col kernels, non-power-of-two Q / fp32 / the direct back end to the direct ones;
  * every test asserts through "stem_s2d_launches" / "stem_mfma_launches" which kernel family served (neither: the direct one);
  * forward with and without output statistics, weights 'sparse' and 'dense'; the frozen bn1 + ReLU epilogue against the
    interpreter's stem + bnrelu_fwd with one launch going out; the weight gradient straight into dw by ONE block walking every
    tile, as slabs at the default count, and as slabs under a cap with the query checked against min(tiles, blocks).

The preconditions (bf16-representable operands, headroom of every fp32 sum -- those of y shifted by the bias included --, exact
BN coefficients, mask shares) are asserted on the interpreter's result by _exact_inputs.check_reference(), and without a device
by tests/test_exact_inputs_cpu.py."""
import ctypes as C

import pytest
import torch

from tests import _exact_inputs as X
from tests import test_kernels_gpu as tk
from tests.test_exact_gpu import exact_equal
from tests.test_kernels_gpu import Bench

pytestmark = pytest.mark.gpu
wmode = pytest.mark.parametrize('wmode', X.WMODES)
stats = pytest.mark.parametrize('stats', [True, False], ids=['stats', 'nostats'])
S2D, MFMA, DIRECT = (1, 0), (0, 1), (0, 0)      # (space-to-depth, im2col) launches of ONE stem op


def _id(case):                                  # (N, H, W, K, blocks)
    return '-'.join(map(str, case))


def setup_module(module):
    tk.setup_module(tk)


def _served():
    return tk.R.set_option('stem_s2d_launches', 0), tk.R.set_option('stem_mfma_launches', 0)


def _run(fn, params, dtype=1, backend=0, blocks=0, slabs=False):
    """Interpreter and device over the ops of fn(bench, *params), the stem lowered as a plan lowers it (plan_stem_act, slabs +
    'wreduce' for the weight gradient).  -> bench, Built, (s2d, im2col) launches served, launches of the plan, slabs written"""
    G, E, R = tk.G, tk.E, tk.R
    bt = Bench(dtype)
    b = fn(bt, *params)
    ops = list(b.ops)
    wg = [o for o in ops if o.kind == 'stem_wgrad']
    if slabs:
        ops.append(G.Op('wreduce', bucket=0, wgrads=wg, bufs=[wg[0].dw, wg[0].dbias]))
    bt.realise()
    tk.PI.run(bt.cpu, ops)
    X.check_reference(bt.cpu, b, fn.__name__)
    prev_blocks, prev_backend = R.set_option('stem_blocks', blocks), R.set_backend(backend)
    try:
        low = E.Lowering(bt.gpu, dtype)
        low.use_partials = slabs
        low.plan_stem_act(ops)
        lowered = [low.op(o) for o in ops]
        low.finish_partials()
        n_slabs = low.partials[id(wg[0])].n if slabs else 0
        if slabs:
            assert n_slabs == R.lib().fpd_stem_wgrad_num_partials(C.byref(low.partials[id(wg[0])].s)), 'the query changed its answer'
        plan = R.Plan()
        for code, st in lowered:
            plan.add(code, st)
        n0 = _served()
        plan.run(0, len(plan))
        torch.cuda.synchronize()
        n1 = _served()
    finally:
        R.set_option('stem_blocks', prev_blocks)
        R.set_backend(prev_backend)
    return bt, b, (n1[0] - n0[0], n1[1] - n0[1]), sum(1 for code, _ in lowered if code != R.OP_NOP), n_slabs


def _equal(bt, b, params):
    for label, buf in b.compare:
        exact_equal(bt, buf, '%s %s' % (label, params))


def _forward(case, wmode, stats, family, dtype=1, backend=0):
    bt, b, served, _, _ = _run(X.stem_forward, (case, wmode, stats), dtype, backend, case[4])
    assert served == family, 'served by (s2d, im2col) = %s launches, expected %s' % (served, family)
    _equal(bt, b, (case, wmode, stats, dtype, backend))


@wmode
@stats
@pytest.mark.parametrize('case', X.STEM_S2D, ids=_id)
def test_stem_s2d_forward_exact(case, stats, wmode):
    """stem_s2d_fwd_kernel<1, false> (K <= 32) / <2, false>: y and, kept per lane over all tiles of a block, its statistics."""
    _forward(case, wmode, stats, S2D)


@wmode
@pytest.mark.parametrize('case', X.STEM_ACT, ids=_id)
def test_stem_s2d_act_exact(case, wmode):
    """stem_s2d_fwd_kernel<1, true> (K = 8, 32) / <2, true> (K = 40, 64): ONE launch writes relu(bn1(stem)); a channel in 16 sits
    on the ReLU boundary as a whole."""
    bt, b, served, launches, _ = _run(X.stem_act, (case, wmode), blocks=case[4])
    assert getattr(b.h['stem'], 'act_active', False) and launches == 1, 'the stem did not take bn1 + ReLU into its epilogue'
    assert served == S2D
    _equal(bt, b, (case, wmode))


@wmode
@stats
@pytest.mark.parametrize('case', X.STEM_MFMA, ids=_id)
def test_stem_mfma_forward_exact(case, stats, wmode):
    """stem_fwd_mfma_kernel<1> (K = 8, 32) / <2> (K = 40, 64): reachable only with an odd H or W."""
    _forward(case, wmode, stats, MFMA)


@wmode
@stats
@pytest.mark.parametrize('case', X.STEM_DIRECT, ids=lambda c: '-'.join(map(str, c[:4])) + '-%s-backend%d' % ('bf16' if c[4] else 'fp32', c[5]))
def test_stem_direct_forward_exact(case, stats, wmode):
    """stem_fwd_kernel<bf16_t> / <float>: shapes the matrix-core kernels decline, fp32 storage, the direct back end."""
    _forward(case[:4] + (0,), wmode, stats, DIRECT, dtype=case[4], backend=case[5])


def _tiles(case, family):
    N, H, W, K, P, Q = X.stem_dims(*case[:4])
    return N * -(-P // 8) * -(-Q // 16) if family == DIRECT else N * P * Q // 128


def _wgrad(case, mode, family, dtype=1):
    """mode 'one': no slabs, ONE block walks every tile and adds into dw; 'slabs': the default slab count + 'wreduce'; 'cap': slabs
    under "stem_blocks" = case[4]."""
    blocks = case[4] if mode == 'cap' else 0
    bt, b, served, _, n_slabs = _run(X.stem_wgrad, (case,), dtype, 0, blocks, slabs=mode != 'one')
    assert served == family, 'served by (s2d, im2col) = %s launches, expected %s' % (served, family)
    if mode == 'cap':
        assert n_slabs == min(_tiles(case, family), blocks), 'fpd_stem_wgrad_num_partials: %d slabs for %d tiles under a cap of %d' % (
            n_slabs, _tiles(case, family), blocks)
    elif mode == 'slabs':
        assert n_slabs == _tiles(case, family)            # (every case has fewer tiles than any default cap)
    _equal(bt, b, (case, mode, dtype))


modes = pytest.mark.parametrize('mode', ['one', 'slabs', 'cap'])


@modes
@pytest.mark.parametrize('case', X.STEM_WGRAD_S2D, ids=_id)
def test_stem_s2d_wgrad_exact(case, mode):
    _wgrad(case, mode, S2D)


@modes
@pytest.mark.parametrize('case', X.STEM_WGRAD_MFMA, ids=_id)
def test_stem_mfma_wgrad_exact(case, mode):
    """stem_wgrad_mfma_kernel<32> (odd sizes, K = 8, 32) / <64> (K = 40, 64: the space-to-depth form stops at K = 32)."""
    _wgrad(case, mode, MFMA)


@modes
@pytest.mark.parametrize('case', X.STEM_WGRAD_DIRECT, ids=lambda c: '-'.join(map(str, c[:5])) + ('-bf16' if c[5] else '-fp32'))
def test_stem_direct_wgrad_exact(case, mode):
    _wgrad(case, mode, DIRECT, dtype=case[5])
