"""Bit-exact parity of the two halo-tile kernels -- csrc/conv_tile.hip (every stride-1 convolution of the HRNet path, of an fp32
build, and every shape the streaming kernels decline) and csrc/wgrad_tile.hip -- and of the stride-2 convolutions, on the dyadic
inputs of tests/_exact_inputs.py: both storage types, every compared buffer equal to the CPU specification (oracle/plan_interp.py)
BIT FOR BIT.  tests/test_exact_gpu.py runs conv_tile forward only, without a BatchNorm prologue, and the weight gradient with
bn=None; the random-input tests allow 3e-2 per element and 3e-2 * N*H*W on the sums, which a dropped 32-pixel wave tile passes, and
launch TN = 1 almost everywhere.  Here

  * conv_tile forward: exact train-mode BN+ReLU prologue with per-channel coefficients (or none), bias, residual, output
    statistics, on shapes that launch every reachable (T, BK, TN, ALLW) -- TN = 4 with 96 and with 128 live accumulator columns;
  * data gradient: the BatchNorm-backward epilogue (mask and both sums) unfolded and with the folded BN-backward apply (dgamma,
    dbeta, the operand written out) on every FOLD variant; where the route declines the fold (TN = 4) the same buffers come
    from the stand-alone apply;
  * pairs, forward with a prologue and as data gradients, at a power-of-two and at HRNet widths;
  * wgrad_tile_kernel in all eight instantiations, with the BN+ReLU prologue on a second and third channel tile, with slabs and
    with the single-block flush; <T, 1, 256> at its smallest legal shape (65536 pixels);
  * stride 2 (conv_mfma / conv_smallc / conv_naive and their weight gradients) forward and weight gradient, back ends 0 and 1
    (back end 2 walks the same kernels as 0 for a stride-2 shape: the halo-tile kernels decline it).

(The bf16 3x3 weight gradients that wgrad_tile's launch function hands to wgrad3 -- C = K in {32, 64}, power-of-two widths, with
slabs -- have their own file, tests/test_exact_wgrad3_gpu.py.)

Every conv_tile / wgrad_tile test asserts through the launch counters that the kernel served the launch, and that the fold was
taken exactly where fpd_conv_tile_variant() -- the route function of the launch -- says FOLD.  Which instantiation each case
launches, and that the lists reach all of them, is checked without a device by tests/test_exact_variants_cpu.py; the
preconditions of exactness by tests/test_exact_inputs_cpu.py and, on the interpreter's result, by check_reference() here."""
import ctypes

import pytest

from tests import _exact_inputs as X
from tests import test_kernels_gpu as tk
from tests.test_exact_gpu import exact_equal
from tests.test_kernels_gpu import Bench

pytestmark = pytest.mark.gpu
wmode = pytest.mark.parametrize('wmode', X.WMODES)
both = pytest.mark.parametrize('dtype', [1, 0], ids=['bf16', 'fp32'])
DT = {1: 'bf16', 0: 'fp32'}


def setup_module(module):
    tk.setup_module(tk)


def _ids(v):
    return '-'.join(str(int(e) if isinstance(e, bool) else e) for e in v if not isinstance(e, tuple)) if isinstance(v, tuple) else None


def _run(fn, params, dtype, backend='tile', partials=False):
    bt = Bench(dtype)
    b = fn(bt, *params)
    bt.realise().run(b.ops, backend, partials=partials)
    X.check_reference(bt.cpu, b, fn.__name__)
    return bt, b


def _equal(bt, b, params, *extra):
    for label, buf in b.compare + [(k, b.h[k]) for k in extra]:
        exact_equal(bt, buf, '%s %s' % (label, params))


def _struct(bt, op, ask_fold=False):
    """The convolution as the graph states it; ask_fold: as a launch that carries a fold (any non-null fold_x asks)."""
    s = tk.E.Lowering(bt.gpu, bt.dtype).conv(op, plain=True)[1]
    if ask_fold:
        s.fold_x = s.x
    return s


def _variant(bt, op, ask_fold=False):
    v = tk.R.lib().fpd_conv_tile_variant(ctypes.byref(_struct(bt, op, ask_fold)))
    assert v >= 0, 'the variant query says conv_tile declines a launch it served'
    return v


@wmode
@pytest.mark.parametrize('case,dtype', [(c, dt) for c in X.TILE_FWD for dt in c[8]], ids=lambda v: _ids(v) or DT[v])
def test_tile_forward_exact(case, dtype, wmode):
    bt, b = _run(X.tile_forward, (case, wmode), dtype)
    assert bt.n_tile == 1, 'the halo-tile kernel did not take the launch'
    _variant(bt, b.ops[0])
    _equal(bt, b, (case, DT[dtype], wmode))


@wmode
@both
@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('case', X.TILE_BWD, ids=_ids)
def test_tile_dgrad_exact(case, fold, dtype, wmode):
    """dz, both BN-backward sums, the dw / dbias of the weight-gradient launch behind it; with the fold asked for: dgamma, dbeta
    and the operand du -- evaluated inside the data gradient where the route offers FOLD, by the stand-alone apply where not."""
    bt, b = _run(X.tile_dgrad, (case, wmode, fold), dtype, partials=True)
    assert bt.n_tile == 1, 'the halo-tile kernel did not take the data gradient'
    folds = bool(_variant(bt, b.h['dg'], ask_fold=fold) >> 17 & 1)
    assert folds == (fold and case != X.TILE_BWD_TN4), 'the route says FOLD = %d' % folds
    assert (bt.n_folded == 1 and getattr(b.h['dg'], 'fold_active', False)) == folds, 'the fold was %staken, the route says FOLD = %d' % (
        '' if bt.n_folded else 'not ', folds)
    _equal(bt, b, (case, fold, DT[dtype], wmode), *(['du'] if fold else []))


@wmode
@both
@pytest.mark.parametrize('case', X.TILE_PAIR, ids=_ids)
def test_tile_pair_exact(case, dtype, wmode):
    bt, b = _run(X.tile_pair, (case, wmode), dtype)
    assert bt.n_tile == 1, 'the pair did not go out as ONE launch of the halo-tile kernel'
    p = tk.R.ConvPairT()
    p.a, p.b = _struct(bt, b.ops[-1].a), _struct(bt, b.ops[-1].b)
    assert tk.R.lib().fpd_conv_tile_pair_variant(ctypes.byref(p)) >= 0
    _equal(bt, b, (case, DT[dtype], wmode))


@pytest.mark.parametrize('case,dtype,slabs', [(c, dt, s) for c in X.TILE_WGRAD for dt in c[7] for s in X.wgrad_flushes(c)],
                         ids=lambda v: _ids(v) or ('slabs' if v is True else 'flush' if v is False else DT[v]))
def test_tile_wgrad_exact(case, dtype, slabs):
    """dw and dbias of wgrad_tile_kernel behind its BN+ReLU prologue (s_scale / s_shift are filled per channel tile c0 + c)."""
    bt, b = _run(X.tile_wgrad, (case,), dtype, partials=slabs)
    assert bt.n_wtile == 1, 'wgrad_tile_kernel did not take the launch'
    _equal(bt, b, (case, DT[dtype], slabs))


@wmode
@pytest.mark.parametrize('backend', [0, 1])
@both
@pytest.mark.parametrize('case', X.S2, ids=_ids)
def test_stride2_forward_exact(case, dtype, backend, wmode):
    bt, b = _run(X.s2_forward, (case, wmode), dtype, backend=backend)
    _equal(bt, b, (case, DT[dtype], backend, wmode))


@pytest.mark.parametrize('slabs', [True, False], ids=['slabs', 'flush'])
@pytest.mark.parametrize('backend', [0, 1])
@both
@pytest.mark.parametrize('case', X.S2, ids=_ids)
def test_stride2_wgrad_exact(case, dtype, backend, slabs):
    bt, b = _run(X.s2_wgrad, (case,), dtype, backend=backend, partials=slabs)
    _equal(bt, b, (case, DT[dtype], backend, slabs))
