"""Bit-exact parity of the kernels that carry the student chain -- conv_c1 (streaming 1x1), conv_c3 (3x3 strips) and the forced
conv_pp -- on the dyadic inputs of tests/_exact_inputs.py: bf16 storage, every compared buffer equal to the CPU specification
(oracle/plan_interp.py) BIT FOR BIT, no tolerance anywhere.  tests/test_exact_gpu.py never forces these kernels, has no
backward case and only a unit BatchNorm; the random-input tests of the kernels compare statistics to 3e-2 * N*H*W and the fused
weight gradient to 2e-2 + 2e-5 * N*H*W, which a missing 256-pixel round or a dropped 32-pixel tile passes.  Here

  * forward: exact train-mode BN+ReLU prologue with PER-CHANNEL coefficients (or none), bias, residual, output statistics;
  * data gradient: BatchNorm-backward epilogue (mask + both sums), the folded BN-backward apply (dgamma, dbeta, the materialised
    operand), the fused / separate weight and bias gradient;
  * more than 1 % of every normalised tensor has x*scale + shift == 0 exactly, so `>` against `>=` in a mask shows;
  * weights 'sparse' (fp32 == bf16 specification) and 'dense' (every MFMA fragment position live; one deterministic rounding
    of an exact fp32 accumulator);
  * shapes: one block looping over rounds, ragged last rounds, idle blocks, uneven splits, one strip, strip == image.

The conv_c1 / conv_c3 tests assert that the forced kernel served the launch; conv_pp keeps no launch counter, so its tests
assert that neither streaming kernel served it (forcing conv_pp switches both off) and, backward, that fold and fusion were
taken.  The preconditions (exact coefficients, headroom of every fp32
sum, non-degeneracy) are asserted on the interpreter's result by _exact_inputs.check_reference(), and on their own, without a
device, by tests/test_exact_inputs_cpu.py."""
import pytest

from tests import _exact_inputs as X
from tests import test_kernels_gpu as tk
from tests.test_exact_gpu import exact_equal
from tests.test_kernels_gpu import Bench

pytestmark = pytest.mark.gpu
wmode = pytest.mark.parametrize('wmode', X.WMODES)


def setup_module(module):
    tk.setup_module(tk)


def _run(fn, params, backend, partials=False):
    bt = Bench(1)
    b = fn(bt, *params)
    bt.realise().run(b.ops, backend, partials=partials)
    X.check_reference(bt.cpu, b, fn.__name__)
    return bt, b


def _equal(bt, b, params, *extra):
    for label, buf in b.compare + [(k, b.h[k]) for k in extra]:
        exact_equal(bt, buf, '%s %s' % (label, params))


@wmode
@pytest.mark.parametrize('variant', X.C1_FWD_VARIANTS, ids=lambda v: 'bn%d-res%d' % v)
@pytest.mark.parametrize('case', X.C1_FWD)
def test_c1_forward_exact(case, variant, wmode):
    bt, b = _run(X.c1_forward, (case, wmode, variant), ('c1', case[5]))
    assert bt.n_c1 == 1, 'the streaming kernel did not take the launch'
    _equal(bt, b, (case, variant, wmode))


@wmode
@pytest.mark.parametrize('fuse', [False, True])
@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('case', X.C1_BWD)
def test_c1_dgrad_exact(case, fold, fuse, wmode):
    """dz, both BN-backward sums, dw, dbias; folded: dgamma, dbeta and -- not fused -- the operand the kernel wrote out."""
    bt, b = _run(X.c1_dgrad, (case, wmode, fold, fuse), ('c1', case[5]), partials=True)
    assert bt.n_c1 == 1, 'the streaming kernel did not take the data gradient'
    if fold:
        assert bt.n_folded == 1 and getattr(b.h['dg'], 'fold_active', False), 'the BN-backward apply was not folded'
    assert bt.n_fused == (1 if fuse else 0)
    _equal(bt, b, (case, fold, fuse, wmode), *(['du'] if fold and not fuse else []))


@wmode
@pytest.mark.parametrize('case', X.C1_BWD_UNFUSED)
def test_c1_dgrad_unfused_domains_exact(case, wmode):
    """Forward convolutions 128 -> 16 and 128 -> 128: the kernel takes the data gradient, the weight gradient stays a launch of
    its own although the fusion was asked for."""
    bt, b = _run(X.c1_dgrad_unfused, (case, wmode), ('c1', case[5]), partials=True)
    assert bt.n_c1 == 1 and bt.n_fused == 0
    _equal(bt, b, (case, wmode))


@wmode
@pytest.mark.parametrize('case', X.C3_FWD)
def test_c3_forward_exact(case, wmode):
    bt, b = _run(X.c3_forward, (case, wmode), ('c3', case[4]))
    assert bt.n_c3 == 1, 'the strip kernel did not take the launch'
    _equal(bt, b, (case, wmode))


@wmode
@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('case', X.C3_BWD)
def test_c3_dgrad_exact(case, fold, wmode):
    """dz, both sums, the dw / dbias of the separate weight-gradient launch behind it; folded: dgamma, dbeta, the operand du."""
    bt, b = _run(X.c3_dgrad, (case, wmode, fold), ('c3', case[3]), partials=True)
    assert bt.n_c3 == 1, 'the strip kernel did not take the data gradient'
    assert bt.n_w3 == 1, 'the weight gradient behind it was not served by wgrad3 (tests/test_exact_wgrad3_gpu.py is its own test)'
    if fold:
        assert bt.n_folded == 1 and getattr(b.h['dg'], 'fold_active', False), 'the BN-backward apply was not folded'
    _equal(bt, b, (case, fold, wmode), *(['du'] if fold else []))


def _stream_launches():
    return tk.R.set_option('conv_c1_launches', 0), tk.R.set_option('conv_c3_launches', 0)


@wmode
@pytest.mark.parametrize('case', X.PP_FWD)
def test_pp_forward_exact(case, wmode):
    n0 = _stream_launches()
    bt, b = _run(X.pp_forward, (case, wmode), ('pp', case[8]))
    assert _stream_launches() == n0, 'a streaming kernel served a launch that conv_pp was forced for'
    _equal(bt, b, (case, wmode))


@wmode
@pytest.mark.parametrize('case', X.PP_BWD)
def test_pp_dgrad_folded_fused_exact(case, wmode):
    n0 = _stream_launches()
    bt, b = _run(X.pp_dgrad, (case, wmode), ('pp', case[5]), partials=True)
    assert _stream_launches() == n0, 'a streaming kernel served a launch that conv_pp was forced for'
    assert bt.n_folded == 1 and getattr(b.h['dg'], 'fold_active', False), 'the BN-backward apply was not folded'
    assert bt.n_fused == 1 and getattr(b.h['dg'], 'fused_active', False), 'the weight gradient was not fused'
    _equal(bt, b, (case, wmode))


@wmode
@pytest.mark.parametrize('case', X.C1_PAIR)
def test_c1_pair_exact(case, wmode):
    bt, b = _run(X.c1_pair, (case, wmode), ('c1', case[7]))
    assert bt.n_c1 == 1, 'the pair did not go out as ONE launch of the streaming kernel'
    _equal(bt, b, (case, wmode))


@wmode
@pytest.mark.parametrize('case', X.C3_PAIR)
def test_c3_pair_exact(case, wmode):
    bt, b = _run(X.c3_pair, (case, wmode), ('c3', case[5]))
    assert bt.n_c3 == 1, 'the pair did not go out as ONE launch of the strip kernel'
    _equal(bt, b, (case, wmode))
