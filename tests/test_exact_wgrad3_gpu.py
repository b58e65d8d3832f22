"""Bit-exact parity of wgrad3 (csrc/wgrad3.hip, wgrad3s_kernel: the 3x3 weight and bias gradient of the student's conv2 at
C = K = 64 and C = K = 32 on 16..128-wide maps) on the dyadic inputs of tests/_exact_inputs.py: dw and dbias equal to the CPU
specification (oracle/plan_interp.py) BIT FOR BIT, no tolerance anywhere.  The random-input test of the kernel
(tests/test_kernels_gpu.py test_conv_wgrad) allows 2e-2 + 2e-5 * N*H*W per element -- a dropped 256-pixel tile, a wrong halo row
at an image border or a range that starts one tile late all pass it -- and tests/test_exact_stream_gpu.py test_c3_dgrad_exact
reaches the kernel only as the launch behind conv_c3's data gradient, at C = K = 64, at most 4 ranges and start slots 0, 2, 4.

The list X.W3_WGRAD walks the kernel's mechanisms: the ring of 2 nrows + 2 rows and its wrap, the per-k-step image row that
decides between the ring and the zero pixels (image changes inside a range, ranges that start inside an image, tiles that
STRADDLE two images), staging two tiles ahead of the multiplying waves in ranges of 1, 2 and 3 tiles, the carried last MFMA
group, both piece counts, 1 .. 64 ranges in one to eight groups of eight blocks with idle blocks, uneven fpd_cut ranges, W = 128
with its four first-row vectors per thread, launches without a BN prologue and one without a bias gradient.  What each case is
there for stands beside it in the list; tests/test_exact_wgrad3_cpu.py asserts without a device that the list reaches those
geometries and that every tile, piece and tap contributes, tests/test_exact_inputs_cpu.py the preconditions of exactness.

Every case asserts through the launch counters that wgrad3 -- and not wgrad_tile -- served the launch, and runs with the slab
workspace POISONED with NaN: a slab word the kernel leaves unwritten shows in dw after fpd_wgrad_reduce."""
import ctypes

import pytest
import torch

from tests import _exact_inputs as X
from tests import test_kernels_gpu as tk
from tests.test_exact_gpu import exact_equal
from tests.test_kernels_gpu import Bench

pytestmark = pytest.mark.gpu


def setup_module(module):
    tk.setup_module(tk)


def _ids(v):
    return '-'.join(str(int(e)) for e in v) if isinstance(v, tuple) else None


def _run(case, bias=True, partials=True):
    bt = Bench(1)
    b = X.w3_wgrad(bt, case, bias)
    bt.realise().run(b.ops, 0, partials=partials, poison_slabs=partials)
    X.check_reference(bt.cpu, b, 'w3_wgrad')
    return bt, b


def _served_by_wgrad3(bt, case):
    assert bt.n_w3 == 1 and bt.n_wtile == 0, 'wgrad3 did not take %s: %d launches of wgrad3, %d of wgrad_tile' % (case, bt.n_w3, bt.n_wtile)
    assert bt.n_partial_ops == 1, 'not ONE set of slabs'


def _equal(bt, b, label):
    for name, buf in b.compare:
        exact_equal(bt, buf, '%s %s' % (name, label))


@pytest.mark.parametrize('case', X.W3_WGRAD, ids=_ids)
def test_wgrad3_exact(case):
    bt, b = _run(case)
    _served_by_wgrad3(bt, case)
    assert [n for n, _ in b.compare] == ['dw', 'dbias']
    _equal(bt, b, case)


def test_wgrad3_without_bias_gradient_exact():
    """dbias = NULL at four pieces: the bias lanes of the ct == 0 pieces stay unused, the bias words of the (poisoned) slabs
    unwritten and unread."""
    bt, b = _run(X.W3_NO_BIAS, bias=False)
    _served_by_wgrad3(bt, X.W3_NO_BIAS)
    assert b.ops[0].dbias is None and [n for n, _ in b.compare] == ['dw']
    _equal(bt, b, (X.W3_NO_BIAS, 'no bias'))


@pytest.mark.parametrize('case', [(5, 52, 64, 64, 64, True), (3, 40, 64, 32, 32, True)], ids=_ids)
def test_wgrad3_repeatable(case):
    """Two runs into fresh benches give identical bytes (fixed-order cross-wave flush, slabs added in index order)."""
    assert case in X.W3_WGRAD
    out = []
    for _ in range(2):
        bt, b = _run(case)
        _served_by_wgrad3(bt, case)
        out.append([bt.gpu.view(buf).cpu().clone() for _, buf in b.compare])
    for (name, _), g0, g1 in zip(b.compare, *out):
        assert torch.equal(g0.contiguous().view(torch.uint8), g1.contiguous().view(torch.uint8)),'%s of %s differs between two runs' % (name, case)


def test_without_slabs_wgrad_tile_serves_and_is_exact():
    """The hand-over in the other direction: no slabs -> wgrad3 declines, wgrad_tile's single-block flush serves, bit-equal too."""
    case = (2, 64, 64, 64, 64, True)
    assert case in X.W3_WGRAD
    bt, b = _run(case, partials=False)
    assert bt.n_w3 == 0 and bt.n_wtile == 1 and bt.n_partial_ops == 0, (bt.n_w3, bt.n_wtile, bt.n_partial_ops)
    _equal(bt, b, (case, 'no slabs'))


def test_wgrad3_refuses_a_short_partial_stride():
    """partial_stride one float short of weight + bias is refused before anything is launched: error code -2, the message names the
    stride, "wgrad3_launches" does not move.  (One range, and the buffer behind `partial` has the full size.)"""
    case = (1, 16, 16, 64, 64, True)
    bt = Bench(1)
    b = X.w3_wgrad(bt, case)
    bt.realise()
    lib = tk.R.lib()
    s = tk.E.Lowering(bt.gpu, 1).wgrad(b.ops[0])[1]
    full = 64 * 9 * 64 + 64
    ws = torch.zeros(full, dtype=torch.float32, device='cuda:0')
    s.partial, s.partial_stride = ws.data_ptr(), full
    assert lib.fpd_wgrad_tile_variant(ctypes.byref(s)) == -1 and lib.fpd_wgrad_num_partials(ctypes.byref(s)) == 1
    s.partial_stride = full - 1
    n0 = tk.R.set_option('wgrad3_launches', 0)
    rc = lib.fpd_conv_wgrad(ctypes.byref(s), tk.R.current_stream())
    err = lib.fpd_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -2 and 'partial_stride %d' % (full - 1) in err, (rc, err)
    assert tk.R.set_option('wgrad3_launches', 0) == n0
    assert not bool(ws.any()), 'the refused launch wrote to the slab'
