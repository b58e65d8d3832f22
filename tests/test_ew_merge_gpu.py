"""BN-backward applies evaluated inside the pool backward that reads them (include/fpd_amd.h fpd_ew_merge_t;
executor.Lowering.plan_ew_merge) on the MI355X.  For every case: (a) the merged launch against the launches it replaces
(option ew_merge 0) -- identical BYTES in every output and in dgamma / dbeta, no tolerance, the existing kernels are the
reference; (b) against the CPU interpreter at the tolerance of the existing elementwise tests (test_kernels_gpu.TOL).
Outputs are poisoned with NaN before each run.  One case per kernel is run twice (identical bytes), one in fp32.

The pooled tensor of pattern 1 lies on a grid of multiples of 0.5 in [-2, 2] so that equal maxima inside a window -- the
tie rule (first maximum in scan order) is what a fused kernel can get wrong -- are frequent; asserted on the CPU."""
import pytest
import torch

from oracle import plan_interp as PI
from tests import _ew_merge_ops as M
from tests import test_kernels_gpu as tk

pytestmark = pytest.mark.gpu

setup_module = tk.setup_module

SHAPES = [(2, 8, 8, 128),
          (1, 2, 2, 32),          # a single window per image
          (3, 6, 10, 64),         # not a power of two; the element count is not a multiple of the block
          (1, 64, 64, 128)]       # 1 024 windows
# (has_full, add_full, add_half): both applies / the lone half-resolution apply in front of a pool backward with an ordinary
# `add` (the 128^2 case of the student) / `add` absent; the first shape also takes the remaining compiled variants
P1_VARIANTS = [(True, True, True), (False, True, True), (True, False, False)]
P1_CASES = [(s, v) for s in SHAPES for v in P1_VARIANTS] + [(SHAPES[0], v) for v in (
    (True, True, False), (True, False, True), (False, False, True), (False, True, False), (False, False, False))]
# (add_low, add of the apply)
P2_CASES = [(s, al, True) for s in SHAPES for al in (True, False)] + [(SHAPES[0], True, False), (SHAPES[0], False, False)]


def _bench(dtype, shape, salt):
    return tk.Bench(dtype), torch.Generator().manual_seed(1000 * salt + sum(shape))


def _check(bt, ops, outs, hidden, dtype, label, blocks=None, twice=False):
    """(a) + (b) of the module docstring; twice: the merged launch again, identical bytes."""
    n0, ref = M.run_gpu(bt, ops, outs, hidden, merge=False)
    assert n0 == 0
    n1, got = M.run_gpu(bt, ops, outs, hidden, merge=True, blocks=blocks)
    assert n1 == 1, '%s: the group was not merged' % label
    for b, r, g in zip(outs, ref, got):
        assert torch.isfinite(bt.gpu.view(b).float()).all(), '%s: non-finite values in %s' % (label, b.name)
        ne = int((r != g).sum())
        assert ne == 0, '%s: %d/%d elements of %s %s differ in their bytes from the un-merged launches' % (label, ne, r.numel(), b.arena, b.shape)
    if twice:
        _, again = M.run_gpu(bt, ops, outs, hidden, merge=True, blocks=blocks)
        assert all(torch.equal(a, g) for a, g in zip(again, got)), '%s: two runs differ' % label
    PI.run(bt.cpu, ops)
    cnt = ops[-1].dims[0] * ops[-1].dims[1] * ops[-1].dims[2]
    for b in outs:
        if b.arena == 'grad':          # dgamma / dbeta: sums over the pixels (the bound test_elementwise_ops uses)
            bt.compare(b, atol=tk.TOL[dtype]['atol'] * cnt, rtol=tk.TOL[dtype]['rtol'], label=label + ' dgamma/dbeta')
        else:
            bt.compare(b, label=label + ' ' + str(b.shape), **tk.TOL[dtype])


@pytest.mark.parametrize('case', P1_CASES, ids=lambda c: '%s-full%d-addf%d-addh%d' % ('x'.join(map(str, c[0])), *c[1]))
def test_apply_pair_maxpool_bwd_merged_is_bit_identical(case):
    shape, (has_full, add_full, add_half) = case
    bt, gen = _bench(1, shape, 1 + 4 * has_full + 2 * add_full + add_half)
    ops, outs, hidden, x_val = M.pool_bwd_ops(bt, gen, shape, has_full, add_full, add_half)
    assert M.max_tie_fraction(x_val) > 0.25, 'too few windows with equal maxima: %.3f' % M.max_tie_fraction(x_val)
    _check(bt.realise(), ops, outs, hidden, 1, 'maxpool_bwd %s' % (case,))


@pytest.mark.parametrize('case', P2_CASES, ids=lambda c: '%s-addlow%d-add%d' % ('x'.join(map(str, c[0])), c[1], c[2]))
def test_apply_sumpool_merged_is_bit_identical(case):
    shape, add_low, add_apply = case
    bt, gen = _bench(1, shape, 11 + 2 * add_low + add_apply)
    ops, outs, hidden, _ = M.sumpool_ops(bt, gen, shape, add_low, add_apply)
    _check(bt.realise(), ops, outs, hidden, 1, 'sumpool %s' % (case,))


@pytest.mark.parametrize('kernel', ['maxpool_bwd', 'sumpool'])
def test_merged_launch_with_several_windows_per_thread_repeats(kernel):
    """(1, 64, 64, 128) has 1 024 windows = 64 blocks of the default grid, one window per thread; capped to 24 blocks a thread
    walks two or three (a ragged last trip).  Run twice: identical bytes."""
    shape = SHAPES[3]
    bt, gen = _bench(1, shape, 21)
    ops, outs, hidden, _ = M.pool_bwd_ops(bt, gen, shape) if kernel == 'maxpool_bwd' else M.sumpool_ops(bt, gen, shape)
    _check(bt.realise(), ops, outs, hidden, 1, kernel + ' 24 blocks', blocks=24, twice=True)


@pytest.mark.parametrize('kernel', ['maxpool_bwd', 'sumpool'])
def test_merged_launch_fp32(kernel):
    shape = SHAPES[2]
    bt, gen = _bench(0, shape, 31)
    ops, outs, hidden, x_val = M.pool_bwd_ops(bt, gen, shape) if kernel == 'maxpool_bwd' else M.sumpool_ops(bt, gen, shape)
    if kernel == 'maxpool_bwd':
        assert M.max_tie_fraction(x_val) > 0.25
    _check(bt.realise(), ops, outs, hidden, 0, kernel + ' fp32', twice=True)


def test_unserved_merged_launch_is_refused_on_the_host():
    """A descriptor whose fields ask for something that is not compiled (here: an output that is also an input) is refused before
    any device call, and the query says so."""
    R = tk.R
    bt, gen = _bench(1, SHAPES[0], 41)
    ops, outs, hidden, _ = M.sumpool_ops(bt, gen, SHAPES[0])
    bt.realise()
    low = tk.E.Lowering(bt.gpu, 1)
    ops[1].ewm_kind, ops[1].ewm_full, ops[1].ewm_half = 'sumpool', ops[0], None
    s = low.ew_merge(ops[1])[1]
    assert R.lib().fpd_ew_merge_supported(R.C.byref(s)) == 1
    s.pool.y = s.full.dy
    assert R.lib().fpd_ew_merge_supported(R.C.byref(s)) == 0
    assert R.lib().fpd_ew_merge(R.C.byref(s), R.current_stream()) < 0
    assert b'output' in R.lib().fpd_last_error()
    prev = R.set_option('ew_merge', 0)
    try:
        s = low.ew_merge(ops[1])[1]
        assert R.lib().fpd_ew_merge_supported(R.C.byref(s)) == 0 and R.lib().fpd_ew_merge(R.C.byref(s), R.current_stream()) < 0
    finally:
        R.set_option('ew_merge', prev)
    torch.cuda.synchronize()
