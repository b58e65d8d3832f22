"""The two persistent kernels of the frozen teacher (csrc/bneck_fused.hip, csrc/head_fused.hip) with SEVERAL TILES PER BLOCK.

Both launch under a grid cap (128 / 160 blocks); in the step (32 x 64 x 64) a Bottleneck block walks 8 consecutive tiles through
the a2 ring and a head block 7 strided ones, but every other kernel test stays below the caps: one tile per block.  Here
fpd_set_option("bneck_blocks" / "head_blocks", n) lowers the cap so that small tensors reach that regime (cases and the properties
each one is there for: tests/_teacher_cases.py; their preconditions: tests/test_teacher_cases_cpu.py).  Per case
  exact               dyadic inputs: the kernel equals the specification (oracle/plan_interp.py) bit for bit;
  grid independence   seeded random inputs: the capped launch and the launch with one tile per block give identical bytes -- a
                      tile's arithmetic does not depend on which block runs it, and ring rows that are reused hold the same bf16
                      values as recomputed ones; no tolerance;
  specification       the same random-input launch against the interpreter at the tolerances of test_bottleneck_fused /
                      test_head_fused (3e-2 absolute + 2e-2 relative, relative L2 below 3e-3);
  repeatability       one case per kernel: two runs give identical bytes."""
import os

import pytest
import torch

from tests import _teacher_cases as T
from tests.test_exact_gpu import exact_equal
from tests.test_kernels_gpu import Bench

pytestmark = pytest.mark.gpu


def setup_module(module):
    from tests import test_exact_gpu as X
    X.setup_module(X)


_ids = lambda v: '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v)
BNECK = T.bneck_params()                                                             # (shape, cap, P)
PAIRS = [(a, b, P, cap) for a, b, P, cap, _ in T.PAIR_CASES]
HEADS = [(shape, cap) for shape, cap, _ in T.HEAD_CASES]
HEADS_MULTI = [(shape, cap) for shape, cap, want in T.HEAD_CASES if 'several tiles in every block' in want]
ENV = {'bneck': 'FPD_BNECK_BLOCKS', 'head': 'FPD_HEAD_BLOCKS'}


def _backend(kernel, cap):
    """cap None: the default cap and no hook at all -- the grid the step launches"""
    if cap is None:
        if os.environ.get(ENV[kernel]):
            pytest.skip('%s is set: the default cap is not in force' % ENV[kernel])
        return 0
    return (kernel, cap)


def _launch(b, c, backend):
    """Runs the case's ops -> the bytes of every compared output (the outputs are poisoned first: an unwritten tile shows)."""
    for _, act in c.compare:
        b.gpu.view(act.buf).fill_(float('nan'))
    b.run(c.ops, backend)
    return [b.gpu.view(act.buf).view(torch.int16).clone() for _, act in c.compare]


def _exact(kernel, cap, build, label):
    b = Bench(1)
    c = build(b, True)
    b.realise()
    _launch(b, c, _backend(kernel, cap))
    for name, act in c.compare:
        exact_equal(b, act, '%s %s' % (label, name))


def _first_diff(x, y, shape):
    bad = torch.nonzero((x != y).view(shape))
    return '%d/%d elements differ, first at %s' % (bad.shape[0], x.numel(), [int(i) for i in bad[0]])


def _random(kernel, cap, tiles, build, label, repeat=False):
    b = Bench(1)
    c = build(b, False)
    b.realise()
    got = _launch(b, c, _backend(kernel, cap))
    # specification (the interpreter ran on the same arenas inside Bench.run)
    for name, act in c.compare:
        b.compare(act, 3e-2, 2e-2, '%s %s' % (label, name))
        if act.shape[-1] != T.HEAD_J:                    # (as test_head_fused: the L2 bound is stated for y / next)
            spec, dev = b.cpu.view(act.buf).float(), b.gpu.view(act.buf).float().cpu()
            rel = float((dev - spec).norm() / spec.norm())
            assert rel < 3e-3, '%s %s: relative L2 vs specification %.3e' % (label, name, rel)
    if repeat:
        again = _launch(b, c, _backend(kernel, cap))
        for (name, act), x, y in zip(c.compare, got, again):
            assert torch.equal(x, y), '%s %s: two runs differ: %s' % (label, name, _first_diff(x, y, act.shape))
    # grid independence: the cap at the tile count -> every block owns one tile
    one = _launch(b, c, (kernel, tiles))
    for (name, act), x, y in zip(c.compare, got, one):
        assert torch.equal(x, y), '%s %s: capped grid and one tile per block differ: %s' % (label, name, _first_diff(x, y, act.shape))


# ---- fused Bottleneck ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('shape,cap,P', BNECK, ids=_ids)
def test_bottleneck_persistent_exact(shape, cap, P, fold):
    _exact('bneck', cap, lambda b, ex: T.bneck_case(b, shape, P, fold, ex), 'bneck %r P=%d cap=%r fold=%s' % (shape, P, cap, fold))


@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('shape,cap,P', BNECK, ids=_ids)
def test_bottleneck_persistent_random(shape, cap, P, fold):
    _random('bneck', cap, T.ntiles(*shape), lambda b, ex: T.bneck_case(b, shape, P, fold, ex),
            'bneck %r P=%d cap=%r fold=%s' % (shape, P, cap, fold), repeat=(shape, cap, P, fold) == ((3, 32, 32), 5, 128, False))


@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('a,b,P,cap', PAIRS, ids=_ids)
def test_bottleneck_pair_persistent_exact(a, b, P, cap, fold):
    _exact('bneck', cap, lambda bt, ex: T.pair_case(bt, a, b, P, fold, ex), 'bneck2 %r + %r P=%d cap=%d fold=%s' % (a, b, P, cap, fold))


@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('a,b,P,cap', PAIRS, ids=_ids)
def test_bottleneck_pair_persistent_random(a, b, P, cap, fold):
    _random('bneck', cap, T.ntiles(*a) + T.ntiles(*b), lambda bt, ex: T.pair_case(bt, a, b, P, fold, ex),
            'bneck2 %r + %r P=%d cap=%d fold=%s' % (a, b, P, cap, fold), repeat=(P == 128 and not fold))


# ---- fused head ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('has_next', [True, False])
@pytest.mark.parametrize('shape,cap', HEADS, ids=_ids)
def test_head_persistent_exact(shape, cap, has_next, fold):
    _exact('head', cap, lambda b, ex: T.head_case(b, shape, has_next, fold, ex),
           'head %r cap=%r next=%s fold=%s' % (shape, cap, has_next, fold))


@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('has_next', [True, False])
@pytest.mark.parametrize('shape,cap', HEADS_MULTI, ids=_ids)
def test_head_persistent_random(shape, cap, has_next, fold):
    _random('head', cap, T.ntiles(*shape), lambda b, ex: T.head_case(b, shape, has_next, fold, ex),
            'head %r cap=%r next=%s fold=%s' % (shape, cap, has_next, fold), repeat=(shape, cap, fold) == ((5, 16, 16), 4, False))
