"""The default dispatch on the MI355X at its boundaries: data gradients behind a BN-backward apply (tests/_fold_ops.py), with
and without the apply attached (fold) and the weight gradient attached (fuse), lowered the way the executor lowers them --
the library's queries decide what is folded and fused -- and run through the C ABI.  Every case must run (a query that
promises a fold the launch cannot make fails on the host, before anything is launched), take the route pinned in ROUTES,
and match the specification (oracle/plan_interp.py, bf16 storage: the same rounding points) with the suite's tolerances.

Cases sit on both sides of conv_c1's data-gradient threshold (2048 pixels), conv_pp's (256 pixel tiles), conv_c3's (32768
pixels, and shapes outside its domain), and conv_tile's fold limit (TN <= 2: 128 -> 128 and 16 -> 128 data gradients between
them have no folded route), plus the benchmark student's own data gradients at batch 32 and pairs on two map sizes.  Shapes are
named as data gradients: N HxW Cin -> Cout RxR (the forward convolution is Cout -> Cin)."""
import itertools

import pytest
import torch

from tests import test_kernels_gpu as tk
from tests._fold_ops import bn_backward_dgrad_ops
from tests.test_kernels_gpu import Bench, TOL

pytestmark = pytest.mark.gpu
G = R = None

# (N, H, W, Cin, Cout, R) of the data-gradient launch
SINGLES = [
    # conv_c1's data-gradient threshold: 1024 / 2048 pixels
    (1, 32, 32, 128, 64, 1), (2, 32, 32, 128, 64, 1), (1, 32, 32, 64, 128, 1), (2, 32, 32, 64, 128, 1),
    # conv_pp's threshold: 1x1 128 -> 16 (outside conv_c1) at 240 / 256 tiles of 4 rows; 3x3 64 -> 64 on 48-wide rows (outside
    # conv_c3) at 240 / 264 tiles of 2 rows; folded 128 -> 128 at 224 tiles (no folded route: goes out unfolded)
    (15, 64, 64, 128, 16, 1), (16, 64, 64, 128, 16, 1), (10, 48, 48, 64, 64, 3), (11, 48, 48, 64, 64, 3), (7, 64, 64, 128, 128, 1),
    # conv_c3: 16384 / 32768 pixels; 128-wide rows (outside its domain, and conv_pp's: conv_tile); 36 rows of 32 (not whole strips)
    (4, 64, 64, 64, 64, 3), (8, 64, 64, 64, 64, 3), (2, 128, 128, 64, 64, 3), (32, 36, 32, 64, 64, 3),
    # conv_tile's fold limit: 16384 pixels of 128 -> 128 and 16 -> 128 (128 tiles at TN = 4), and from 256 tiles (conv_pp folds)
    (1, 128, 128, 128, 128, 1), (4, 64, 64, 128, 128, 1), (16, 32, 32, 128, 128, 1),
    (1, 128, 128, 16, 128, 1), (4, 64, 64, 16, 128, 1), (16, 32, 32, 16, 128, 1),
    (8, 64, 64, 128, 128, 1), (8, 64, 64, 16, 128, 1),
    # the benchmark student at batch 32: Bottleneck data gradients on every level, fc_ (128 -> 128) and score_ (16 -> 128)
    (32, 64, 64, 128, 64, 1), (32, 64, 64, 64, 128, 1), (32, 64, 64, 64, 64, 3),
    (32, 32, 32, 128, 64, 1), (32, 32, 32, 64, 128, 1), (32, 32, 32, 64, 64, 3),
    (32, 16, 16, 128, 64, 1), (32, 16, 16, 64, 128, 1), (32, 16, 16, 64, 64, 3),
    (32, 8, 8, 128, 64, 1), (32, 8, 8, 64, 128, 1), (32, 8, 8, 64, 64, 3),
    (32, 4, 4, 128, 64, 1), (32, 4, 4, 64, 128, 1), (32, 4, 4, 64, 64, 3),
    (32, 64, 64, 128, 128, 1), (32, 64, 64, 16, 128, 1),
]
# (N, H, W, Cin, Cout, R) of the first half; the second is on the map of half the size (the low branch of an hourglass level)
PAIRS = [(4, 64, 64, 128, 128, 1), (16, 32, 32, 128, 128, 1), (4, 64, 64, 16, 128, 1), (16, 32, 32, 16, 128, 1),
         (32, 16, 16, 128, 64, 1), (32, 16, 16, 64, 64, 3), (2, 32, 32, 64, 128, 1)]
FOLD = ('off', 'on')
PAIR_FOLD = ('off', 'a', 'both')
FUSE = ('off', 'on')


def _cid(c):
    return 'N%d %dx%d %d->%d %dx%d' % (c[0], c[1], c[2], c[3], c[4], c[5], c[5])


# Route of each case, computed once from the host predicates: per (fold, fuse) in the order off/off, off/on, on/off, on/on (pairs:
# fold off / a / both, each with fuse off / on), four digits = applies folded, weight gradients fused, conv_c1 launches, conv_c3
# launches.  A threshold or domain change that moves a launch to another route shows up here, as an edit of this table.
_ROUTE_TABLE = {
    'N1 32x32 128->64 1x1': '0000 0000 1000 1000',
    'N2 32x32 128->64 1x1': '0010 0110 1010 1110',
    'N1 32x32 64->128 1x1': '0000 0000 1000 1000',
    'N2 32x32 64->128 1x1': '0010 0110 1010 1110',
    'N15 64x64 128->16 1x1': '0000 0000 1000 1000',
    'N16 64x64 128->16 1x1': '0000 0000 1000 1000',
    'N10 48x48 64->64 3x3': '0000 0000 1000 1000',
    'N11 48x48 64->64 3x3': '0000 0000 1000 1000',
    'N7 64x64 128->128 1x1': '0010 0010 0010 0010',
    'N4 64x64 64->64 3x3': '0000 0000 1000 1000',
    'N8 64x64 64->64 3x3': '0001 0001 1001 1001',
    'N2 128x128 64->64 3x3': '0000 0000 1000 1000',
    'N32 36x32 64->64 3x3': '0000 0000 1000 1000',
    'N1 128x128 128->128 1x1': '0010 0010 0010 0010',
    'N4 64x64 128->128 1x1': '0010 0010 0010 0010',
    'N16 32x32 128->128 1x1': '0010 0010 0010 0010',
    'N1 128x128 16->128 1x1': '0010 0010 0010 0010',
    'N4 64x64 16->128 1x1': '0010 0010 0010 0010',
    'N16 32x32 16->128 1x1': '0010 0010 0010 0010',
    'N8 64x64 128->128 1x1': '0010 0010 1000 1000',
    'N8 64x64 16->128 1x1': '0010 0010 1000 1000',
    'N32 64x64 128->64 1x1': '0010 0110 1010 1110',
    'N32 64x64 64->128 1x1': '0010 0110 1010 1110',
    'N32 64x64 64->64 3x3': '0001 0001 1001 1001',
    'N32 32x32 128->64 1x1': '0010 0110 1010 1110',
    'N32 32x32 64->128 1x1': '0010 0110 1010 1110',
    'N32 32x32 64->64 3x3': '0001 0001 1001 1001',
    'N32 16x16 128->64 1x1': '0010 0110 1010 1110',
    'N32 16x16 64->128 1x1': '0010 0110 1010 1110',
    'N32 16x16 64->64 3x3': '0000 0000 1000 1000',
    'N32 8x8 128->64 1x1': '0010 0110 1010 1110',
    'N32 8x8 64->128 1x1': '0010 0110 1010 1110',
    'N32 8x8 64->64 3x3': '0000 0000 1000 1000',
    'N32 4x4 128->64 1x1': '0000 0000 1000 1000',
    'N32 4x4 64->128 1x1': '0000 0000 1000 1000',
    'N32 4x4 64->64 3x3': '0000 0000 1000 1000',
    'N32 64x64 128->128 1x1': '0010 0010 1000 1000',
    'N32 64x64 16->128 1x1': '0010 0010 1000 1000',
    'N4 64x64 128->128 1x1 pair': '0010 0010 0010 0010 0010 0010',
    'N16 32x32 128->128 1x1 pair': '0010 0010 0010 0010 0010 0010',
    'N4 64x64 16->128 1x1 pair': '0010 0010 0010 0010 0010 0010',
    'N16 32x32 16->128 1x1 pair': '0010 0010 0010 0010 0010 0010',
    'N32 16x16 128->64 1x1 pair': '0010 0210 1010 1210 2010 2210',
    'N32 16x16 64->64 3x3 pair': '0000 0000 1000 1000 2000 2000',
    'N2 32x32 64->128 1x1 pair': '0010 0210 1010 1210 2010 2210',
}
ROUTES = {}
for _c, _r in _ROUTE_TABLE.items():
    _keys = itertools.product(PAIR_FOLD if _c.endswith('pair') else FOLD, FUSE)
    ROUTES.update({(_c, f, u): tuple(int(d) for d in r) for (f, u), r in zip(_keys, _r.split())})


def _route(c, fold, fuse):
    return ROUTES[(_cid(c), fold, fuse)]


def setup_module(module):
    global G, R
    tk.setup_module(tk)
    G, R = tk.G, tk.R
    # default dispatch only: the routes below are those of the default options
    for name, v in (('conv_c1', 1), ('conv_c3', 1), ('conv_pp', 1), ('conv_c1_blocks', 192), ('conv_c3_blocks', 160),
                    ('conv_pp_blocks', 256)):
        prev = R.set_option(name, v)
        R.set_option(name, prev)
        assert prev == v, 'option %s is %d, not its default %d' % (name, prev, v)


def _run(bt, ops):
    c1, c3 = R.set_option('conv_c1_launches', 0), R.set_option('conv_c3_launches', 0)      # (read-only counters)
    bt.realise().run(ops, 0, partials=True)
    return R.set_option('conv_c1_launches', 0) - c1, R.set_option('conv_c3_launches', 0) - c3


def _compare(bt, o, case, label):
    N, H, W = case[:3]
    m = N * H * W
    bt.compare(o['dz'], label='%s dz' % label, **TOL[1])
    bt.compare(o['bst'], atol=TOL[1]['atol'] * m, rtol=TOL[1]['rtol'], label='%s bn sums' % label)
    bt.compare(o['dgam'], atol=1e-3, rtol=1e-4, label='%s dgamma of the folded BN' % label)
    bt.compare(o['dbet'], atol=1e-3, rtol=1e-4, label='%s dbeta of the folded BN' % label)
    tol = dict(atol=2e-2 + 2e-5 * m, rtol=3e-2)
    bt.compare(o['dw'], label='%s dw' % label, **tol)
    if o['db'] is not None:
        bt.compare(o['db'], label='%s dbias' % label, **tol)
    dg = o['dg']
    if not (getattr(dg, 'fold_active', False) and getattr(dg, 'fused_active', False)):
        bt.compare(o['du'], label='%s materialised operand' % label, **TOL[1])   # (written unless folded AND fused)


@pytest.mark.parametrize('fuse', FUSE)
@pytest.mark.parametrize('fold', FOLD)
@pytest.mark.parametrize('case', SINGLES, ids=_cid)
def test_default_dispatch_of_a_data_gradient(case, fold, fuse):
    N, H, W, Cin, Cout, Rr = case
    gen = torch.Generator().manual_seed(401 + sum(case))
    bt = Bench(1)
    ops, o = bn_backward_dgrad_ops(bt, gen, N, H, W, Cout, Cin, Rr, bias=Rr == 1, fold=fold == 'on', fuse=fuse == 'on')
    n_c1, n_c3 = _run(bt, ops)
    got = (bt.n_folded, bt.n_fused, n_c1, n_c3)
    assert got == _route(case, fold, fuse), '%s fold %s fuse %s: route (folded, fused, conv_c1, conv_c3) %s, pinned %s' % (
        _cid(case), fold, fuse, got, _route(case, fold, fuse))
    _compare(bt, o, case, _cid(case))


@pytest.mark.parametrize('fuse', FUSE)
@pytest.mark.parametrize('fold', PAIR_FOLD)
@pytest.mark.parametrize('case', PAIRS, ids=lambda c: _cid(c) + ' + %dx%d' % (c[1] // 2, c[2] // 2))
def test_default_dispatch_of_a_data_gradient_pair(case, fold, fuse):
    N, H, W, Cin, Cout, Rr = case
    gen = torch.Generator().manual_seed(503 + sum(case))
    bt = Bench(1)
    halves = []
    for i, (h, w) in enumerate(((H, W), (H // 2, W // 2))):
        on = fold == 'both' or (fold == 'a' and i == 0)
        halves.append(bn_backward_dgrad_ops(bt, gen, N, h, w, Cout, Cin, Rr, bias=Rr == 1, fold=on, fuse=fuse == 'on'))
    (oa, a), (ob, b) = halves
    # [wprep a, wprep b, apply a, apply b, both data gradients in one launch, weight gradient a, weight gradient b]
    ops = [oa[0], ob[0], oa[1], ob[1], G.Op('conv2', a=a['dg'], b=b['dg']), oa[3], ob[3]]
    n_c1, n_c3 = _run(bt, ops)
    got = (bt.n_folded, bt.n_fused, n_c1, n_c3)
    pinned = ROUTES[(_cid(case) + ' pair', fold, fuse)]
    assert got == pinned, '%s pair fold %s fuse %s: route (folded, fused, conv_c1, conv_c3) %s, pinned %s' % (
        _cid(case), fold, fuse, got, pinned)
    _compare(bt, a, case, _cid(case) + ' pair[a]')
    _compare(bt, b, (N, H // 2, W // 2), _cid(case) + ' pair[b]')
