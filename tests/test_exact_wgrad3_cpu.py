"""What the bit-exact list of the wgrad3 weight gradient (tests/_exact_inputs.py W3_WGRAD; tests/test_exact_wgrad3_gpu.py runs it)
reaches, checked without a device.

  * Geometry, asked of the library: every case is handed to wgrad3 (fpd_wgrad_tile_variant() answers -1 with slabs) and writes as
    many slabs (fpd_wgrad_num_partials()) as X.w3_geometry() -- the Python restatement of w3_grid() / fpd_cut and of the kernel's
    block -> (range, piece) map -- says it has ranges; the map gives every (range, piece) to exactly one block.
  * Coverage: from that restatement, the list as a whole reaches both piece counts, every width, ranges of 1, 2, 3 and >= 7
    tiles, an uneven cut, fewer than / exactly / more than 8 ranges, a range that starts inside an image, a tile that straddles
    two images (at three tile heights), a range that crosses two image boundaries, and six distinct ring slots at which the
    ranges of one launch start.
  * Every tile matters: on the inputs of the cases up to 16384 pixels, the contribution sum |a| * |dy| of every 256-pixel tile
    to every 32 x 32 piece and every one of the nine taps is non-zero, so that "bit-equal" means a dropped tile, piece or tap
    cannot pass.  The same is asserted per 16-pixel k-step (the unit whose image row decides between the ring and the zero
    pixels), tap rows outside the image excepted.

The preconditions of exactness of the same cases are the `w3_wgrad` parameters of tests/test_exact_inputs_cpu.py."""
import ctypes
import os

import pytest
import torch

from oracle import plan_interp as PI
from tests import _exact_inputs as X

CASES = X.W3_WGRAD


def _ids(c):
    return '-'.join(str(int(v)) for v in c)


@pytest.fixture(scope='module')
def R():
    from fpd_amd import runtime
    runtime.lib()
    return runtime


def _wgrad(R, N, H, W, C, K, slabs=True):
    w = R.WgradT()
    w.x = w.dy = w.dw = 64                        # (never dereferenced: the queries are pure host code)
    w.N, w.H, w.W, w.C, w.K, w.R, w.S, w.stride, w.pad, w.P, w.Q = N, H, W, C, K, 3, 3, 1, 1, H, W
    w.dtype = R.BF16
    if slabs:
        w.partial, w.partial_stride = 64, K * 9 * C + K
    return w


def _geo(case):
    g = X.w3_geometry(*case[:5])
    assert g is not None, 'outside the restated domain: %s' % (case,)
    return g


def _ranges(case):
    """[(first flat row, one past the last flat row, tiles)] of the ranges of a case"""
    g = _geo(case)
    return [(g['cuts'][i] * g['nrows'], g['cuts'][i + 1] * g['nrows'], g['cuts'][i + 1] - g['cuts'][i]) for i in range(g['nranges'])]


def test_library_hands_every_case_to_wgrad3_with_the_restated_geometry(R):
    for v in ('FPD_WGRAD3', 'FPD_WGRAD3_RANGES'):
        if os.environ.get(v) is not None:
            pytest.skip('%s is set: the launch geometry of this process is not the default the restatement describes' % v)
    lib = R.lib()
    for c in CASES:
        g = _geo(c)
        assert lib.fpd_wgrad_tile_variant(ctypes.byref(_wgrad(R, *c[:5]))) == -1, 'wgrad3 does not take %s' % (c,)
        assert lib.fpd_wgrad_num_partials(ctypes.byref(_wgrad(R, *c[:5]))) == g['nranges'], (c, g['nranges'])
        # the block map: every (range, piece) has exactly one block; tiles per range sum to the tiles
        owners = sorted(g['live'].values())
        assert owners == [(r, p) for r in range(g['nranges']) for p in range(g['npieces'])], c
        assert g['cuts'][0] == 0 and g['cuts'][-1] == g['mtiles'] and all(b > a for a, b in zip(g['cuts'], g['cuts'][1:])), c
    # without slabs wgrad3 declines: the case the device test runs that way is wgrad_tile's
    assert lib.fpd_wgrad_tile_variant(ctypes.byref(_wgrad(R, 2, 64, 64, 64, 64, slabs=False))) >= 0


def test_restatement_reproduces_the_geometries_the_list_names():
    """The comments of W3_WGRAD, as numbers: (tiles, ranges, set of tiles per range)."""
    want = {(1, 16, 16, 64, 64): (1, 1, {1}), (2, 16, 16, 64, 64): (2, 1, {2}), (3, 16, 16, 64, 64): (3, 1, {3}),
            (2, 24, 16, 64, 64): (3, 1, {3}), (2, 12, 32, 32, 32): (3, 1, {3}), (2, 6, 64, 64, 64): (3, 1, {3}),
            (1, 8, 32, 64, 64): (1, 1, {1}), (1, 4, 64, 64, 64): (1, 1, {1}), (1, 2, 128, 64, 64): (1, 1, {1}),
            (3, 2, 128, 32, 32): (3, 1, {3}), (1, 14, 128, 32, 32): (7, 1, {7}), (3, 6, 128, 64, 64): (9, 2, {4, 5}),
            (5, 24, 32, 32, 32): (15, 3, {5}), (17, 16, 16, 32, 32): (17, 4, {4, 5}), (3, 40, 64, 32, 32): (30, 7, {4, 5}),
            (2, 64, 64, 64, 64): (32, 8, {4}), (9, 32, 32, 64, 64): (36, 8, {4, 5}), (5, 40, 64, 64, 64): (50, 8, {6, 7}),
            (5, 52, 64, 64, 64): (65, 16, {4, 5}), (9, 40, 32, 32, 32): (45, 8, {5, 6}), (1, 64, 128, 32, 32): (32, 8, {4}),
            (2, 40, 128, 32, 32): (40, 8, {5}), (2, 128, 128, 32, 32): (128, 32, {4}), (16, 64, 64, 32, 32): (256, 64, {4})}
    assert {c[:5] for c in CASES} == set(want)
    for c in CASES:
        g = _geo(c)
        assert (g['mtiles'], g['nranges'], {t for _, _, t in _ranges(c)}) == want[c[:5]], c
    slots = lambda c: [g0 % _geo(c)['ring'] for g0, _, _ in _ranges(c)]
    assert slots((17, 16, 16, 32, 32, True)) == [0, 30, 26, 22] and slots((5, 24, 32, 32, 32, False)) == [0, 4, 8]
    assert set(slots((9, 32, 32, 64, 64, True))) == {0, 14} and len(set(slots((9, 40, 32, 32, 32, True)))) == 8
    assert len(_geo((1, 16, 16, 64, 64, True))['live']) == 4 and _geo((1, 16, 16, 64, 64, True))['blocks'] == 32
    assert len(_geo((3, 40, 64, 32, 32, True))['live']) == 7 and _geo((3, 40, 64, 32, 32, True))['blocks'] == 8
    assert len(_geo((2, 64, 64, 64, 64, True))['live']) == 32 == _geo((2, 64, 64, 64, 64, True))['blocks']


def test_list_reaches_the_geometries_a_wgrad3_launch_can_go_wrong_at():
    geos = {c: _geo(c) for c in CASES}
    assert {g['npieces'] for g in geos.values()} == {1, 4}
    assert {c[2] for c in CASES} == {16, 32, 64, 128}
    per_range = {t for c in CASES for _, _, t in _ranges(c)}
    assert {1, 2, 3} <= per_range and max(per_range) >= 7, per_range
    assert any(len({t for _, _, t in _ranges(c)}) > 1 for c in CASES), 'no uneven cut'
    nr = {g['nranges'] for g in geos.values()}
    assert min(nr) < 8 and 8 in nr and max(nr) > 8, nr
    assert any(1 < g['nranges'] < 8 for g in geos.values()), 'no group of eight blocks with an idle and a second live block'
    assert any(g0 % c[1] != 0 for c in CASES for g0, _, _ in _ranges(c)), 'no range starts inside an image'
    straddle = {geos[c]['nrows'] for c in CASES for t in range(geos[c]['mtiles'])
                if (t * geos[c]['nrows']) // c[1] != (t * geos[c]['nrows'] + geos[c]['nrows'] - 1) // c[1]}
    assert straddle == {16, 8, 4}, 'tile heights with a tile that straddles two images: %s' % sorted(straddle)
    # image boundaries strictly inside a range: flat rows that are multiples of H in (first row, one past the last row)
    crossings = max((g1 - 1) // c[1] - g0 // c[1] for c in CASES for g0, g1, _ in _ranges(c))
    assert crossings >= 2, crossings
    assert max(len({g0 % geos[c]['ring'] for g0, _, _ in _ranges(c)}) for c in CASES) >= 6, 'fewer than 6 distinct start slots in every launch'
    assert any(c[0] * c[1] * c[2] == 65536 and geos[c]['nranges'] == 64 for c in CASES), 'the largest one-piece grid is not reached'
    assert not all(c[5] for c in CASES) and any(c[5] for c in CASES), 'with and without a BN prologue'


SMALL = [c for c in CASES if c[0] * c[1] * c[2] <= 16384]
assert len(SMALL) >= 15


@pytest.mark.parametrize('case', SMALL, ids=_ids)
def test_every_tile_piece_and_tap_contributes(case):
    """sum |a| * |dy| of every tile to every (32 x 32 piece, tap) block is non-zero -- NO tap is excepted at tile level: a tile has
    nrows >= 2 image rows of W >= 16 pixels, so no tap lies outside the image for all of its pixels.  Per 16-pixel k-step (one
    image row ph): non-zero too, EXCEPT tap row r with ph + r - 1 outside [0, H) -- r = 0 on the first row of an image, r = 2 on
    the last; those the kernel reads from the zero pixels.  No tap column is excepted (one of a k-step's 16 pixels at most)."""
    N, H, W, C, K, use_bn = case
    g = _geo(case)
    bt = X.CpuBench(1)
    b = X.w3_wgrad(bt, case)
    bt.realise()                                          # (inputs only: the prologue reads the statistics, an input)
    op = b.ops[0]
    a = PI._prologue(bt.cpu, PI._act(bt.cpu, op.x), op.bn).double().abs()
    dy = PI._act(bt.cpu, op.dy).double().abs()
    ac = a.reshape(N, H, W, C // 32, 32).sum(-1)          # |a| summed over the channels of a piece column
    dk = dy.reshape(N, H, W, K // 32, 32).sum(-1)
    ap = torch.zeros(N, H + 2, W + 2, C // 32, dtype=torch.float64)
    ap[:, 1:H + 1, 1:W + 1] = ac
    ksteps = N * H * W // 16
    row = (torch.arange(ksteps) * 16 // W) % H            # image row of a k-step
    for r in range(3):
        inside = (row + r - 1 >= 0) & (row + r - 1 < H)
        for s in range(3):
            sh = ap[:, r:r + H, s:s + W]                  # a[m + (r - 1, s - 1)], zero outside the image
            prod = dk.reshape(-1, K // 32)[:, :, None] * sh.reshape(-1, C // 32)[:, None, :]      # [pixel][kt][ct]
            per_step = prod.reshape(ksteps, 16, K // 32, C // 32).sum(1)
            per_tile = per_step.reshape(g['mtiles'], 16, K // 32, C // 32).sum(1)
            assert bool((per_tile > 0).all()), 'tap (%d, %d): tiles %s contribute nothing to a piece' % (
                r, s, sorted({int(i[0]) for i in torch.nonzero(per_tile == 0)}))
            assert bool((per_step[inside] > 0).all()), 'tap (%d, %d): k-steps %s contribute nothing to a piece' % (
                r, s, sorted({int(i[0]) for i in torch.nonzero((per_step == 0) & inside[:, None, None])}))
            assert bool((per_step[~inside] == 0).all())
