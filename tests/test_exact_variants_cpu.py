"""Which instantiation of the halo-tile kernels every case of the bit-exact lists launches (tests/_exact_inputs.py TILE_FWD,
TILE_BWD, TILE_PAIR, TILE_WGRAD; tests/test_exact_tile_gpu.py runs them), asked of the library without a device:
fpd_conv_tile_variant() / fpd_conv_tile_pair_variant() answer through the tile_route() the launch walks, fpd_wgrad_tile_variant()
through wt_grid() and the launch's own choice of the template arguments.

conv_tile is compiled for T x BK x TN x ALLW x FOLD, wgrad_tile_kernel for T x R x TP x H4 x SMALL.  The REACHABLE set is what a
sweep of the query finds over N in 1..32, the map sizes of the case lists and of the networks, C and K in 16..384, 1x1 and 3x3,
both storage types and -- conv_tile -- a forward launch, a BNRELU_BWD data gradient and one that asks for the fold (weight
gradients: with slabs and without).  The union over the case lists must equal it: a list that stops reaching an instantiation
fails here by the instantiation's name, before any device is involved.  (ALLW with TN = 4 is compiled and not reachable: nine
staged weight tiles of 128 channels do not fit the LDS next to the halo.)"""
import ctypes
import itertools

import pytest

from tests import _exact_inputs as X

MAPS = [(64, 48), (32, 24), (16, 12), (8, 6), (44, 48), (20, 48), (7, 6), (6, 128), (16, 16), (32, 32), (64, 64)]
CHANNELS = (16, 32, 48, 64, 96, 128, 192, 256, 384)
FWD, BWD, BWD_FOLD = 0, 1, 2


@pytest.fixture(scope='module')
def R():
    from fpd_amd import runtime
    runtime.lib()
    return runtime


def _conv(R, dtype):
    a = R.ConvT()
    a.x = a.w = a.y = 64                          # (never dereferenced: the queries are pure host code)
    a.dtype = dtype
    return a


def _set(R, a, N, H, W, C, K, r, situation):
    """Stride-1 'same' convolution C -> K; BWD: a BNRELU_BWD data gradient, BWD_FOLD: one that asks for the folded apply."""
    a.N, a.H, a.W, a.C, a.K, a.R, a.S, a.stride, a.pad, a.P, a.Q = N, H, W, C, K, r, r, 1, (r - 1) // 2, H, W
    a.epi = R.EPI_PLAIN if situation == FWD else R.EPI_BNRELU_BWD
    if situation != FWD:
        a.epi_x = a.epi_stats = 64
        a.epi_bn.mode, a.epi_bn.gamma, a.epi_bn.beta, a.epi_bn.stats = R.BN_TRAIN, 64, 64, 64
    a.fold_x = 64 if situation == BWD_FOLD else None
    return a


def conv_name(v):
    return '%s BK%d TN%d%s%s' % ({2: 'bf16', 4: 'fp32'}[v & 15], v >> 4 & 255, v >> 12 & 15, ' ALLW' if v >> 16 & 1 else '', ' FOLD' if v >> 17 & 1 else '')


def wgrad_name(R, v):
    return '<%s, %d, %d%s%s>%s' % ('bf16' if v & 15 == R.BF16 else 'float', v >> 4 & 15, v >> 8 & 4095, ', H4' if v >> 20 & 1 else '',
                                   ', SMALL' if v >> 21 & 1 else '', ' KSPLIT' if v >> 22 & 1 else '')


def _reachable_conv(R):
    lib, out = R.lib(), set()
    for dtype in (R.BF16, R.F32):
        a = _conv(R, dtype)
        for N, (H, W), C, K, r, sit in itertools.product(range(1, 33), MAPS, CHANNELS, CHANNELS, (1, 3), (FWD, BWD, BWD_FOLD)):
            out.add(lib.fpd_conv_tile_variant(ctypes.byref(_set(R, a, N, H, W, C, K, r, sit))))
    return out - {-1}


def _case_variants_conv(R):
    """{variant: a case that launches it} over TILE_FWD and TILE_BWD in both storage types"""
    lib, got = R.lib(), {}
    for dtype in (R.BF16, R.F32):
        a = _conv(R, dtype)
        for c in (c for c in X.TILE_FWD if dtype in c[8]):
            got.setdefault(lib.fpd_conv_tile_variant(ctypes.byref(_set(R, a, *c[:6], FWD))), ('TILE_FWD', c, dtype))
        for c in X.TILE_BWD:
            N, H, W, C, K, r = c                  # the data gradient reads the forward's K channels and writes its C
            for sit in (BWD, BWD_FOLD):
                got.setdefault(lib.fpd_conv_tile_variant(ctypes.byref(_set(R, a, N, H, W, K, C, r, sit))), ('TILE_BWD', c, dtype, sit))
    return got


def test_conv_tile_cases_reach_every_reachable_instantiation(R):
    reach, got = _reachable_conv(R), _case_variants_conv(R)
    assert -1 not in got, 'conv_tile declines %s' % (got[-1],)
    missing, beyond = reach - set(got), set(got) - reach
    assert not missing, 'no exact case launches: ' + '; '.join(sorted(conv_name(v) for v in missing))
    assert not beyond, 'the sweep does not find: ' + '; '.join('%s (%s)' % (conv_name(v), got[v]) for v in sorted(beyond))
    # the compiled set: bf16 x BK {64, 32, 16}, fp32 x BK {32, 16}; TN {1, 2, 4}; ALLW for one-chunk kernels (bf16 BK64, fp32 BK32);
    # FOLD for TN <= 2.  All of it is reachable but ALLW at TN = 4
    compiled = {esz | bk << 4 | tn << 12 | allw << 16 | fold << 17
                for esz, bks in ((2, (64, 32, 16)), (4, (32, 16))) for bk in bks for tn in (1, 2, 4)
                for allw in ((0, 1) if bk == bks[0] else (0,)) for fold in ((0, 1) if tn <= 2 else (0,))}
    assert compiled - reach == {2 | 64 << 4 | 4 << 12 | 1 << 16, 4 | 32 << 4 | 4 << 12 | 1 << 16}, sorted(conv_name(v) for v in compiled ^ reach)
    assert reach <= compiled and len(reach) == 33


def test_conv_tile_fold_is_declined_at_four_output_tiles(R):
    """... and offered for every other data gradient of the list, in both storage types."""
    lib = R.lib()
    for dtype in (R.BF16, R.F32):
        for N, H, W, C, K, r in X.TILE_BWD:
            v = lib.fpd_conv_tile_variant(ctypes.byref(_set(R, _conv(R, dtype), N, H, W, K, C, r, BWD_FOLD)))
            assert v >= 0 and (v >> 17 & 1) == ((N, H, W, C, K, r) != X.TILE_BWD_TN4), ((N, H, W, C, K, r), conv_name(v))
    for dtype in (R.BF16, R.F32):
        N, H, W, C, K, r = X.TILE_BWD_TN4
        v = lib.fpd_conv_tile_variant(ctypes.byref(_set(R, _conv(R, dtype), N, H, W, K, C, r, BWD_FOLD)))
        assert v >> 12 & 15 == 4 and v >> 17 & 1 == 0, conv_name(v)


def test_conv_tile_pairs_go_out_as_one_launch(R):
    """Every pair of TILE_PAIR is served by the pair kernel (both halves in the domain, one chunking) in both storage types, at
    more than one (BK, TN)."""
    lib, seen = R.lib(), set()
    for dtype in (R.BF16, R.F32):
        for N, H, W, C, K, r, bn, epi in X.TILE_PAIR:
            p = R.ConvPairT()
            sit = FWD if epi == 'plain' else BWD
            p.a, p.b = _set(R, _conv(R, dtype), N, H, W, C, K, r, sit), _set(R, _conv(R, dtype), N, H // 2, W // 2, C, K, r, sit)
            v = lib.fpd_conv_tile_pair_variant(ctypes.byref(p))
            assert v >= 0, 'conv_tile does not pair %s' % ((N, H, W, C, K, r),)
            seen.add(v)
    assert len({v >> 4 for v in seen}) >= 3, sorted(conv_name(v) for v in seen)


def _wgrad(R, dtype, N, H, W, C, K, r, slabs):
    w = R.WgradT()
    w.x = w.dy = w.dw = 64
    w.N, w.H, w.W, w.C, w.K, w.R, w.S, w.stride, w.pad, w.P, w.Q = N, H, W, C, K, r, r, 1, (r - 1) // 2, H, W
    w.dtype = dtype
    if slabs:
        w.partial, w.partial_stride = 64, K * r * r * C + K
    return w


def test_wgrad_tile_cases_reach_every_instantiation(R):
    lib, reach, got = R.lib(), set(), {}
    for dtype, N, (H, W), C, K, r, slabs in itertools.product((R.BF16, R.F32), (1, 2, 3, 4, 8, 16, 32), MAPS, CHANNELS, CHANNELS, (1, 3), (False, True)):
        reach.add(lib.fpd_wgrad_tile_variant(ctypes.byref(_wgrad(R, dtype, N, H, W, C, K, r, slabs))))
    reach.discard(-1)
    for c in X.TILE_WGRAD:
        for dtype in c[7]:
            for slabs in X.wgrad_flushes(c):
                v = lib.fpd_wgrad_tile_variant(ctypes.byref(_wgrad(R, dtype, *c[:6], slabs)))
                assert v >= 0, 'wgrad_tile_kernel does not serve %s (dtype %d, slabs %s)' % (c, dtype, slabs)
                got.setdefault(v, c)
    missing = reach - set(got)
    assert not missing, 'no exact case launches wgrad_tile_kernel' + '; '.join(sorted(wgrad_name(R, v) for v in missing))
    # the eight instantiations fpd_wgrad_tile_launch can choose
    want = {(R.BF16, 3, 128, 0, 0, 0), (R.BF16, 3, 128, 1, 0, 0), (R.BF16, 3, 128, 0, 1, 0), (R.F32, 3, 128, 0, 0, 0),
            (R.BF16, 1, 128, 0, 0, 1), (R.F32, 1, 128, 0, 0, 1), (R.BF16, 1, 256, 0, 0, 1), (R.F32, 1, 256, 0, 0, 1)}
    assert {(v & 15, v >> 4 & 15, v >> 8 & 4095, v >> 20 & 1, v >> 21 & 1, v >> 22 & 1) for v in got} == want == \
        {(v & 15, v >> 4 & 15, v >> 8 & 4095, v >> 20 & 1, v >> 21 & 1, v >> 22 & 1) for v in reach}
    # the per-channel table of the prologue is indexed c0 + c: exact cases with a prologue on a second channel tile, per kernel family
    multi = {(dtype, c[5]) for c in X.TILE_WGRAD for dtype in c[7] if c[6] and c[3] > (64 if dtype == R.BF16 else 32)}
    assert multi == {(R.BF16, 1), (R.BF16, 3), (R.F32, 1), (R.F32, 3)}
