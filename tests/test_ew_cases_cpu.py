"""What the case tables of tests/test_elementwise_gpu.py (tests/_ew_cases.py) do and do not reach, worked out from the grid
rule of csrc/elementwise.hip on the host: these are conditions on the committed tables, not measurements.  The option the
multi-trip runs rely on is a host-side integer, so its round trip is checked here too (the library loads without a GPU)."""
import os
import subprocess

import pytest

from tests import _ew_cases as K


def test_grid_rule_by_hand():
    """The figures the case table was chosen by: bf16 at C = 64 steps over 32 pixels, fp32 over 16; the pooled ops of the
    multi-trip shape have 90 pixels, so one bf16 block makes trips of 32 / 32 / 26."""
    assert K.pixels_per_step(64, 1) == 32 and K.pixels_per_step(64, 0) == 16
    assert K.pixels_per_step(8, 1) == 256 and K.pixels_per_step(384, 1) == 5 and K.pixels_per_step(384, 0) == 2
    assert K.pixels_per_step(512, 0) == 2 and K.pixels_per_step(48, 1) == 42 and 256 % (48 // 8) != 0
    assert K.npix('add', K.MULTI) == 360 and K.npix('maxpool_fwd', K.MULTI) == 90
    assert K.trips('maxpool_fwd', K.MULTI, 1, True, 1) == (3, 26, 32)
    assert K.trips('add', K.MULTI, 1, False, 3) == (4, 72, 96)
    assert K.grid('add', (32, 128, 128, 64), 1, False) == 2048 and K.grid('bnrelu_fwd', (32, 128, 128, 64), 1, True) == 512


@pytest.mark.parametrize('dtype', K.DTYPES)
def test_every_multi_trip_launch_makes_three_trips_with_a_ragged_last_one(dtype):
    launches = K.b2_launches()
    assert {l[1] for l in launches} >= set(K.EW_OPS) | {'affsum'}
    for label, op, dims, stats in launches:
        assert K.grid(op, dims, dtype, stats) > min(K.CAPS), label      # the smallest cap does cap
        hit = []
        for cap in K.CAPS:
            t, last, full = K.trips(op, dims, dtype, stats, cap)
            hit.append(t >= 3 and last < full)
        assert any(hit), '%s (dtype %d): no cap of %s gives >= 3 trips with a ragged last trip' % (label, dtype, K.CAPS)


@pytest.mark.parametrize('dtype', K.DTYPES)
def test_default_grid_of_every_all_ops_shape_is_a_single_trip(dtype):
    """What the default-grid runs cover: every pixel has a thread of its own (grid = cdiv(npix, PB), no cap reached), so they
    check the per-pixel arithmetic, the idle-thread guard and the ragged last block -- not the grid-stride walk."""
    for shape in K.SHAPES:
        for label, op, dims, stats in K.b1_launches(shape):
            g = K.grid(op, dims, dtype, stats)
            assert g == K.cdiv(K.npix(op, dims), K.pixels_per_step(dims[3], dtype)), (label, shape)
            assert K.trips(op, dims, dtype, stats)[0] == 1, (label, shape)


def test_shapes_cover_the_channel_edges():
    cs = {s[3] for s in K.SHAPES}
    assert {8, 48, 384, 512} <= cs
    for n, h, w, c in K.SHAPES:
        assert h % 2 == 0 and w % 2 == 0
    assert all(s in K.SHAPES for s in K.INPLACE_SHAPES)


def test_ew_blocks_option_round_trip_without_a_device():
    from fpd_amd import runtime as R
    if not os.path.exists(R.LIB_PATH):
        subprocess.check_call(['bash', os.path.join(os.path.dirname(R.LIB_PATH), 'build.sh')])
    lib = R.lib()
    prev = lib.fpd_set_option(b'ew_blocks', 5)
    try:
        assert prev == 0                                        # the default: no cap
        assert lib.fpd_set_option(b'ew_blocks', -1) == 5        # a negative value only reads
        assert lib.fpd_set_option(b'ew_blocks', -1000) == 5
        assert lib.fpd_set_option(b'ew_blocks', 0) == 5
        assert lib.fpd_set_option(b'ew_blocks', 1) == 0
    finally:
        lib.fpd_set_option(b'ew_blocks', prev)
    assert lib.fpd_set_option(b'ew_blocks', -1) == prev
