"""Preconditions of tests/test_step_kernels_gpu.py, asserted without a device: the launch geometry every loss case claims
(through fpd_loss_geometry, which fpd_loss's launch computes its grid with), the headroom that makes the loss sums exact, the
reachability and the teeth of the Adam bar (tests/_adam_ref.py), the exactness of the degenerate Adam trajectory, the planted
ties of the weight-prep masters and the bound of the running-statistics update on the reference's own two evaluation orders."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import _adam_ref, _sgd_ref, _step_cases as SC


@pytest.fixture(scope='module')
def runtime():
    from fpd_amd import runtime as R
    if not os.path.exists(R.LIB_PATH):
        subprocess.check_call(['bash', os.path.join(os.path.dirname(R.LIB_PATH), 'build.sh')])
    R.lib()
    return R


def test_loss_cases_take_the_launch_geometry_they_claim(runtime):
    R = runtime
    seen = set()
    for case, dtype, variant in SC.LOSS_RUNS:
        want = SC.LOSS_CLAIMS[(case, dtype)]
        exp = SC.expected_geometry(case, dtype)
        assert exp[:4] == want, (case, dtype, exp, want)                       # the claim against the rule restated
        got = SC.loss_geometry(R, SC.loss_struct(R, case, dtype, variant))
        assert got == want[:3], (case, dtype, variant, got, want)              # ... and against the library
        seen.add((want[0], want[2] > 1))
        assert np.prod(case[:4]) <= 2 ** 20                                    # every map at or below 2^20 elements
    assert seen == {(1, True), (1, False), (0, False)}
    # what the single cases are there for
    g = lambda c, dt: SC.expected_geometry(c, dt)
    assert g((33, 16, 40, 40, 1), SC.BF16)[3:] == (True, 64) and g((40, 8, 24, 56, 3), SC.F32)[3:] == (True, 64)
    assert g((2, 32, 16, 8, 8), SC.BF16)[4] == 128 and g((300, 16, 8, 8, 1), SC.BF16)[4] == 64
    assert g((3, 17, 12, 9, 2), SC.F32)[4] == 44 and g((2, 20, 10, 13, 2), SC.F32)[4] == 2
    cnt = int(np.prod(SC.POW2_CASE[:4]))
    assert cnt & (cnt - 1) == 0 and all(int(np.prod(c[:4])) & (int(np.prod(c[:4])) - 1) for c, _, _ in SC.LOSS_CASES[1:4])
    # every variant runs on a case whose blocks walk several tiles and on a scalar case
    for key, values in (('nchw', (0, 1)), ('wkd', (False, True)), ('null', (None, 'one', 'all'))):
        k = ('nchw', 'wkd', 'null').index(key)
        for val in values:
            hit = {(SC.LOSS_CLAIMS[(c, dt)][0], SC.LOSS_CLAIMS[(c, dt)][2] > 1) for c, dt, v in SC.LOSS_RUNS if v[k] == val}
            assert (1, True) in hit and (0, False) in hit, (key, val, hit)
    assert all(not (v[2] == 'one' and c[4] < 2) for c, _, v in SC.LOSS_RUNS)


def test_loss_geometry_follows_pointer_alignment_and_refuses_bad_dimensions(runtime):
    R = runtime
    case, variant = SC.POW2_CASE, SC.V_A
    a = SC.loss_struct(R, case, SC.BF16, variant)
    assert SC.loss_geometry(R, a) == (1, 256, 2)
    for field in ('teacher', 'out', 'dout'):
        a = SC.loss_struct(R, case, SC.BF16, variant)
        if field == 'teacher':
            a.teacher = 4096 + 2
        else:
            getattr(a, field)[1] = 4096 + 2
        assert SC.loss_geometry(R, a) == (0, 16 * 64, 1), field                 # one map two bytes off: the scalar kernel, 64-pixel tiles
    import ctypes as C
    a = SC.loss_struct(R, case, SC.BF16, variant)
    v, b, t = C.c_int32(7), C.c_int32(7), C.c_int32(7)
    a.J = 33
    assert R.lib().fpd_loss_geometry(C.byref(a), C.byref(v), C.byref(b), C.byref(t)) != 0 and b'J=33' in R.lib().fpd_last_error()
    a.J, a.S = 16, 9
    assert R.lib().fpd_loss_geometry(C.byref(a), C.byref(v), C.byref(b), C.byref(t)) != 0
    assert R.lib().fpd_loss_geometry(None, C.byref(v), C.byref(b), C.byref(t)) != 0 and b'null' in R.lib().fpd_last_error()
    assert (v.value, b.value, t.value) == (7, 7, 7)                             # a refused query writes nothing


@pytest.mark.parametrize('case,variant', sorted({(c, v) for c, _, v in SC.LOSS_RUNS}, key=str))
def test_loss_reference_is_exact_and_has_headroom(case, variant):
    ref = SC.loss_reference(case, variant)
    SC.loss_headroom(ref)
    i = SC.loss_inputs(case, variant[1])
    assert bool((i['w'] == 0).any()) and bool((i['w'] != 0).any())
    for t in i['outs'] + [i['teacher'], i['target']]:
        assert torch.equal(t.bfloat16().float(), t)                             # one specification for both storage types
    w0 = (ref['w2'] == 0) & (ref['w2k'] == 0)
    for s, (g32, g16) in enumerate(zip(ref['grads'][SC.F32], ref['grads'][SC.BF16])):
        assert float(g32.abs().max()) > 0 and float(g16.float().abs().max()) > 0
        assert not bool(g32[w0.expand_as(g32)].any())
    assert ref['losses'][0] > 0 and ref['losses'][1] > 0 and ref['losses'][0] < 2 ** 9
    cnt = ref['cnt']
    assert (SC.loss_bound(ref['losses'][0], 256, cnt) == 0.0) == (cnt & (cnt - 1) == 0)


@pytest.mark.parametrize('regime', _adam_ref.REGIMES)
def test_adam_bar_is_reachable_by_the_kernels_arithmetic_and_has_teeth(regime):
    n = 20011
    for kind in _adam_ref.STARTS:
        p0, grads = _adam_ref.start(kind, n), _adam_ref.gradients(regime, n)
        r32, r64 = _adam_ref.adam_trajectory(p0, grads), _adam_ref.adam_trajectory(p0, grads, dtype=torch.float64)
        ours = _adam_ref.restated(p0, grads)
        ratio = _sgd_ref.assert_as_close_as_fp32(ours[0], r32[0], r64[0], 'restated kernel arithmetic, %s start, %s' % (kind, regime))
        print('adam restated, %s start, %s gradients: ratio %.3f' % (kind, regime, ratio))
        assert not torch.equal(r64[0], p0.double())
        if kind == 'zero':                       # (on an N(0,1) start the parameter's own ulp hides part of a wrong update)
            for mutant in _adam_ref.MUTANTS:
                bad = _adam_ref.ratio(_adam_ref.restated(p0, grads, mutant=mutant)[0], r32[0], r64[0])
                print('    mutant %s: ratio %.3g' % (mutant, bad))
                assert bad > 2.0, (mutant, bad)
                with pytest.raises(AssertionError):
                    _sgd_ref.assert_as_close_as_fp32(_adam_ref.restated(p0, grads, mutant=mutant)[0], r32[0], r64[0], mutant)


def test_adam_moments_follow_torch_with_the_betas_as_float32():
    """fpd_adam_t carries the betas as float32, so m and v are those of Adam at betas (float32(0.9), float32(0.999)): against
    THAT trajectory the restated arithmetic is as close as float32 torch is; against the nominal betas 1 - beta2 is off by
    1.3e-5 of itself, which the bias correction (formed from the same float32 beta) cancels in the parameters."""
    n = 20011
    betas32 = tuple(float(np.float32(b)) for b in _adam_ref.BETAS)
    for regime in _adam_ref.REGIMES:
        p0, grads = _adam_ref.start('zero', n), _adam_ref.gradients(regime, n)
        r32 = _adam_ref.adam_trajectory(p0, grads, betas=betas32)
        r64 = _adam_ref.adam_trajectory(p0, grads, betas=betas32, dtype=torch.float64)
        ours = _adam_ref.restated(p0, grads)
        for k, name in ((1, 'm'), (2, 'v')):
            _sgd_ref.assert_as_close_as_fp32(ours[k], r32[k], r64[k], '%s, %s' % (name, regime))


def test_adam_schedule_and_degenerate_trajectory_are_exact_on_the_reference():
    for t in (1, 2, 3):
        bc1, bc2 = _adam_ref.bias_corrections(t)
        assert bc1.dtype == np.float32 and abs(float(bc1) - (1 - 0.9 ** t)) < 1e-6 and abs(float(bc2) - (1 - 0.999 ** t)) < 1e-6
    assert _adam_ref.bias_corrections(3, (0.0, 0.0)) == (1.0, 1.0)
    p0, grads = _adam_ref.exact_inputs(4099)
    assert all(bool((g != 0).all()) and float(g.abs().max()) <= 1 and float(g.abs().min()) >= 0.125 for g in grads)
    want = _adam_ref.exact_expected(p0, grads)
    for dt in (torch.float32, torch.float64):    # torch.optim.Adam itself walks the closed form, in both precisions
        got = _adam_ref.adam_trajectory(p0, grads, _adam_ref.EXACT_LRS, (0.0, 0.0), 0.0, dtype=dt)
        assert all(torch.equal(a.double(), b.double()) for a, b in zip(got, want))
    got = _adam_ref.restated(p0, grads, _adam_ref.EXACT_LRS, (0.0, 0.0), 0.0)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(want[0].bfloat16().float(), want[0])                     # (k/8: the bf16 copy is exact here)


def test_weight_prep_masters_carry_ties_and_the_tables_reach_what_they_claim():
    sp = SC.special_values()
    b16 = SC.bits(sp.bfloat16())
    up = lambda x: SC.bits(torch.tensor([x]).bfloat16()).item() & 0xffff
    assert up(1 + 2.0 ** -8) == 0x3f80 and up(1 + 3 * 2.0 ** -8) == 0x3f82          # ties go to the even neighbour: down, up
    assert up(-(1 + 2.0 ** -8)) == 0xbf80 and (b16[-1].item() & 0xffff) == 0x8000 and b16[-2].item() == 0
    for name, table in SC.WPREP_TABLES.items():
        for k, (K, R, S, C, mode) in enumerate(table):
            w = SC.wprep_master(K, R, S, C, k)
            flat = SC.bits(w).reshape(-1)
            assert all(bool((flat == p).any()) for p in SC.bits(sp)), (name, k)       # every special value, by bit pattern
            assert not torch.equal(w.bfloat16().float(), w)
            wf, wb = SC.wprep_reference(w, SC.BF16)
            assert wb.shape == (C, R, S, K) and wb[C - 1, 0, S - 1, 0] == wf[0, R - 1, 0, C - 1]
    tiles = lambda K, R, S, C: R * S * -(-K // 32) * -(-C // 32)
    grid = lambda t: max(1, min((max(k * r * s * c for k, r, s, c, _ in t) + 1023) // 1024, 64))
    main = SC.WPREP_TABLES['main']
    assert grid(main) == 64 and tiles(*main[0][:4]) == 576 and {m for *_, m in main} == {'both', 'fwd', 'bwd'}
    assert any(K % 32 and C % 32 for K, R, S, C, _ in main) and any(R != S for K, R, S, C, _ in main)
    one = SC.WPREP_TABLES['one_block']
    assert grid(one) == 1 and max(tiles(*e[:4]) for e in one) > 1 and grid(SC.WPREP_TABLES['single']) == 9


@pytest.mark.parametrize('kind', sorted(SC.BNUPD_TABLES))
def test_bn_update_reference_is_exact_or_within_its_own_bound(kind):
    seen_neg = False
    for k, (C, count, _) in enumerate(SC.BNUPD_TABLES[kind]):
        i = SC.bnupd_inputs(kind, k, C, count)
        plain, fused = SC.bnupd_reference(i), SC.bnupd_reference(i, fused=True)
        assert bool((i['stats'][:, 0] > 0).any()) and bool((i['stats'][:, 0] < 0).any())      # replicas of mixed signs ...
        s = SC.joined_sums(i['stats'])
        assert not torch.equal(SC.joined_sums(i['stats'][:1]), s)                             # ... none of which is the sum
        if kind == 'dyadic':
            assert count & (count - 1) == 0 and torch.equal(i['stats'] * 2 ** 20, torch.round(i['stats'] * 2 ** 20))
            assert torch.equal(plain[2], fused[2]) and bool((plain[2][i['flat']] == 0).all()) and bool((plain[2] >= 0).all())
            assert float((s[0] / count).abs().max()) == 64.0
            assert torch.equal(plain[0], fused[0]) and torch.equal(plain[1], fused[1])
        else:
            seen_neg = seen_neg or bool((plain[2][i['neg']] < 0).all() and (fused[2][i['neg']] < 0).all() and i['neg'].any())
            bm, bv = SC.bnupd_bound(i, plain)
            assert bool(((plain[0] - fused[0]).abs() <= bm).all()) and bool(((plain[1] - fused[1]).abs() <= bv).all())
            mom = float(np.float32(SC.BN_MOMENTUM))
            assert torch.equal(plain[1][i['neg']], (1.0 - mom) * i['rvar'].double()[i['neg']])      # the clamp: 0.9 running_var
    assert kind == 'dyadic' or seen_neg
    assert {c for c, _, _ in SC.BNUPD_TABLES[kind]} == {16, 48, 257, 384} and sum(1 for *_, nbt in SC.BNUPD_TABLES[kind] if not nbt) == 1


def test_cast_sources_hold_the_values_they_are_there_for():
    x = SC.cast_source_f32()
    assert x.numel() > 4096 * 256 and bool(torch.isnan(x).any()) and bool(torch.isinf(x).any())
    assert all(bool((SC.bits(x) == p).any()) for p in SC.bits(SC.special_values()))
    b = SC.cast_source_bf16()
    assert not bool(torch.isnan(b.float()).any()) and bool(torch.isinf(b.float()).any())
    assert bool(((b.float() != 0) & (b.float().abs() < 2.0 ** -126)).any())                    # denormals
    n, c, h, w = SC.LAYOUT_SHAPES[-1]
    assert n * c * h * w > 4096 * 256 and all(np.prod(s) <= 4096 * 256 for s in SC.LAYOUT_SHAPES[:-1])
