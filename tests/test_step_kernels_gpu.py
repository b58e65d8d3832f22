"""The step-boundary kernels of csrc/loss_adam.hip on the MI355X, each against a plain CPU reference (tests/_step_cases.py,
tests/_adam_ref.py; preconditions in tests/test_step_cases_cpu.py):

  fpd_loss               bit for bit on dyadic inputs, on every launch geometry (vector kernel with one and with several tiles per
                         block, short last block, ragged last tile, scalar kernel, misaligned maps), NULL gradients, weight_kd,
                         both target layouts; general inputs with a per-element bf16 bound
  fpd_adam               as close to float64 torch as float32 torch is (parameters; m and v at the float32 betas), both ways of
                         passing the schedule, grad_scale, param_lp, a bit-exact degenerate trajectory through the grid-stride
                         loop, zero gradients
  fpd_weight_prep        bit for bit: both outputs, tables of unequal entries, the capped grid, ragged tiles, planted bf16 ties
  fpd_bn_update_running  statistics spread over all replicas; exact on dyadic statistics, a derived bound on general ones
  fpd_cast, layouts      all four casts and both layout changes through the grid-stride loop
Every destination is sentinel-filled with guard elements on both sides, which have to stay intact."""
import numpy as np
import pytest
import torch

from tests import _adam_ref, _sgd_ref, _step_cases as SC

pytestmark = pytest.mark.gpu

R = None
DEV = torch.device('cuda:0')
G = SC.GUARD


def setup_module(module):
    global R
    from fpd_amd import runtime
    R = runtime
    R.lib()


class Guarded:
    """n elements with G sentinel-filled guard elements on each side (and `offset` more in front: a start off the 16-byte grid)."""

    def __init__(self, n, dtype, src=None, offset=0, sentinel=SC.SENTINEL):
        self.n, self.lo = n, G + offset
        self.full = torch.full((n + 2 * G + offset,), sentinel, dtype=dtype, device=DEV)
        self.sent = self.full[:1].clone()
        self.t = self.full[self.lo:self.lo + n]
        if src is not None:
            self.t.copy_(src.reshape(-1).to(dtype))

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.full[:self.lo] == self.sent).all() and (self.full[self.lo + self.n:] == self.sent).all())

    def cpu(self, shape=None):
        t = self.t.cpu()
        return t if shape is None else t.view(shape)


def _same(a, b):
    """Equal by value, element for element (-0 == +0; no NaN on either side)."""
    return a.dtype == b.dtype and a.shape == b.shape and not bool(torch.isnan(a.float()).any()) and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# fpd_loss
def run_loss(case, dtype, variant, inputs, offset=0, calls=1, zero_between=True):
    """-> dict(losses [2] float64 numpy after the last call, douts [S] Guarded or None, geometry, raw: losses bytes per call)"""
    B, J, H, W, S = case
    nchw, wkd, null, alpha, gs = variant
    n = B * H * W * J
    t = SC.tdt(dtype)
    outs = [Guarded(n, t, o, offset) for o in inputs['outs']]
    teacher = Guarded(n, t, inputs['teacher'], offset)
    douts = [None if SC.skipped(null, s, S) else Guarded(n, t, None, offset) for s in range(S)]
    target = (inputs['target'] if nchw else inputs['target'].permute(0, 2, 3, 1)).contiguous().to(DEV)
    w = inputs['w'].contiguous().to(DEV)
    wk = inputs['wk'].contiguous().to(DEV) if inputs.get('wk') is not None else None
    losses = torch.zeros(2, dtype=torch.float64, device=DEV)
    a = SC.loss_struct(R, case, dtype, (nchw, wkd, null, inputs.get('alpha', alpha), gs), dict(
        out=[o.ptr() for o in outs], dout=[d.ptr() if d is not None else None for d in douts], teacher=teacher.ptr(),
        target=target.data_ptr(), weight=w.data_ptr(), weight_kd=wk.data_ptr() if wk is not None else None, losses=losses.data_ptr()))
    geo = SC.loss_geometry(R, a)
    raw = []
    for k in range(calls):
        if k and zero_between:
            losses.zero_()
        R.check(R.lib().fpd_loss(a, R.current_stream()), 'fpd_loss')
        torch.cuda.synchronize()
        raw.append(losses.cpu().numpy().tobytes())
    assert all(x.intact() for x in outs + [teacher]) and all(d is None or d.intact() for d in douts), 'a guard element was written'
    return dict(losses=losses.cpu().numpy(), douts=douts, geo=geo, raw=raw)


@pytest.mark.parametrize('case,dtype,variant', SC.LOSS_RUNS, ids=lambda v: str(v).replace(' ', ''))
def test_loss_is_bit_exact_on_dyadic_inputs(case, dtype, variant):
    B, J, H, W, S = case
    inputs, ref = SC.loss_inputs(case, variant[1]), SC.loss_reference(case, variant)
    r = run_loss(case, dtype, variant, inputs)
    want = SC.LOSS_CLAIMS[(case, dtype)]
    assert r['geo'] == want[:3], (r['geo'], want)                    # the path this case is there for, as launched
    print('loss %s dtype %d: vectorised %d, blocks %d, tiles_per_block %d' % ((case, dtype) + r['geo']))
    for k, name in enumerate(('pose', 'kd')):
        bound = SC.loss_bound(ref['losses'][k], r['geo'][1], ref['cnt'])
        err = abs(r['losses'][k] - ref['losses'][k])
        print('    %s %.17g reference %.17g |diff| %.3e allowed %.3e' % (name, r['losses'][k], ref['losses'][k], err, bound))
        assert err <= bound, (name, r['losses'][k], ref['losses'][k], err, bound)
    w0 = ((ref['w2'] == 0) & (ref['w2k'] == 0)).expand(B, H, W, J)
    checked = 0
    for s in range(S):
        if SC.skipped(variant[2], s, S):
            assert r['douts'][s] is None
            continue
        got, exp = r['douts'][s].cpu((B, H, W, J)), ref['grads'][dtype][s]
        assert bool(got.float().abs().max() > 0)
        assert _same(got, exp), 'stack %d: %d of %d gradient elements differ, max %.3e' % (
            s, int((got != exp).sum()), got.numel(), float((got.float() - exp.float()).abs().max()))
        assert not bool(got[w0].any())
        checked += 1
    assert checked == S - sum(SC.skipped(variant[2], s, S) for s in range(S))


@pytest.mark.parametrize('dtype', SC.DTYPES)
def test_loss_null_gradients_leave_the_losses_unchanged(dtype):
    """dout[s] == NULL for one stack and for all (the validation call): the same losses, byte for byte, as the full call."""
    for case in (SC.POW2_CASE, (3, 17, 12, 9, 2)):
        inputs = SC.loss_inputs(case, False)
        raws = [run_loss(case, dtype, (1, False, null, 0.25, 1.0), inputs)['raw'][0] for null in (None, 'one', 'all')]
        assert raws[0] == raws[1] == raws[2] and raws[0] != bytes(16)


@pytest.mark.parametrize('dtype', SC.DTYPES)
def test_loss_misaligned_maps_take_the_scalar_kernel_and_give_the_same_bits(dtype):
    case, variant = SC.POW2_CASE, SC.V_A
    B, J, H, W, S = case
    inputs = SC.loss_inputs(case, variant[1])
    al, mis = run_loss(case, dtype, variant, inputs), run_loss(case, dtype, variant, inputs, offset=1)
    assert al['geo'] == (1, 256, 2) and mis['geo'] == (0, B * (H * W // 64), 1)
    assert all(d.ptr() % 16 != 0 for d in mis['douts'])
    assert mis['raw'][0] == al['raw'][0]                             # cnt is a power of two: exact on either path
    for s in range(S):
        assert torch.equal(SC.bits(mis['douts'][s].cpu()), SC.bits(al['douts'][s].cpu())), 'stack %d' % s


@pytest.mark.parametrize('dtype', SC.DTYPES)
def test_loss_accumulates_and_repeats(dtype):
    case, variant = SC.POW2_CASE, SC.V_A
    inputs, ref = SC.loss_inputs(case, variant[1]), SC.loss_reference(case, variant)
    twice = run_loss(case, dtype, variant, inputs, calls=2, zero_between=False)
    assert np.array_equal(twice['losses'], 2.0 * ref['losses'])      # losses += : the caller zeroes
    again = run_loss(case, dtype, variant, inputs, calls=2)
    assert again['raw'][0] == again['raw'][1] and np.array_equal(again['losses'], ref['losses'])
    case = (33, 16, 40, 40, 1)                                       # ... and where the terms are rounded: still the same bytes
    again = run_loss(case, dtype, SC.V_B, SC.loss_inputs(case, True), calls=2)
    assert again['raw'][0] == again['raw'][1]


@pytest.mark.parametrize('dtype', SC.DTYPES)
@pytest.mark.parametrize('case', SC.GENERAL_CASES)
def test_loss_general_inputs(case, dtype):
    """test_loss's random construction and criteria on a multi-tile and on a scalar case; in bf16 every gradient element
    within one bf16 rounding of the fp64 value: |got - ref| <= 2^-8 |ref| + 2^-20 max|ref|."""
    B, J, H, W, S = case
    i = SC.general_loss_inputs(case, dtype)
    r = run_loss(case, dtype, (1, False, None, i['alpha'], 1.0), i)
    assert r['geo'] == SC.LOSS_CLAIMS[(case, dtype)][:3]
    assert abs(r['losses'][0] - i['pose']) < 1e-6 * max(1, i['pose']), (r['losses'], i['pose'])
    assert abs(r['losses'][1] - i['kd']) < 1e-6 * max(1, i['kd']), (r['losses'], i['kd'])
    for s in range(S):
        got, ref = r['douts'][s].cpu((B, H, W, J)).double(), i['grads'][s]
        mx = ref.abs().max().item()
        err = (got - ref).abs()
        tol = 1e-9 if dtype == 0 else 1e-2 * mx
        print('loss general %s dtype %d: max err %.3e (max |ref| %.3e)' % (case, dtype, err.max().item(), mx))
        assert err.max().item() <= tol + 1e-6 * mx
        if dtype == SC.BF16:
            excess = (err - (2.0 ** -8 * ref.abs() + 2.0 ** -20 * mx)).max().item()
            print('    per element: max(err - bound) = %.3e' % excess)
            assert excess <= 0, excess


# ---------------------------------------------------------------------------------------------------------------------
# fpd_adam
def run_adam(p0, grads, lrs, betas=_adam_ref.BETAS, eps=_adam_ref.EPS, grad_scale=1.0, host_schedule=False, with_lp=True, offset=0):
    """fpd_adam once per gradient.  The schedule through step_dev + lr_dev, or -- host_schedule -- bias_corr1 / bias_corr2 / lr
    in the struct with both pointers NULL.  -> dict(p, m, v, lp or None: CPU tensors, step)"""
    n = p0.numel()
    p, m, v = Guarded(n, torch.float32, p0, offset), Guarded(n, torch.float32, torch.zeros(n), offset), Guarded(n, torch.float32, torch.zeros(n), offset)
    lp = Guarded(n, torch.bfloat16, None, offset) if with_lp else None
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    lr = torch.zeros(1, device=DEV)
    for t, (g, l) in enumerate(zip(grads, lrs), start=1):
        gd = Guarded(n, torch.float32, g, offset)
        lr.fill_(l)
        a = R.AdamT()
        a.n, a.param, a.grad, a.m, a.v = n, p.ptr(), gd.ptr(), m.ptr(), v.ptr()
        a.param_lp = lp.ptr() if lp is not None else None
        a.beta1, a.beta2, a.eps, a.grad_scale = betas[0], betas[1], eps, grad_scale
        if host_schedule:
            bc1, bc2 = _adam_ref.bias_corrections(t, betas)
            a.lr, a.bias_corr1, a.bias_corr2, a.lr_dev, a.step_dev = l, float(bc1), float(bc2), None, None
        else:
            a.lr, a.bias_corr1, a.bias_corr2, a.lr_dev, a.step_dev = 0.0, 1.0, 1.0, lr.data_ptr(), step.data_ptr()
        R.check(R.lib().fpd_adam(a, R.current_stream()), 'fpd_adam')
        torch.cuda.synchronize()
        assert gd.intact()
    assert all(x is None or x.intact() for x in (p, m, v, lp)), 'a guard element was written'
    return dict(p=p.cpu(), m=m.cpu(), v=v.cpu(), lp=lp.cpu() if lp is not None else None, step=int(step.item()))


@pytest.mark.parametrize('kind', _adam_ref.STARTS)
@pytest.mark.parametrize('regime', _adam_ref.REGIMES)
def test_adam_is_as_close_to_fp64_torch_as_fp32_torch_is(regime, kind):
    n = 100003
    p0, grads = _adam_ref.start(kind, n), _adam_ref.gradients(regime, n)
    r32, r64 = _adam_ref.adam_trajectory(p0, grads), _adam_ref.adam_trajectory(p0, grads, dtype=torch.float64)
    dev = run_adam(p0, grads, _adam_ref.LRS)
    assert dev['step'] == 3
    host = run_adam(p0, grads, _adam_ref.LRS, host_schedule=True)
    assert host['step'] == 0
    for k in ('p', 'm', 'v', 'lp'):                                  # both ways of passing the schedule: the same bits
        assert torch.equal(SC.bits(dev[k]), SC.bits(host[k])), k
    e, e32 = float((dev['p'].double() - r64[0]).abs().max()), float((r32[0].double() - r64[0]).abs().max())
    print('adam %s start, %s gradients: max|ours - r64| %.3e, max|r32 - r64| %.3e, ratio %.3f' % (kind, regime, e, e32, e / e32))
    _sgd_ref.assert_as_close_as_fp32(dev['p'], r32[0], r64[0], 'parameters, %s start, %s gradients' % (kind, regime))
    # m and v: Adam at the betas the struct carries, float32(0.9) and float32(0.999) (tests/test_step_cases_cpu.py says why)
    b32 = tuple(float(np.float32(b)) for b in _adam_ref.BETAS)
    q32, q64 = _adam_ref.adam_trajectory(p0, grads, betas=b32), _adam_ref.adam_trajectory(p0, grads, betas=b32, dtype=torch.float64)
    for k, i in (('m', 1), ('v', 2)):
        print('    %s: ratio %.3f' % (k, _sgd_ref.assert_as_close_as_fp32(dev[k], q32[i], q64[i], '%s, %s start, %s gradients' % (k, kind, regime))))
    assert torch.equal(SC.bits(dev['lp']), SC.bits(dev['p'].bfloat16()))             # round to nearest even ...
    assert not torch.equal(dev['lp'].float(), dev['p'])                              # ... of values that do need rounding


def test_adam_grad_scale():
    n = 100003
    p0, grads = _adam_ref.start('zero', n), _adam_ref.gradients('small', n)
    half = [g / 2 for g in grads]
    r32, r64 = _adam_ref.adam_trajectory(p0, half), _adam_ref.adam_trajectory(p0, half, dtype=torch.float64)
    dev = run_adam(p0, grads, _adam_ref.LRS, grad_scale=0.5)
    ratio = _sgd_ref.assert_as_close_as_fp32(dev['p'], r32[0], r64[0], 'parameters, grad_scale 0.5')
    print('adam grad_scale 0.5: ratio %.3f' % ratio)
    assert torch.equal(SC.bits(dev['p']), SC.bits(run_adam(p0, half, _adam_ref.LRS)['p']))      # (a power of two: the very same run)


@pytest.mark.parametrize('n,offset,host', [(1, 0, False), (4099, 0, False), (4099, 1, True), (4099, 2, False),
                                           (4096 * 256 + 4099, 0, False), (4096 * 256 + 4099, 1, True)])
def test_adam_degenerate_trajectory_is_bit_exact(n, offset, host):
    """beta1 = beta2 = 0, eps = 0: m = g, v = g*g, p -= lr * sign(g), exact on EVERY element -- also past the 4096 x 256 threads of
    the capped grid, with param_lp, and with arenas one and two elements off a 16-byte boundary."""
    p0, grads = _adam_ref.exact_inputs(n)
    want = _adam_ref.exact_expected(p0, grads)
    r = run_adam(p0, grads, _adam_ref.EXACT_LRS, betas=(0.0, 0.0), eps=0.0, host_schedule=host, offset=offset)
    assert r['step'] == (0 if host else 3)
    for k, w in zip(('p', 'm', 'v'), want):
        assert torch.equal(SC.bits(r[k]), SC.bits(w)), '%s: %d of %d elements differ' % (k, int((r[k] != w).sum()), n)
    assert torch.equal(SC.bits(r['lp']), SC.bits(want[0].bfloat16()))


def test_adam_zero_gradients_keep_parameter_and_moments():
    """Elements whose gradient is zero from the first step on keep the bits of param, m and v under the default eps (the
    alignment gaps of the flat arena rely on it)."""
    n = 4099
    p0, grads = _adam_ref.start('randn', n), _adam_ref.gradients('small', n)
    p0[10], p0[11] = 0.0, -0.0
    quiet = torch.zeros(n, dtype=torch.bool)
    quiet[5:70] = True
    quiet[n - 3:] = True
    grads = [torch.where(quiet, torch.zeros(n), g) for g in grads]
    grads[1][6] = -0.0
    r = run_adam(p0, grads, _adam_ref.LRS)
    assert torch.equal(SC.bits(r['p'][quiet]), SC.bits(p0[quiet]))
    assert not bool(SC.bits(r['m'][quiet]).any()) and not bool(SC.bits(r['v'][quiet]).any())
    assert float((r['p'][~quiet] != p0[~quiet]).float().mean()) > 0.99 and bool((r['v'][~quiet] > 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# tables on the device
def _table(entries, struct):
    arr = (struct * len(entries))(*entries)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


@pytest.mark.parametrize('dtype', SC.DTYPES)
@pytest.mark.parametrize('name', sorted(SC.WPREP_TABLES))
def test_weight_prep_is_bit_exact(name, dtype):
    t = SC.tdt(dtype)
    ents, bufs = [], []
    for k, (K, Rr, S, Cc, mode) in enumerate(SC.WPREP_TABLES[name]):
        w = SC.wprep_master(K, Rr, S, Cc, k)
        n = w.numel()
        src = Guarded(n, torch.float32, w)
        wf = Guarded(n, t) if mode in ('both', 'fwd') else None
        wb = Guarded(n, t) if mode in ('both', 'bwd') else None
        e = R.WprepEntryT()
        e.w, e.w_fwd, e.w_bwd = src.ptr(), wf.ptr() if wf else None, wb.ptr() if wb else None
        e.K, e.R, e.S, e.C = K, Rr, S, Cc
        ents.append(e)
        bufs.append((w, src, wf, wb))
    table = _table(ents, R.WprepEntryT)
    mx = max(b[0].numel() for b in bufs)
    R.check(R.lib().fpd_weight_prep(table.data_ptr(), len(ents), mx, dtype, R.current_stream()), 'fpd_weight_prep')
    torch.cuda.synchronize()
    for k, (w, src, wf, wb) in enumerate(bufs):
        ref_f, ref_b = SC.wprep_reference(w, dtype)
        label = '%s entry %d %s' % (name, k, SC.WPREP_TABLES[name][k])
        assert src.intact() and torch.equal(SC.bits(src.cpu()), SC.bits(w.reshape(-1))), label
        for got, ref, what in ((wf, ref_f, 'w_fwd'), (wb, ref_b, 'w_bwd')):
            if got is None:
                continue
            assert got.intact(), label + ': a guard element of %s was written' % what
            bad = SC.bits(got.cpu()) != SC.bits(ref.reshape(-1))
            assert not bool(bad.any()), '%s %s: %d of %d bit patterns differ, first at %d' % (
                label, what, int(bad.sum()), bad.numel(), int(torch.nonzero(bad)[0]))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', sorted(SC.BNUPD_TABLES))
def test_bn_update_running(kind):
    from fpd_amd import executor as E, graph as Gr
    assert Gr.STATS_REPLICAS == SC.RS
    spec = SC.BNUPD_TABLES[kind]
    A = E.Arenas(DEV, 0)
    A.alloc('stats', sum(SC.RS * 2 * c for c, _, _ in spec))
    ents, items, off = [], [], 0
    for k, (Cc, count, has_nbt) in enumerate(spec):
        i = SC.bnupd_inputs(kind, k, Cc, count)
        buf = Gr.Buf('stats', off, (SC.RS, 2, Cc))
        off += SC.RS * 2 * Cc
        A.stats_write(buf, i['stats'])                               # the full [R][2][C]: every replica carries a share
        rm, rv = Guarded(Cc, torch.float32, i['rmean']), Guarded(Cc, torch.float32, i['rvar'])
        nbt = Guarded(1, torch.int64, torch.zeros(1), sentinel=-77)
        e = R.BnupdEntryT()
        e.stats, e.running_mean, e.running_var = A.ptr(buf), rm.ptr(), rv.ptr()
        e.num_batches_tracked = nbt.ptr() if has_nbt else None
        e.count, e.momentum, e.C = float(count), SC.BN_MOMENTUM, Cc
        ents.append(e)
        items.append((i, rm, rv, nbt, has_nbt))
    table = _table(ents, R.BnupdEntryT)
    raw_before = A.tensor('stats').clone()
    R.check(R.lib().fpd_bn_update_running(table.data_ptr(), len(ents), R.current_stream()), 'fpd_bn_update_running')
    torch.cuda.synchronize()
    assert torch.equal(A.tensor('stats'), raw_before)
    for k, (i, rm, rv, nbt, has_nbt) in enumerate(items):
        label = '%s entry %d %s' % (kind, k, spec[k])
        ref = SC.bnupd_reference(i)
        assert rm.intact() and rv.intact() and nbt.intact(), label
        gm, gv = rm.cpu(), rv.cpu()
        if kind == 'dyadic':
            assert torch.equal(SC.bits(gm), SC.bits(ref[0].float())), label + ' running_mean'
            assert torch.equal(SC.bits(gv), SC.bits(ref[1].float())), label + ' running_var'
        else:
            bm, bv = SC.bnupd_bound(i, ref)
            em, ev = (gm.double() - ref[0]).abs(), (gv.double() - ref[1]).abs()
            print('%s: running_mean max err / bound %.3f, running_var %.3f' % (label, float((em / bm).max()), float((ev / bv).max())))
            assert bool((em <= bm).all()) and bool((ev <= bv).all()), label
            assert bool((ref[2][i['neg']] < 0).all())                   # the clamped channels: 0.9 running_var, inside the same bound
        assert int(nbt.cpu().item()) == (1 if has_nbt else 0), label
    R.check(R.lib().fpd_bn_update_running(table.data_ptr(), len(ents), R.current_stream()), 'fpd_bn_update_running')
    torch.cuda.synchronize()
    for i, rm, rv, nbt, has_nbt in items:
        assert int(nbt.cpu().item()) == (2 if has_nbt else 0) and nbt.intact() and rm.intact() and rv.intact()


# ---------------------------------------------------------------------------------------------------------------------
def test_casts_through_the_grid_stride_loop():
    n = SC.LOOP_N
    l, st = R.lib(), R.current_stream()
    x32, x16 = SC.cast_source_f32(n), SC.cast_source_bf16(n)
    for src, sd, dd in ((x32, 0, 1), (x16, 1, 0), (x32, 0, 0), (x16, 1, 1)):
        s = Guarded(n, src.dtype, src)
        d = Guarded(n, SC.tdt(dd))
        R.check(l.fpd_cast(s.ptr(), d.ptr(), n, sd, dd, st), 'fpd_cast')
        torch.cuda.synchronize()
        got, ref = d.cpu(), src.to(SC.tdt(dd))
        nan = torch.isnan(ref.float())
        assert d.intact() and s.intact(), (sd, dd)
        assert bool(torch.isnan(got.float())[nan].all()) and (bool(nan.any()) or sd == 1)      # NaN stays NaN (the bf16 source has none)
        bad = (SC.bits(got) != SC.bits(ref)) & ~nan
        assert not bool(bad.any()), 'cast %d -> %d: %d of %d bit patterns differ, first at %d (%r)' % (
            sd, dd, int(bad.sum()), n, int(torch.nonzero(bad)[0]), float(src[int(torch.nonzero(bad)[0])]))


@pytest.mark.parametrize('dtype', SC.DTYPES)
@pytest.mark.parametrize('shape', SC.LAYOUT_SHAPES)
def test_layout_changes(shape, dtype):
    N, Cc, H, W = shape
    n = N * Cc * H * W
    l, st, t = R.lib(), R.current_stream(), SC.tdt(dtype)
    gen = SC.gen_for('layout', shape)
    src = torch.randn(N, Cc, H, W, generator=gen)
    src.view(-1)[:14] = SC.special_values()
    s = Guarded(n, torch.float32, src)
    d = Guarded(n, t)
    R.check(l.fpd_nchw_to_nhwc(s.ptr(), d.ptr(), N, Cc, H, W, dtype, st), 'fpd_nchw_to_nhwc')
    torch.cuda.synchronize()
    nhwc = src.permute(0, 2, 3, 1).contiguous().to(t)
    assert d.intact() and s.intact()
    assert torch.equal(SC.bits(d.cpu()), SC.bits(nhwc.reshape(-1)))
    back = Guarded(n, torch.float32)
    R.check(l.fpd_nhwc_to_nchw(d.ptr(), back.ptr(), N, Cc, H, W, dtype, st), 'fpd_nhwc_to_nchw')
    torch.cuda.synchronize()
    assert back.intact() and d.intact()
    assert torch.equal(SC.bits(back.cpu()), SC.bits(nhwc.permute(0, 3, 1, 2).contiguous().float().reshape(-1)))
