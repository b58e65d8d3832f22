"""JointsKLDLoss on the MI355X (csrc/loss_kl.hip): fpd_loss_kl, core.loss.JointsKLDLoss, FusedFPDStep(kl=...) and the
core.function entry points against the float64 closed form tests/_kl_ref.py, evaluated on the very values the kernel read.

The accuracy bar is measured in the test, not fixed: on the same shapes, weights and temperatures, over 8 seeds, the largest
error that torch's float32 CPU evaluation of the same composition (F.kl_div of F.log_softmax / F.softmax, F.mse-like sums,
autograd) makes against float64 -- relative error for the two loss scalars, relative L2 for the gradient of every stack.  The
kernel may be at most 4 x that (hardware exp against libm's, another summation order).  A bf16 gradient additionally gets one
bf16 ulp per element: one rounding, which an fp32 error can push across a tie.

Measured on an MI355X, largest over the cases of ACCURACY below (`torch fp32` is the bar before the factor 4; relative error of
the pose loss / of the kd loss / relative L2 of the gradient):
    fp32 maps   torch fp32 7.9e-06 / 2.4e-07 / 4.7e-07    kernel 1.5e-07 / 2.1e-08 / 1.1e-07   (worst kernel : torch 0.39 / 0.09 / 0.91)
    bf16 maps   torch fp32 3.8e-06 / 8.3e-06 / 2.6e-06    kernel 4.8e-08 / 7.4e-08 / 1.7e-03   (gradient: the one bf16 rounding)
    +-100 at T = 0.05 (fp32)   torch fp32 4.8e-07 / 9.2e-08 / 4.8e-06    kernel 3.6e-08 / 4.4e-08 / 4.0e-08
    one-hot reference row, kd loss   torch fp32 1.4e-07    kernel 2.9e-08
    class (loss / gradient)   torch fp32 1.5e-06 / 8.7e-07    class 2.4e-07 / 2.7e-07
    fused step (fp32, tiny pair)   torch fp32 9.5e-08 / 1.8e-07 / 1.7e-07    kernel 2.8e-10 / 8.3e-10 / 6.7e-08
Every test prints its own figures (pytest -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _cases, _kl_ref

pytestmark = pytest.mark.gpu

SHAPES = {   # B, J, H, W, S
    'A': (2, 5, 8, 8, 1),        # scalar path, one chunk, one partial tile
    'B': (3, 17, 20, 24, 2),     # odd J, 3.75 tiles: four chunks per image, merged in the second launch
    'C': (2, 16, 64, 64, 4),     # vector path, the benchmark's map
    'D': (1, 32, 8, 8, 1),       # the largest J
    'E': (5, 16, 128, 128, 1),   # 5 x 128 tiles > 512 blocks: a block walks two tiles (and turns the target again in its second pass)
    'F': (2, 16, 12, 9, 2),      # run one element off the 16-byte grid: J a multiple of the vector on the scalar path, 16 joint lanes
}
CHUNKS = {'A': 1, 'B': 4, 'C': 32, 'D': 1, 'E': 64, 'F': 1}
SEEDS = 8
MARGIN = 4.0


def _tdt(dtype):
    return torch.bfloat16 if dtype == 1 else torch.float32


def _nchw64(t):
    """NHWC tensor (any float dtype) -> float64 numpy NCHW"""
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous().numpy()


def run_kl(outs, teacher, target, w, temps, alpha, dtype, w_kd=None, nchw=1, dout=True, grad_scale=1.0, keep=False, offset=0):
    """One fpd_loss_kl call.  outs / teacher: NHWC CPU tensors already in the storage type; target: NCHW float32 CPU tensor;
    w / w_kd: [B,J] float32; temps: (T_pose or None, T_kd or None), None = that term is MSE.  offset: every map and gradient
    starts that many elements behind a 16-byte boundary, between guard elements that have to stay intact.
    -> dict(losses [2] float64, douts: NCHW float64 numpy, raw: the gradient buffers' bytes, scratch, chunks)."""
    from fpd_amd import runtime as R
    dev = torch.device('cuda:0')
    B, H, W, J = outs[0].shape
    S = len(outs)
    k = R.LossKlT()
    a = k.base
    a.B, a.J, a.H, a.W, a.S, a.dtype, a.target_nchw, a.alpha, a.grad_scale = B, J, H, W, S, dtype, nchw, alpha, grad_scale
    guarded = []
    if offset:
        from tests.test_step_kernels_gpu import Guarded
        guarded = [Guarded(o.numel(), o.dtype, o, offset) for o in outs + [teacher]] + [Guarded(o.numel(), o.dtype, None, offset) for o in outs]
        d_outs, d_t, d_douts = ([x.t.view(outs[0].shape) for x in guarded[i:j]] for i, j in ((0, S), (S, S + 1), (S + 1, 2 * S + 1)))
        d_t = d_t[0]
        assert all(x.data_ptr() % 16 == offset * x.element_size() for x in d_outs + d_douts + [d_t])
    else:
        d_outs = [o.to(dev).contiguous() for o in outs]
        d_douts = [torch.full_like(o, float('nan')) for o in d_outs]
        d_t = teacher.to(dev).contiguous()
    for i in range(S):
        a.out[i] = d_outs[i].data_ptr()
        a.dout[i] = d_douts[i].data_ptr() if dout else None
    d_tg = (target if nchw else target.permute(0, 2, 3, 1)).contiguous().to(dev)
    d_w = w.float().contiguous().to(dev)
    d_wk = w_kd.float().contiguous().to(dev) if w_kd is not None else None
    losses = torch.zeros(2, dtype=torch.float64, device=dev)
    a.teacher, a.target, a.weight, a.losses = d_t.data_ptr(), d_tg.data_ptr(), d_w.data_ptr(), losses.data_ptr()
    a.weight_kd = d_wk.data_ptr() if d_wk is not None else None
    k.kl_pose, k.kl_kd = int(temps[0] is not None), int(temps[1] is not None)
    k.temp_pose, k.temp_kd = temps[0] or 0.0, temps[1] or 0.0      # (the temperature of an MSE term is not looked at)
    nbytes = R.lib().fpd_loss_kl_scratch_bytes(a)
    slab = ((3 * S + 4) * J + 2) * 8
    assert nbytes > 0 and nbytes % (B * slab) == 0
    scratch = torch.full((nbytes // 8,), float('nan'), dtype=torch.float64, device=dev)
    k.scratch, k.scratch_bytes = scratch.data_ptr(), nbytes
    calls = 2 if keep else 1
    raws = []
    for _ in range(calls):
        losses.zero_()
        R.check(R.lib().fpd_loss_kl(k, R.current_stream()), 'fpd_loss_kl')
        torch.cuda.synchronize()
        raws.append((losses.cpu().numpy().tobytes(), [d.cpu().view(torch.uint8).numpy().tobytes() for d in d_douts],
                     scratch.cpu().numpy().tobytes()))
    assert all(x.intact() for x in guarded)
    return {'losses': losses.cpu().numpy(), 'douts': [_nchw64(d) for d in d_douts], 'raws': raws,
            'chunks': nbytes // (B * slab)}


def reference(outs, teacher, target, w, temps, alpha, w_kd=None, grad_scale=1.0):
    wp = w.double().numpy()
    wk = w_kd.double().numpy() if w_kd is not None else wp
    return _kl_ref.fused([_nchw64(o) for o in outs], target.double().numpy(), _nchw64(teacher), wp, wk, temps[0], temps[1], alpha,
                         grad_scale)


def torch_f32(outs, teacher, target, w, temps, alpha, w_kd=None, grad_scale=1.0):
    """The same composition in float32 by torch on the CPU, gradient by autograd -> dict(pose, kd, grads)"""
    wp = w.float()
    wk = w_kd.float() if w_kd is not None else wp
    tg, tc = target.float(), teacher.float().permute(0, 3, 1, 2)
    leaves = [o.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for o in outs]
    B, J, H, W = leaves[0].shape

    def term(s, r, wt, T):
        if T is None:
            return 0.5 * ((s * wt[:, :, None, None] - r * wt[:, :, None, None]) ** 2).mean()
        s2, r2 = s.reshape(B * J, H * W), r.reshape(B * J, H * W)
        rows = F.kl_div(F.log_softmax(s2 / T, 1), F.softmax(r2 / T, 1), reduction='none').sum(1)
        return T * T * (wt.reshape(-1) * rows).sum() / (B * J)
    pose = sum(term(s, tg, wp, temps[0]) for s in leaves)
    kd = sum(term(s, tc, wk, temps[1]) for s in leaves)
    (grad_scale * ((1.0 - alpha) * pose + alpha * kd)).backward()
    return {'pose': pose.item(), 'kd': kd.item(), 'grads': [s.grad.double().numpy() for s in leaves]}


def errors(got_pose, got_kd, got_grads, ref):
    rel = lambda v, r: abs(v - r) / abs(r) if r != 0 else abs(v)
    l2 = lambda g, r: float(np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-300))
    return rel(got_pose, ref['pose']), rel(got_kd, ref['kd']), max(l2(g, r) for g, r in zip(got_grads, ref['grads']))


def make_inputs(seed, B, J, H, W, S, dtype, kd_weights=False, amp=1.0):
    """seeded random inputs, already rounded to the storage type; the weights contain 0 and 1.5"""
    gen = torch.Generator().manual_seed(seed)
    scale = amp * (0.2 + 0.8 * torch.rand(1, 1, 1, J, generator=gen))          # joints of different sharpness
    outs = [(torch.randn(B, H, W, J, generator=gen) * scale).to(_tdt(dtype)) for _ in range(S)]
    teacher = (torch.randn(B, H, W, J, generator=gen) * scale).to(_tdt(dtype))
    target = torch.rand(B, J, H, W, generator=gen) * amp
    w = (torch.rand(B, J, generator=gen) * 1.5) * (torch.rand(B, J, generator=gen) < 0.8)
    w[0, 0], w[0, 1] = 0.0, 1.5
    w_kd = (0.5 + torch.rand(B, J, generator=gen)) if kd_weights else None
    if w_kd is not None:
        w_kd[0, 1], w_kd[0, 2] = 0.0, 1.5
    return outs, teacher, target, w, w_kd


def measured_bar(shape, dtype, temps, alpha, kd_weights, grad_scale, amp=1.0, seed0=100):
    """the largest error of torch's float32 evaluation against float64 over SEEDS seeds of the same kind of inputs"""
    bar = np.zeros(3)
    for i in range(SEEDS):
        outs, teacher, target, w, w_kd = make_inputs(seed0 + i, *shape, dtype, kd_weights, amp)
        ref = reference(outs, teacher, target, w, temps, alpha, w_kd, grad_scale)
        f32 = torch_f32(outs, teacher, target, w, temps, alpha, w_kd, grad_scale)
        bar = np.maximum(bar, errors(f32['pose'], f32['kd'], f32['grads'], ref))
    return bar


def bf16_ulp(r):
    """spacing of bf16 (8 significant bits) at |r|, elementwise"""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(r), 2.0 ** -126))) - 7)


def check(got, ref, bar, dtype, label, grads=True):
    e = errors(got['losses'][0], got['losses'][1], got['douts'] if grads else ref['grads'], ref)
    print('%s: torch fp32 pose %.2e kd %.2e grad %.2e | kernel pose %.2e kd %.2e grad %.2e' % ((label,) + tuple(bar) + e))
    assert np.isfinite(got['losses']).all()
    assert e[0] <= MARGIN * bar[0] and e[1] <= MARGIN * bar[1], (label, e, bar)
    if not grads:
        return
    if dtype == 0:
        assert e[2] <= MARGIN * bar[2], (label, e, bar)
    else:       # one rounding of a value that carries the fp32 error: a bf16 ulp + the fp32 bar taken at the largest element
        for g, r in zip(got['douts'], ref['grads']):
            assert np.isfinite(g).all()
            assert (np.abs(g - r) <= bf16_ulp(r) + MARGIN * bar[2] * np.abs(r).max()).all(), (label, np.abs(g - r).max())


# ---- accuracy ---------------------------------------------------------------------------------------------------------------
ACCURACY = [   # shape, dtype, target_nchw, (T_pose, T_kd), alpha, kwargs
    ('A', 0, 1, (None, 1.0), 0.5, {}),
    ('A', 1, 0, (0.05, None), 0.0, {}),
    ('A', 0, 1, (4.0, 0.05), 1.0, {'kd_weights': True}),
    ('A', 1, 1, (None, 4.0), 0.5, {'dout': False}),
    ('B', 0, 1, (None, 1.0), 0.5, {'kd_weights': True, 'grad_scale': 0.5}),
    ('B', 1, 0, (1.0, 4.0), 0.5, {}),
    ('B', 0, 0, (0.05, None), 1.0, {}),
    ('B', 1, 1, (None, 0.05), 0.5, {'kd_weights': True}),
    ('C', 1, 1, (None, 1.0), 0.5, {}),
    ('C', 0, 1, (1.0, 1.0), 0.5, {'grad_scale': 0.5}),
    ('C', 1, 0, (4.0, None), 0.0, {'kd_weights': True}),
    ('D', 0, 1, (None, 1.0), 0.5, {}),
    ('D', 1, 0, (1.0, 0.05), 1.0, {'kd_weights': True}),
    ('E', 0, 1, (1.0, 0.05), 0.5, {}),
    ('E', 1, 0, (None, 1.0), 0.5, {}),
    ('F', 0, 1, (1.0, 4.0), 0.5, {'offset': 1}),
    ('F', 1, 0, (None, 1.0), 0.5, {'offset': 1}),
]


@pytest.mark.parametrize('case', ACCURACY, ids=lambda c: '%s-%s-%s-T%s,%s-a%s' % (c[0], 'bf16' if c[1] else 'fp32', 'nchw' if c[2] else 'nhwc', c[3][0], c[3][1], c[4]))
def test_kernel_is_within_four_times_torch_float32_of_float64(case):
    name, dtype, nchw, temps, alpha, kw = case
    shape = SHAPES[name]
    gs, kdw = kw.get('grad_scale', 1.0), kw.get('kd_weights', False)
    bar = measured_bar(shape, dtype, temps, alpha, kdw, gs)
    outs, teacher, target, w, w_kd = make_inputs(100, *shape, dtype, kdw)
    ref = reference(outs, teacher, target, w, temps, alpha, w_kd, gs)
    got = run_kl(outs, teacher, target, w, temps, alpha, dtype, w_kd=w_kd, nchw=nchw, dout=kw.get('dout', True), grad_scale=gs,
                 offset=kw.get('offset', 0))
    assert got['chunks'] == CHUNKS[name]
    check(got, ref, bar, dtype, 'accuracy %s' % (case,), grads=kw.get('dout', True))
    if not kw.get('dout', True):
        assert all(np.isnan(d).all() for d in got['douts'])                 # forward only: nothing written
    if w_kd is None:
        assert all((g[0, 0] == 0).all() for g in got['douts'] if kw.get('dout', True))     # a zero weight: no gradient


def test_the_weight_enters_a_kl_term_once():
    """Doubling the weights doubles a KL term (and quadruples an MSE term): both exact in binary arithmetic."""
    outs, teacher, target, w, _ = make_inputs(7, *SHAPES['B'], 0)
    a = run_kl(outs, teacher, target, w, (None, 1.0), 0.5, 0)
    b = run_kl(outs, teacher, target, 2.0 * w, (None, 1.0), 0.5, 0)
    # (every block rounds its share to a multiple of 2^-44 before it adds it: up to a unit per block, 12 blocks here)
    assert abs(b['losses'][1] - 2.0 * a['losses'][1]) <= 64 * 2.0 ** -44 and abs(b['losses'][0] - 4.0 * a['losses'][0]) <= 64 * 2.0 ** -44
    assert a['losses'][1] > 1e-4
    a = run_kl(outs, teacher, target, w, (None, 1.0), 1.0, 0)
    b = run_kl(outs, teacher, target, 2.0 * w, (None, 1.0), 1.0, 0)
    assert all(np.array_equal(2.0 * x, y) for x, y in zip(a['douts'], b['douts']))


# ---- exact properties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [0, 1])
@pytest.mark.parametrize('T', [0.05, 1.0, 4.0])
@pytest.mark.parametrize('name', ['A', 'B', 'C', 'D'])
def test_same_map_twice_gives_exactly_zero(name, T, dtype):
    B, J, H, W, _ = SHAPES[name]
    outs, _, target, w, _ = make_inputs(11, B, J, H, W, 1, dtype)
    got = run_kl(outs, outs[0].clone(), target, w, (None, T), 1.0, dtype)
    assert got['losses'][1] == 0.0 and got['losses'][0] > 0
    assert (got['douts'][0] == 0).all()


@pytest.mark.parametrize('dtype,J', [(0, 16), (1, 16), (1, 4), (0, 2)])
def test_alpha_zero_with_a_kl_distillation_term_equals_fpd_loss_bitwise_on_dyadic_inputs(dtype, J):
    """maps and targets in {-1, -0.5, 0, 0.5, 1} (tests/_exact_inputs.py's activations), weights in {0, 0.5, 1}, B*J*hw a power of
    two: every MSE product and sum is exact, and with alpha = 0 the KL term adds 0 * finite to the gradient"""
    from fpd_amd import runtime as R
    from tests import _exact_inputs as X
    gen = X.seed('kl', dtype, J)
    B, H, W, S = 2, 8, 8, 2
    outs = [X.small(gen, B, H, W, J).to(_tdt(dtype)) for _ in range(S)]
    teacher = X.small(gen, B, H, W, J).to(_tdt(dtype))
    target = X.small(gen, B, J, H, W).float()
    w = X.pick(gen, [0.0, 0.5, 1.0], B * J).float().view(B, J)
    got = run_kl(outs, teacher, target, w, (None, 1.0), 0.0, dtype)
    dev = torch.device('cuda:0')
    a = R.LossT()
    a.B, a.J, a.H, a.W, a.S, a.dtype, a.target_nchw, a.alpha, a.grad_scale = B, J, H, W, S, dtype, 1, 0.0, 1.0
    d_outs = [o.to(dev) for o in outs]
    d_douts = [torch.zeros_like(o) for o in d_outs]
    for i in range(S):
        a.out[i], a.dout[i] = d_outs[i].data_ptr(), d_douts[i].data_ptr()
    d_t, d_tg, d_w = teacher.to(dev), target.to(dev), w.to(dev)
    losses = torch.zeros(2, dtype=torch.float64, device=dev)
    a.teacher, a.target, a.weight, a.losses = d_t.data_ptr(), d_tg.data_ptr(), d_w.data_ptr(), losses.data_ptr()
    R.check(R.lib().fpd_loss(a, R.current_stream()), 'fpd_loss')
    torch.cuda.synchronize()
    ref = reference(outs, teacher, target, w, (None, 1.0), 0.0)
    assert losses[0].item() == got['losses'][0] == ref['pose'] and got['losses'][0] > 0
    assert np.isfinite(got['losses'][1]) and got['losses'][1] > 0
    for d, g in zip(d_douts, got['douts']):
        assert np.array_equal(_nchw64(d), g) and np.abs(g).max() > 0


@pytest.mark.parametrize('dtype', [0, 1])
def test_two_calls_on_the_same_buffers_give_identical_bytes(dtype):
    outs, teacher, target, w, w_kd = make_inputs(13, *SHAPES['B'], dtype, True)
    got = run_kl(outs, teacher, target, w, (1.0, 0.05), 0.5, dtype, w_kd=w_kd, keep=True)
    assert got['chunks'] == 4 and got['raws'][0] == got['raws'][1]
    assert not np.isnan(np.frombuffer(got['raws'][0][2], np.float64)).any()     # every slab of the scratch is written


# ---- range and refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [0, 1])
def test_maps_of_plus_minus_100_at_T_0_05_stay_finite_and_inside_the_bar(dtype):
    shape = SHAPES['B']
    temps, alpha = (0.05, 0.05), 0.5
    bar = measured_bar(shape, dtype, temps, alpha, False, 1.0, amp=100.0)
    outs, teacher, target, w, _ = make_inputs(100, *shape, dtype, amp=100.0)
    assert max(float(o.float().abs().max()) for o in outs) > 100.0
    ref = reference(outs, teacher, target, w, temps, alpha)
    got = run_kl(outs, teacher, target, w, temps, alpha, dtype)
    assert all(np.isfinite(g).all() for g in got['douts'])
    check(got, ref, bar, dtype, 'range +-100 dtype %d' % dtype)


@pytest.mark.parametrize('dtype', [0, 1])
@pytest.mark.parametrize('T', [0.05, 1.0])
def test_a_one_hot_reference_row_gives_minus_w_T2_log_p(T, dtype):
    B, J, H, W, _ = SHAPES['B']
    outs, _, target, w, _ = make_inputs(17, B, J, H, W, 1, dtype)
    teacher = torch.full((B, H, W, J), -1e4).to(_tdt(dtype))
    hot = [(3 * j + 5) % (H * W) for j in range(J)]                         # a pixel per joint, in different tiles
    for j, x in enumerate(hot):
        teacher[:, x // W, x % W, j] = 0.0
    got = run_kl(outs, teacher, target, w, (None, T), 1.0, dtype)
    assert np.isfinite(got['losses']).all() and np.isfinite(got['douts'][0]).all()
    s = _nchw64(outs[0]).reshape(B, J, H * W) / T
    lse = s.max(2) + np.log(np.exp(s - s.max(2, keepdims=True)).sum(2))
    logp = np.stack([s[:, j, hot[j]] for j in range(J)], 1) - lse
    want = (w.double().numpy() * (-T * T * logp)).sum() / (B * J)
    ref = reference(outs, teacher, target, w, (None, T), 1.0)
    assert abs(ref['kd'] - want) <= 1e-12 * abs(want)                       # (the closed form itself)
    bar = 0.0                                                               # torch float32 on one-hot rows, 8 draws of the student
    for i in range(SEEDS):
        o_i = make_inputs(17 + i, B, J, H, W, 1, dtype)[0]
        r_i = reference(o_i, teacher, target, w, (None, T), 1.0)
        f_i = torch_f32(o_i, teacher, target, w, (None, T), 1.0)
        assert np.isfinite(f_i['kd'])
        bar = max(bar, abs(f_i['kd'] - r_i['kd']) / abs(r_i['kd']))
    print('one-hot T=%g dtype %d: torch fp32 kd %.2e | kernel kd %.2e' % (T, dtype, bar, abs(got['losses'][1] - want) / abs(want)))
    assert abs(got['losses'][1] - want) <= MARGIN * bar * abs(want), (got['losses'][1], want, bar)


def test_refusals():
    from fpd_amd import runtime as R
    outs, teacher, target, w, _ = make_inputs(19, *SHAPES['A'], 0)
    _raw_call(outs, teacher, target, w, (False, True), (0.0, 1.0))          # (accepted: the temperature of an MSE term is not read)
    for flags, temps, what in (((False, False), (1.0, 1.0), 'neither'), ((False, True), (1.0, 0.0), 'temperature'),
                               ((True, True), (0.0, 1.0), 'temperature'), ((False, True), (1.0, -1.0), 'temperature')):
        with pytest.raises(R.FpdError, match=what):
            _raw_call(outs, teacher, target, w, flags, temps)
    o33 = [torch.zeros(1, 4, 4, 33)]
    with pytest.raises(R.FpdError, match='J=33'):
        _raw_call(o33, o33[0], torch.zeros(1, 33, 4, 4), torch.ones(1, 33), (False, True), (1.0, 1.0))


def _raw_call(outs, teacher, target, w, flags, temps):
    from fpd_amd import runtime as R
    dev = torch.device('cuda:0')
    B, H, W, J = outs[0].shape
    k = R.LossKlT()
    a = k.base
    a.B, a.J, a.H, a.W, a.S, a.dtype, a.target_nchw, a.alpha, a.grad_scale = B, J, H, W, 1, 0, 1, 0.5, 1.0
    keep = [outs[0].to(dev), teacher.to(dev), target.to(dev), w.to(dev), torch.zeros(2, dtype=torch.float64, device=dev),
            torch.zeros(1 << 16, dtype=torch.float64, device=dev)]
    a.out[0], a.teacher, a.target, a.weight, a.losses = (t.data_ptr() for t in keep[:5])
    k.kl_pose, k.kl_kd = int(flags[0]), int(flags[1])
    k.temp_pose, k.temp_kd = temps
    k.scratch, k.scratch_bytes = keep[5].data_ptr(), keep[5].numel() * 8
    R.check(R.lib().fpd_loss_kl(k, R.current_stream()), 'fpd_loss_kl')
    torch.cuda.synchronize()


# ---- the class -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_w,T', [(True, 1.0), (True, 0.05), (False, 4.0)])
def test_class_forward_and_backward_match_the_torch_composition(use_w, T):
    from fpd_amd.lib.core.loss import JointsKLDLoss
    B, J, H, W = 3, 17, 12, 9
    bar = np.zeros(2)
    for i in range(SEEDS):
        gen = torch.Generator().manual_seed(200 + i)
        out, tg = torch.randn(B, J, H, W, generator=gen), torch.rand(B, J, H, W, generator=gen)
        wt = torch.rand(B, J, 1, generator=gen) * 1.5
        wt[0, 0], wt[0, 1] = 0.0, 1.5
        wn = wt[:, :, 0].numpy() if use_w else np.ones((B, J))
        l64, g64 = _kl_ref.torch_composition(out.numpy(), tg.numpy(), wn, T, torch.float64)
        l32, g32 = _kl_ref.torch_composition(out.numpy(), tg.numpy(), wn, T, torch.float32)
        bar = np.maximum(bar, [abs(l32 - l64) / abs(l64), np.linalg.norm(g32 - g64) / np.linalg.norm(g64)])
        if i == 0:
            first = (out, tg, wt, l64, g64)
    out, tg, wt, l64, g64 = first
    crit = JointsKLDLoss(use_w, temperature=T).cuda()
    od = out.cuda().requires_grad_(True)
    loss = crit(od, tg.cuda(), wt.cuda())
    assert loss.dim() == 0
    (2.0 * loss).backward()
    torch.cuda.synchronize()
    e = (abs(loss.item() - l64) / abs(l64), np.linalg.norm(od.grad.cpu().double().numpy() - 2.0 * g64) / np.linalg.norm(2.0 * g64))
    print('class T=%g use_w=%s: torch fp32 loss %.2e grad %.2e | class loss %.2e grad %.2e' % ((T, use_w) + tuple(bar) + e))
    # the class returns the loss as a float32 scalar: half an ulp of that on top
    assert e[0] <= MARGIN * bar[0] + 2.0 ** -24 and e[1] <= MARGIN * bar[1], (e, bar)
    if use_w:
        assert (od.grad[0, 0] == 0).all()


# ---- the fused step ---------------------------------------------------------------------------------------------------------
def _tiny_step(kl, **kw):
    from fpd_amd import executor as E
    from tests.test_model_gpu import build_models
    c, gold, student, teacher = build_models('tiny')
    if kw.pop('pass_none', False) or kl is not None:
        kw['kl'] = kl
    step = E.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, c['batch'],
                          c['image'][1], c['image'][0], alpha=0.5, **kw)
    return c, student, teacher, step


def test_fused_step_with_kl_matches_the_reference_on_its_own_maps():
    """fp32 step.  The bar is the measured one again: torch's float32 evaluation on the step's OWN maps and on 7 further draws of
    maps of the same shape and spread."""
    from fpd_amd import runtime as R
    T = 0.5
    c, student, teacher, step = _tiny_step((None, T))
    assert step.kl == (None, T)
    x, tg, tw = _cases.batch('tiny', 0)
    step.set_batch(x, tg, tw)
    step.teacher_async(x)
    s = step.student
    torch.cuda.current_stream().wait_event(step.ev_t[0])
    s.run('prep'); s.run('fwd'); s.run('mid')
    pose, kd, _ = step.losses()
    S = c['s'][1]
    outs = [s.output_view(i).float().cpu() for i in range(S)]
    tmap = step.tmap[0].view(outs[0].shape).float().cpu()
    w = tw[:, :, 0]
    ref = reference(outs, tmap, tg, w, (None, T), 0.5)
    f32 = torch_f32(outs, tmap, tg, w, (None, T), 0.5)
    bar = np.array(errors(f32['pose'], f32['kd'], f32['grads'], ref))
    gen = torch.Generator().manual_seed(5)
    for _ in range(SEEDS - 1):
        o2 = [o + 0.05 * float(o.std()) * torch.randn(o.shape, generator=gen) for o in outs]
        r2 = reference(o2, tmap, tg, w, (None, T), 0.5)
        f2 = torch_f32(o2, tmap, tg, w, (None, T), 0.5)
        bar = np.maximum(bar, errors(f2['pose'], f2['kd'], f2['grads'], r2))
    got = {'losses': np.array([pose, kd]), 'douts': [_nchw64(s.out_grad_view(i)) for i in range(S)]}
    check(got, ref, bar, 0, 'fused step')
    assert kd > 0
    # the plan: same size as the default step's, the loss op exchanged; kl=None and no kl at all are the default plan
    _, _, _, plain = _tiny_step(None)
    _, _, _, none = _tiny_step(None, pass_none=True)
    types = lambda st: [st.student.plan.op_type(i) for i in range(len(st.student.plan))]
    assert types(none) == types(plain) and none.launches_per_step() == plain.launches_per_step() and none.kl is None
    assert len(step.student.plan) == len(plain.student.plan) and step.launches_per_step() == plain.launches_per_step()
    assert types(plain).count(R.OP_LOSS) == 2 and R.OP_LOSS_KL not in types(plain) and 'kl_scratch' not in plain.student.A.t
    assert 'kl_scratch' not in none.student.A.t and 'ohkm_scratch' not in step.student.A.t
    assert types(step).count(R.OP_LOSS_KL) == 2 and R.OP_LOSS not in types(step)
    assert [t for t in types(step) if t != R.OP_LOSS_KL] == [t for t in types(plain) if t != R.OP_LOSS]


def test_fused_step_with_kl_is_bit_repeatable():
    runs = []
    for _ in range(2):
        c, student, teacher, step = _tiny_step((None, 0.5), lr=2.5e-4)
        step.set_batch(*_cases.batch('tiny', 0))
        step.step()
        torch.cuda.synchronize()
        runs.append((step.student.A.tensor('losses')[:2].cpu().clone(),
                     [step.student.out_grad_view(i).cpu().clone() for i in range(c['s'][1])],
                     student.device_state().A.tensor('param').cpu().clone(), student.device_state().A.tensor('grad').cpu().clone()))
    a, b = runs
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and float(a[3].abs().max()) > 0


def test_twenty_steps_on_one_batch_lower_the_kd_loss():
    c, student, teacher, step = _tiny_step((None, 0.5), lr=2.5e-4)
    step.set_batch(*_cases.batch('tiny', 0))
    kd = []
    for i in range(20):
        step.step()
        if i in (0, 19):
            kd.append(step.losses()[1])
    assert np.isfinite(kd).all() and 0 < kd[1] < kd[0], kd


def test_fused_step_refuses_kl_with_ohkm_and_a_non_positive_temperature():
    from fpd_amd import runtime as R
    for kw in ({'kl': (None, 1.0), 'ohkm': (8, None)}, {'kl': (None, 0.0)}, {'kl': (-0.5, None)}):
        with pytest.raises(R.FpdError):
            _tiny_step(kw.pop('kl'), **kw)


# ---- entry points -----------------------------------------------------------------------------------------------------------
def test_fpd_train_and_train_run_with_the_kl_criterion(caplog):
    import logging
    import re
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsKLDLoss, JointsMSELoss
    from fpd_amd.lib.utils.utils import FusedAdam
    from tests.test_entry_gpu import _Loader, _cfgnode, _models
    shape = _cases.batch('tiny', 0)[0].shape
    c, gold, student, teacher = _models('tiny')
    opt = FusedAdam(student, lr=2.5e-4)
    before = student.device_state().A.tensor('param').clone()
    mse, kl = JointsMSELoss(True).cuda(), JointsKLDLoss(True, 0.5).cuda()
    with caplog.at_level(logging.INFO, logger=F.logger.name):
        loss = F.fpd_train(_cfgnode(print_freq=1), _Loader('tiny', 2), student, teacher, mse, kl, opt, 0, '/tmp', '/tmp', None)
    logged = [float(v) for v in re.findall(r'KD_POSE_Loss ([0-9.eE+-]+|nan|inf) ', caplog.text)]
    assert len(logged) == 2 and np.isfinite(logged).all() and all(v > 0 for v in logged), caplog.text
    step = F.fused_step_for(student, teacher, opt, shape, 0.5, 1, (True, True), None, (None, 0.5))
    assert step.kl == (None, 0.5) and int(opt.step_dev) == 2
    assert np.isfinite(loss) and 0 < loss < 10
    assert not torch.equal(before, student.device_state().A.tensor('param'))
    assert F.fused_step_for(student, teacher, opt, shape, 0.5, 1, (True, True)) is not step      # the MSE step is another plan
    assert F.fused_step_for(student, teacher, opt, shape, 0.5, 1, (True, True), None, (None, 0.25)) is not step
    # plain training: one KL criterion for both terms (alpha 0)
    c, gold, student, teacher = _models('tiny')
    opt = FusedAdam(student, lr=2.5e-4)
    before = student.device_state().A.tensor('param').clone()
    loss = F.train(_cfgnode(alpha=0.0), _Loader('tiny', 1), student, JointsKLDLoss(True, 1.0).cuda(), opt, 0, '/tmp', '/tmp', None)
    step = F.fused_step_for(student, None, opt, shape, 0.0, 1, (True, True), None, (1.0, 1.0))
    assert abs(loss - step.losses()[0]) < 1e-12 and 0 < loss < 10
    assert not torch.equal(before, student.device_state().A.tensor('param'))
