"""JointsOHKMMSELoss on the MI355X (csrc/loss_ohkm.hip): fpd_loss_ohkm and core.loss.JointsOHKMMSELoss against the reference's own
class (tests/golden/ohkm_small.npz) and against the float64 restatement tests/_ohkm_ref.py -- bit for bit on dyadic inputs --,
the tie rule, FusedFPDStep(ohkm=...) and the core.function entry points.

Tolerances are those tests/test_kernels_gpu.py::test_loss applies to fpd_loss, whose per-element arithmetic is the same:
losses 1e-6 * max(1, |ref|); gradients 1e-9 (fp32) or 1e-2 * max|ref| (bf16, one rounding of the result), + 1e-6 * max|ref|."""
import os

import numpy as np
import pytest
import torch

from tests import _cases, _ohkm_ref
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, 'tests', 'golden', 'ohkm_small.npz')
GAP = 1e-3


def _tdt(dtype):
    return torch.bfloat16 if dtype == 1 else torch.float32


def _nchw64(t):
    """NHWC tensor (any float dtype) -> float64 numpy NCHW"""
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous().numpy()


def run_ohkm(outs, teacher, target, w, topk, alpha, dtype, w_kd=None, nchw=1, dout=True, grad_scale=1.0, offset=0):
    """One fpd_loss_ohkm call.  outs / teacher: NHWC CPU tensors already in the storage type; target: NCHW float32 CPU tensor;
    w / w_kd: [B,J] float32.  offset: every map and gradient starts that many elements behind a 16-byte boundary, between guard
    elements that have to stay intact.
    -> dict(losses [2] float64, douts: NCHW float64 numpy, masks uint32 [S,2,B], rows float64 [S,2,B,J])."""
    from fpd_amd import runtime as R
    dev = torch.device('cuda:0')
    B, H, W, J = outs[0].shape
    S = len(outs)
    k = R.LossOhkmT()
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
    k.topk_pose, k.topk_kd = topk
    nbytes = R.lib().fpd_loss_ohkm_scratch_bytes(a)
    assert nbytes > 0 and nbytes % (B * S * 2 * J * 8) == 0
    scratch = torch.full((nbytes // 8,), float('nan'), dtype=torch.float64, device=dev)      # every slab must be written
    masks = torch.full((S, 2, B), -1, dtype=torch.int32, device=dev)
    k.scratch, k.scratch_bytes, k.masks = scratch.data_ptr(), nbytes, masks.data_ptr()
    R.check(R.lib().fpd_loss_ohkm(k, R.current_stream()), 'fpd_loss_ohkm')
    torch.cuda.synchronize()
    assert all(x.intact() for x in guarded)
    rows = scratch.view(B, -1, S, 2, J).cpu().numpy()
    return {'losses': losses.cpu().numpy(), 'douts': [_nchw64(d) for d in d_douts],
            'masks': masks.cpu().numpy().view(np.uint32), 'rows': rows.sum(1).transpose(1, 2, 0, 3), 'chunks': rows.shape[1]}


def reference(outs, teacher, target, w, topk, alpha, w_kd=None, grad_scale=1.0):
    wp = w.double().numpy()
    wk = w_kd.double().numpy() if w_kd is not None else wp
    return _ohkm_ref.fused([_nchw64(o) for o in outs], target.double().numpy(), _nchw64(teacher), wp, wk, topk[0], topk[1], alpha,
                           grad_scale)


def assert_close(got, ref, dtype, grads=True):
    """test_kernels_gpu.py::test_loss's tolerances (module docstring)"""
    assert np.array_equal(got['masks'], ref['masks']), (got['masks'], ref['masks'])
    for v, r in ((got['losses'][0], ref['pose']), (got['losses'][1], ref['kd'])):
        assert abs(v - r) < 1e-6 * max(1.0, abs(r)), (got['losses'], ref['pose'], ref['kd'])
    assert np.abs(got['rows'] - ref['rows']).max() <= 1e-6 * np.abs(ref['rows']).max()      # fp32 products, short fp32 sums, fp64 beyond
    if grads:
        for g, r in zip(got['douts'], ref['grads']):
            m = np.abs(r).max()
            tol = 1e-9 if dtype == 0 else 1e-2 * m
            assert np.abs(g - r).max() <= tol + 1e-6 * m, (np.abs(g - r).max(), m)


def _gap_ok(ref, topk):
    """the k-th and (k+1)-th largest per-joint sum of every (stack, term, sample) differ by >= GAP relative: a condition on the
    INPUTS (evaluated in float64 on the CPU) that makes the selection unambiguous in fp32 and bf16"""
    for term, k in enumerate(topk):
        r = -np.sort(-ref['rows'][:, term], -1)
        if k < r.shape[-1] and not (np.all(r[..., k - 1] - r[..., k] >= GAP * r[..., k - 1]) and np.all(r[..., k - 1] > 0)):
            return False
    return True


def make_inputs(seed, B, J, H, W, S, dtype, topk, alpha, kd_weights=False):
    """seeded random inputs (already rounded to the storage type) + their reference; the seed moves on until _gap_ok"""
    while True:
        gen = torch.Generator().manual_seed(seed)
        scale = 0.2 + 0.8 * torch.rand(1, 1, 1, J, generator=gen)              # joints of different difficulty
        outs = [(torch.randn(B, H, W, J, generator=gen) * scale).to(_tdt(dtype)) for _ in range(S)]
        teacher = (torch.randn(B, H, W, J, generator=gen) * scale).to(_tdt(dtype))
        target = torch.rand(B, J, H, W, generator=gen)
        w = (torch.rand(B, J, generator=gen) * 1.5) * (torch.rand(B, J, generator=gen) < 0.8)
        w_kd = (0.5 + torch.rand(B, J, generator=gen)) if kd_weights else None
        ref = reference(outs, teacher, target, w, topk, alpha, w_kd)
        if _gap_ok(ref, topk):
            return outs, teacher, target, w, w_kd, ref
        seed += 1000


# ---- golden: the reference's own class -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,use_w,k', [('j16', 1, 8), ('j16', 0, 8), ('j17', 1, 1), ('j17', 1, 17), ('j17', 0, 1), ('j17', 0, 17)])
def test_golden_kernel_and_class_match_the_reference_class(name, use_w, k):
    from fpd_amd.lib.core.loss import JointsOHKMMSELoss
    g = np.load(GOLD)
    out, tg, wt = (torch.from_numpy(g[name + '/' + n]) for n in ('output', 'target', 'weight'))
    key = '%s/w%d/k%d' % (name, use_w, k)
    gl, gg = float(g[key + '/loss']), g[key + '/grad']
    B, J = out.shape[:2]
    w = wt[:, :, 0] if use_w else torch.ones(B, J)
    sel = _ohkm_ref.criterion(out.numpy(), tg.numpy(), w.numpy(), k)['sel']      # == the reference's (tests/test_ohkm_cpu.py)
    want = _ohkm_ref.mask_words(sel)
    assert ((gg != 0).any((2, 3)) <= sel).all()
    m = np.abs(gg).max()
    # the C entry point: S = 1, alpha = 0, teacher = the output (what the class passes)
    o = out.permute(0, 2, 3, 1).contiguous()
    got = run_ohkm([o], o, tg, w, (k, J), 0.0, 0)
    assert np.array_equal(got['masks'][0, 0], want) and (got['masks'][0, 1] == (1 << J) - 1).all()
    assert abs(got['losses'][0] - gl) < 1e-6 * max(1.0, abs(gl)) and got['losses'][1] == 0.0
    assert np.abs(got['douts'][0] - gg).max() <= 1e-9 + 1e-6 * m
    # the stand-alone class
    crit = JointsOHKMMSELoss(bool(use_w), topk=k).cuda()
    od = out.cuda().requires_grad_(True)
    loss = crit(od, tg.cuda(), wt.cuda())
    assert loss.dim() == 0
    (2.0 * loss).backward()
    torch.cuda.synchronize()
    assert np.array_equal(crit.last_mask.cpu().numpy().view(np.uint32), want)
    assert abs(loss.item() - gl) < 1e-6 * max(1.0, abs(gl))
    assert np.abs(od.grad.cpu().double().numpy() - 2.0 * gg).max() <= 2.0 * (1e-9 + 1e-6 * m)


def test_class_refuses_a_topk_outside_1_to_J():
    from fpd_amd import runtime as R
    from fpd_amd.lib.core.loss import JointsOHKMMSELoss
    o = torch.zeros(1, 4, 4, 4, device='cuda')
    for k in (0, 5):
        with pytest.raises(R.FpdError):
            JointsOHKMMSELoss(True, topk=k)(o, o, torch.ones(1, 4, 1, device='cuda'))


# ---- bit-exact on dyadic inputs ------------------------------------------------------------------------------------------------
def _dyadic(S, seed=5, B=2, J=16, H=8, W=8):
    """maps / targets: multiples of 2^-4 in [-2, 2]; weights in {0, 0.5, 1}: every product and sum below is exact in fp32, and with
    alpha = 0.5 and B*k*HW a power of two so are the loss and the gradient (which then fits bf16's 8 bits or is rounded once)"""
    gen = torch.Generator().manual_seed(seed)
    q = lambda *shape: torch.randint(-32, 33, shape, generator=gen).float() / 16.0
    outs = [q(B, H, W, J) for _ in range(S)]
    teacher, target = q(B, H, W, J), q(B, J, H, W)
    w = torch.randint(0, 3, (B, J), generator=gen).float() / 2.0
    return outs, teacher, target, w


@pytest.mark.parametrize('dtype', [0, 1])
@pytest.mark.parametrize('S,misaligned', [(1, False), (2, False), (2, True)], ids=['1', '2', 'misaligned'])
def test_dyadic_inputs_are_bit_exact(S, misaligned, dtype):
    if misaligned:
        # J a multiple of the vector but every map and gradient one element off the 16-byte grid: the scalar kernels with
        # 16 joint lanes per pixel, on a ragged 108-pixel tile.  B k HW is no power of two here, so the gradient is rounded:
        # what is expected is what the aligned run (the vector kernels) gives on the same inputs, bit for bit.
        outs, teacher, target, w = _dyadic(2, B=2, J=16, H=12, W=9)
        outs, teacher = [o.to(_tdt(dtype)) for o in outs], teacher.to(_tdt(dtype))
        want = run_ohkm(outs, teacher, target, w, (8, 8), 0.5, dtype)
        got = run_ohkm(outs, teacher, target, w, (8, 8), 0.5, dtype, offset=1)
        ref = reference(outs, teacher, target, w, (8, 8), 0.5)
        assert np.array_equal(got['rows'], ref['rows']) and np.array_equal(got['masks'], ref['masks'])      # (sums of dyadic products: exact)
        assert np.array_equal(got['rows'], want['rows']) and np.array_equal(got['masks'], want['masks'])
        assert np.array_equal(got['losses'], want['losses'])
        for g, r in zip(got['douts'], want['douts']):
            assert not np.isnan(r).any() and np.array_equal(g, r)
        return
    outs, teacher, target, w = _dyadic(S)
    outs, teacher = [o.to(_tdt(dtype)) for o in outs], teacher.to(_tdt(dtype))       # exact: 6 significant bits
    ref = reference(outs, teacher, target, w, (8, 8), 0.5)
    got = run_ohkm(outs, teacher, target, w, (8, 8), 0.5, dtype)
    assert np.array_equal(got['rows'], ref['rows'])
    assert np.array_equal(got['masks'], ref['masks'])
    assert got['losses'][0] == ref['pose'] and got['losses'][1] == ref['kd']
    for g, r in zip(got['douts'], ref['grads']):
        want = torch.from_numpy(r).to(_tdt(dtype)).double().numpy()                  # the fp64 result rounded once
        assert np.array_equal(g, want)
        if dtype == 0:
            assert np.array_equal(g, r)


@pytest.mark.parametrize('dtype', [0, 1])
def test_topk_J_equals_fpd_loss_bitwise_on_dyadic_inputs(dtype):
    from fpd_amd import runtime as R
    outs, teacher, target, w = _dyadic(2, seed=6)
    outs, teacher = [o.to(_tdt(dtype)) for o in outs], teacher.to(_tdt(dtype))
    J = 16
    got = run_ohkm(outs, teacher, target, w, (J, J), 0.5, dtype)
    assert (got['masks'] == (1 << J) - 1).all()
    dev = torch.device('cuda:0')
    a = R.LossT()
    B, H, W, _ = outs[0].shape
    a.B, a.J, a.H, a.W, a.S, a.dtype, a.target_nchw, a.alpha, a.grad_scale = B, J, H, W, 2, dtype, 1, 0.5, 1.0
    d_outs = [o.to(dev) for o in outs]
    d_douts = [torch.zeros_like(o) for o in d_outs]
    for i in range(2):
        a.out[i], a.dout[i] = d_outs[i].data_ptr(), d_douts[i].data_ptr()
    d_t, d_tg, d_w = teacher.to(dev), target.to(dev), w.to(dev)
    losses = torch.zeros(2, dtype=torch.float64, device=dev)
    a.teacher, a.target, a.weight, a.losses = d_t.data_ptr(), d_tg.data_ptr(), d_w.data_ptr(), losses.data_ptr()
    R.check(R.lib().fpd_loss(a, R.current_stream()), 'fpd_loss')
    torch.cuda.synchronize()
    assert np.array_equal(losses.cpu().numpy(), got['losses'])
    for d, g in zip(d_douts, got['douts']):
        assert np.array_equal(_nchw64(d), g)


# ---- shapes where it can go wrong --------------------------------------------------------------------------------------------
SHAPES = {   # B, J, H, W, S, topk, kwargs
    'J17_scalar_path': (2, 17, 8, 8, 2, (5, 5), {}),
    'HW108_partial_tile': (2, 16, 12, 9, 1, (8, 8), {}),
    'HW156_partial_last_tile': (2, 16, 13, 12, 2, (8, 8), {}),
    'B3_eight_chunks': (3, 16, 32, 32, 2, (8, 4), {'grad_scale': 0.25}),      # (grad_scale: 1 / world_size)
    'two_tiles_per_block': (5, 16, 128, 128, 1, (8, 8), {}),                 # B * tiles > 512 blocks: a block walks two tiles
    'pose_ohkm_kd_mse': (2, 16, 8, 8, 2, (8, 16), {}),
    'pose_mse_kd_ohkm': (2, 16, 8, 8, 2, (16, 5), {}),
    'weight_kd': (2, 16, 8, 8, 2, (8, 8), {'kd_weights': True}),
    'forward_only': (2, 16, 12, 9, 2, (8, 8), {'dout': False}),
    'target_nhwc': (2, 16, 12, 9, 2, (8, 8), {'nchw': 0}),
    'target_nhwc_J17': (2, 17, 12, 9, 1, (3, 17), {'nchw': 0}),
    'J32_S8': (1, 32, 8, 8, 8, (8, 31), {}),
    'S3_below_its_register_variant': (2, 16, 12, 9, 3, (8, 5), {}),          # three stacks in the four-stack instantiation
    'S4_benchmark_stacks': (2, 16, 16, 16, 4, (8, 8), {}),
    'S3_J17': (2, 17, 8, 8, 3, (5, 17), {}),
    'S4_J17': (1, 17, 12, 9, 4, (17, 4), {}),
}


@pytest.mark.parametrize('dtype', [0, 1])
@pytest.mark.parametrize('case', sorted(SHAPES))
def test_shapes_match_the_reference(case, dtype):
    B, J, H, W, S, topk, kw = SHAPES[case]
    alpha, gs = 0.3, kw.get('grad_scale', 1.0)
    outs, teacher, target, w, w_kd, ref = make_inputs(17 + B + J + H + S, B, J, H, W, S, dtype, topk, alpha, kw.get('kd_weights', False))
    ref['grads'] = [gs * g for g in ref['grads']]
    got = run_ohkm(outs, teacher, target, w, topk, alpha, dtype, w_kd=w_kd, nchw=kw.get('nchw', 1), dout=kw.get('dout', True),
                   grad_scale=gs)
    assert got['chunks'] == {'B3_eight_chunks': 8, 'two_tiles_per_block': 64}.get(case, -(-H * W // 128))
    assert_close(got, ref, dtype, grads=kw.get('dout', True))
    if not kw.get('dout', True):
        assert all(np.isnan(d).all() for d in got['douts'])                 # forward only: nothing written


# ---- the tie rule and fewer than k weighted joints ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [0, 1])
def test_equal_joints_at_the_k_boundary_keep_the_lower_index(dtype):
    B, J, H, W, k = 2, 16, 8, 8, 8
    gen = torch.Generator().manual_seed(3)
    base = torch.randint(1, 9, (B, H, W), generator=gen).float() / 8.0
    amp = torch.tensor([4.0, 0.25, 3.0, 0.5, 2.5, 1.0, 0.125, 3.5, 0.375, 2.0, 0.625, 1.0, 1.5, 0.75, 1.75, 0.0625])
    assert (amp > 1.0).sum() == k - 1 and amp[5] == amp[11] == 1.0           # joints 5 and 11 are equal and rank k, k + 1
    out = (base[..., None] * amp).to(_tdt(dtype))
    zero = torch.zeros(B, J, H, W)
    got = run_ohkm([out], out, zero, torch.ones(B, J), (k, J), 0.0, dtype)
    ref = reference([out], out, zero, torch.ones(B, J), (k, J), 0.0)
    assert (ref['rows'][0, 0, :, 5] == ref['rows'][0, 0, :, 11]).all()
    assert np.array_equal(got['rows'], ref['rows']) and np.array_equal(got['masks'], ref['masks'])
    nz = (got['douts'][0] != 0).any((2, 3))
    assert (nz.sum(1) == k).all() and nz[:, 5].all() and not nz[:, 11].any()
    assert (got['masks'][0, 0] >> 5 & 1).all() and not (got['masks'][0, 0] >> 11 & 1).any()


@pytest.mark.parametrize('dtype', [0, 1])
def test_fewer_than_k_weighted_joints(dtype):
    B, J, H, W, k = 2, 16, 8, 8, 8
    outs, teacher, target, w, _, _ = make_inputs(41, B, J, H, W, 1, dtype, (J, J), 0.0)
    w = torch.zeros(B, J)
    w[0, [1, 4, 9, 12, 15]] = torch.tensor([1.0, 0.5, 1.5, 0.75, 1.25])
    w[1, [0, 2]] = torch.tensor([0.5, 1.0])
    ref = reference(outs, teacher, target, w, (k, k), 0.0)
    got = run_ohkm(outs, teacher, target, w, (k, k), 0.0, dtype)
    assert_close(got, ref, dtype)
    pop = np.array([[bin(int(m)).count('1') for m in row] for row in got['masks'][0]])
    assert (pop == k).all()                                                  # zero-weight joints fill the mask (lowest indices first) ...
    assert (got['douts'][0][w.numpy() == 0] == 0).all()                      # ... and carry no gradient
    assert (np.abs(got['douts'][0][w.numpy() != 0]).max((1, 2)) > 0).all()


def test_a_nan_joint_ranks_first_and_the_mask_keeps_k_bits():
    """Diverged maps: a NaN per-joint sum counts as the largest value (torch.topk's order), so the mask still has k bits."""
    B, J, H, W, k = 2, 16, 8, 8, 8
    outs, teacher, target, w, _, _ = make_inputs(43, B, J, H, W, 1, 0, (J, J), 0.0)
    w = torch.ones(B, J)
    outs[0][0, 3, 2, 9] = float('nan')
    outs[0][1, :, :, 14] = float('nan')
    got = run_ohkm(outs, teacher, target, w, (k, k), 0.5, 0)
    pop = np.array([[bin(int(m)).count('1') for m in row] for row in got['masks'][0]])
    assert (pop == k).all(), got['masks']
    assert (got['masks'][0, :, 0] >> 9 & 1).all() and (got['masks'][0, :, 1] >> 14 & 1).all()


# ---- the fused step ---------------------------------------------------------------------------------------------------------
def _tiny_step(ohkm, **kw):
    from fpd_amd import executor as E
    from tests.test_model_gpu import build_models
    c, gold, student, teacher = build_models('tiny')
    step = E.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, c['batch'],
                          c['image'][1], c['image'][0], alpha=0.5, ohkm=ohkm, **kw)
    return c, student, teacher, step


def test_fused_step_with_ohkm_matches_the_reference_on_its_own_maps():
    from fpd_amd import runtime as R
    c, student, teacher, step = _tiny_step((8, None))
    assert step.ohkm == (8, 16)
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
    ref = reference(outs, tmap, tg, tw[:, :, 0], (8, 16), 0.5)
    assert _gap_ok(ref, (8, 16))                                             # (a property of these maps: the selection is unambiguous)
    assert np.array_equal(step.ohkm_masks().numpy().view(np.uint32), ref['masks'])
    assert abs(pose - ref['pose']) < 1e-5 * max(1, abs(ref['pose'])) and abs(kd - ref['kd']) < 1e-5 * max(1, abs(ref['kd']))
    for i in range(S):
        g, r = _nchw64(s.out_grad_view(i)), ref['grads'][i]
        assert np.abs(g - r).max() <= 1e-9 + 1e-6 * np.abs(r).max()
    # the plan: same size as the JointsMSELoss step's, the loss op exchanged
    _, _, _, plain = _tiny_step(None)
    types = lambda st: [st.student.plan.op_type(i) for i in range(len(st.student.plan))]
    assert len(step.student.plan) == len(plain.student.plan) and step.launches_per_step() == plain.launches_per_step()
    assert types(plain).count(R.OP_LOSS) == 2 and R.OP_LOSS_OHKM not in types(plain) and 'ohkm_scratch' not in plain.student.A.t
    assert types(step).count(R.OP_LOSS_OHKM) == 2 and R.OP_LOSS not in types(step)
    assert [t for t in types(step) if t != R.OP_LOSS_OHKM] == [t for t in types(plain) if t != R.OP_LOSS]


def test_fused_step_with_ohkm_is_bit_repeatable():
    runs = []
    for _ in range(2):
        c, student, teacher, step = _tiny_step((8, 4), lr=2.5e-4)
        step.set_batch(*_cases.batch('tiny', 0))
        step.step()
        torch.cuda.synchronize()
        runs.append((step.student.A.tensor('losses')[:2].cpu().clone(), step.ohkm_masks().clone(),
                     [step.student.out_grad_view(i).cpu().clone() for i in range(c['s'][1])],
                     student.device_state().A.tensor('param').cpu().clone(), student.device_state().A.tensor('grad').cpu().clone()))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and float(a[4].abs().max()) > 0


def test_fused_step_refuses_a_topk_outside_1_to_J():
    from fpd_amd import runtime as R
    with pytest.raises(R.FpdError):
        _tiny_step((17, None))


# ---- entry points -----------------------------------------------------------------------------------------------------------
def test_fpd_train_and_train_run_with_the_ohkm_criterion():
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss, JointsOHKMMSELoss
    from fpd_amd.lib.utils.utils import FusedAdam
    from tests.test_entry_gpu import _Loader, _cfgnode, _models
    shape = _cases.batch('tiny', 0)[0].shape
    popcount = lambda m: [bin(int(v) & 0xffffffff).count('1') for v in m.reshape(-1)]
    # distillation: OHKM pose criterion, MSE distillation criterion
    c, gold, student, teacher = _models('tiny')
    opt = FusedAdam(student, lr=2.5e-4)
    before = student.device_state().A.tensor('param').clone()
    hard, mse = JointsOHKMMSELoss(True, 8).cuda(), JointsMSELoss(True).cuda()
    loss = F.fpd_train(_cfgnode(), _Loader('tiny', 1), student, teacher, hard, mse, opt, 0, '/tmp', '/tmp', None)
    step = F.fused_step_for(student, teacher, opt, shape, 0.5, 1, (True, True), (8, None))
    assert step.ohkm == (8, 16) and int(opt.step_dev) == 1
    assert abs(loss - step.losses()[2]) < 1e-12 and 0 < loss < 10
    m = step.ohkm_masks().numpy()
    assert set(popcount(m[:, 0])) == {8} and set(popcount(m[:, 1])) == {16}
    assert not torch.equal(before, student.device_state().A.tensor('param'))
    assert F.fused_step_for(student, teacher, opt, shape, 0.5, 1, (True, True)) is not step      # the MSE step is another plan
    # plain training: one OHKM criterion for both terms (alpha 0)
    c, gold, student, teacher = _models('tiny')
    opt = FusedAdam(student, lr=2.5e-4)
    before = student.device_state().A.tensor('param').clone()
    loss = F.train(_cfgnode(alpha=0.0), _Loader('tiny', 1), student, JointsOHKMMSELoss(True, 8).cuda(), opt, 0, '/tmp', '/tmp', None)
    step = F.fused_step_for(student, None, opt, shape, 0.0, 1, (True, True), (8, 8))
    assert abs(loss - step.losses()[0]) < 1e-12 and 0 < loss < 10
    assert set(popcount(step.ohkm_masks().numpy())) == {8}
    assert not torch.equal(before, student.device_state().A.tensor('param'))
