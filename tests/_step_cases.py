"""Inputs, case lists and references of the tests of the step-boundary kernels (csrc/loss_adam.hip): fpd_loss, fpd_adam,
fpd_weight_prep, fpd_bn_update_running, fpd_cast and the two layout changes.  tests/test_step_kernels_gpu.py runs them on the
device, tests/test_step_cases_cpu.py asserts the preconditions on the references alone.  No device is needed to import or use
this module; the Adam reference is tests/_adam_ref.py.

fpd_loss, exact inputs: maps, teacher and target in {-1, -0.5, 0, 0.5, 1}, weights in {0, 0.5, 1}, alpha in {0, 0.25, 1},
grad_scale in {1, 0.25}.  Then E = (1-alpha) w^2 (p-g) + alpha w_kd^2 (p-t) is exact in float32 however it is grouped or
contracted, the gradient RN32(RN32(grad_scale / float32(cnt)) * E) has ONE reproducible rounding (two in bf16: the same two
the kernel makes), and every per-thread float32 sum of w^2 d^2 is exact (a multiple of 2^-6 far below 2^24: loss_headroom()).
With cnt a power of two the loss itself is exact; otherwise the kernel's documented rounding of every block's term to a
multiple of 2^-44 and the roundings of 0.5 / cnt and of the product remain: loss_bound().  The sign of a zero gradient is left
open (comparisons are by value: -0 == +0).

Every case carries the launch geometry it is there for -- (vectorised, blocks, tiles_per_block, last block of an image short)
per dtype -- as a literal claim; the CPU test holds fpd_loss_geometry() against it."""
import functools
from fractions import Fraction

import numpy as np
import torch

F32, BF16 = 0, 1
DTYPES = (F32, BF16)
RS = 4                 # FPD_STATS_REPLICAS
GUARD = 64             # guard elements on each side of every destination
SENTINEL = -12345.0
BN_MOMENTUM = 0.1


def tdt(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


def gen_for(*parts):
    """A generator seeded by the case (ints and short strings, possibly in tuples)."""
    s = 0
    for p in parts:
        for v in (p if isinstance(p, tuple) else (p,)):
            s = (s * 31 + (sum(map(ord, v)) if isinstance(v, str) else int(v))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(5000 + s)


def pick(gen, values, shape):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), tuple(shape), generator=gen)]


# ---------------------------------------------------------------------------------------------------------------------
# fpd_loss
# variants: (target_nchw, weight_kd given, dout NULL for: None / 'one' stack (the middle or last of several) / 'all', alpha, grad_scale)
V_A = (1, False, None, 0.25, 1.0)
V_B = (0, True, None, 0.25, 0.25)
V_C = (1, True, 'one', 1.0, 0.25)
V_D = (0, False, 'all', 0.25, 1.0)
V_E = (1, False, None, 0.0, 1.0)
# (B, J, H, W, S), {dtype: (vectorised, blocks, tiles_per_block, last block of an image owns fewer tiles)}, variants
LOSS_CASES = [
    ((16, 16, 64, 64, 2), {F32: (1, 256, 2, False), BF16: (1, 256, 2, False)}, (V_A, V_C)),     # 32 tiles per image, cnt = 2^20: exact losses
    ((33, 16, 40, 40, 1), {F32: (1, 231, 2, True), BF16: (1, 231, 2, True)}, (V_B, V_D)),       # 13 tiles: the 7th block owns one, ragged (64 pixels)
    ((40, 8, 24, 56, 3), {F32: (1, 240, 2, True), BF16: (1, 240, 2, True)}, (V_C,)),            # 11 tiles; one / two vectors per pixel
    ((2, 24, 16, 16, 2), {F32: (1, 4, 1, False), BF16: (1, 4, 1, False)}, (V_B,)),              # six / three vectors per pixel
    ((2, 32, 16, 8, 8), {F32: (1, 2, 1, False), BF16: (1, 2, 1, False)}, (V_E, V_C)),           # J = 32, S = 8, HW = one tile exactly
    ((300, 16, 8, 8, 1), {F32: (1, 300, 1, False), BF16: (1, 300, 1, False)}, (V_B,)),          # > 256 images, half-filled tiles
    ((2, 17, 64, 48, 1), {F32: (0, 96, 1, False), BF16: (0, 96, 1, False)}, (V_A, V_D)),        # scalar kernel, 48 tiles per image
    ((3, 17, 12, 9, 2), {F32: (0, 6, 1, False), BF16: (0, 6, 1, False)}, (V_B, V_C)),           # ... a ragged second tile (44 pixels)
    ((5, 1, 9, 7, 1), {F32: (0, 5, 1, False), BF16: (0, 5, 1, False)}, (V_E,)),                 # J = 1
    ((2, 20, 10, 13, 2), {F32: (1, 4, 1, False), BF16: (0, 6, 1, False)}, (V_B,)),              # vector kernel in fp32 only; 2 pixels in the last tile
    ((2, 4, 16, 16, 2), {F32: (1, 4, 1, False), BF16: (0, 8, 1, False)}, (V_C,)),
]
LOSS_RUNS = [(c, dt, v) for c, _, vs in LOSS_CASES for v in vs for dt in DTYPES]
LOSS_CLAIMS = {(c, dt): g[dt] for c, g, _ in LOSS_CASES for dt in DTYPES}
POW2_CASE = LOSS_CASES[0][0]
GENERAL_CASES = [(33, 16, 40, 40, 1), (2, 17, 64, 48, 1)]


def loss_struct(R, case, dtype, variant, ptrs=None):
    """The fpd_loss_t of a run.  ptrs: dict(out=[...], dout=[... or None], teacher, target, weight, weight_kd, losses) of device
    addresses; None: placeholders (16-byte aligned, never dereferenced) with the variant's NULLs, for the geometry query."""
    B, J, H, W, S = case
    nchw, _, null, alpha, gs = variant
    a = R.LossT()
    a.B, a.J, a.H, a.W, a.S, a.dtype, a.target_nchw, a.alpha, a.grad_scale = B, J, H, W, S, dtype, nchw, alpha, gs
    if ptrs is None:
        ptrs = dict(out=[4096] * S, dout=[None if skipped(null, s, S) else 4096 for s in range(S)], teacher=4096, target=4096,
                    weight=4096, weight_kd=4096 if variant[1] else None, losses=4096)
    for s in range(S):
        a.out[s], a.dout[s] = ptrs['out'][s], ptrs['dout'][s]
    a.teacher, a.target, a.weight, a.weight_kd, a.losses = ptrs['teacher'], ptrs['target'], ptrs['weight'], ptrs['weight_kd'], ptrs['losses']
    return a


def skipped(null, s, S):
    """Whether stack s has dout[s] == NULL under the variant's `null`."""
    return null == 'all' or (null == 'one' and s == (S - 1 if S < 3 else 1))


def loss_geometry(R, a):
    import ctypes as C
    v, b, t = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    R.check(R.lib().fpd_loss_geometry(C.byref(a), C.byref(v), C.byref(b), C.byref(t)), 'fpd_loss_geometry')
    return v.value, b.value, t.value


def expected_geometry(case, dtype, aligned=True):
    """The rule of csrc/loss_adam.hip restated: (vectorised, blocks, tiles_per_block, short last block, pixels of the last tile)."""
    B, J, H, W, S = case
    hw = H * W
    if aligned and J % (8 if dtype == BF16 else 4) == 0:
        tpi = -(-hw // 128)
        tpb = 1
        while B * -(-tpi // tpb) > 256 and tpb < tpi:
            tpb += 1
        return 1, B * -(-tpi // tpb), tpb, tpi % tpb != 0, hw - (tpi - 1) * 128
    return 0, B * -(-hw // 64), 1, False, hw - (-(-hw // 64) - 1) * 64


@functools.lru_cache(maxsize=4)
def loss_inputs(case, wkd):
    """outs [S] / teacher NHWC, target NCHW, w / w_kd [B,J]: float32 CPU tensors of exact values (identical in both storage types)."""
    B, J, H, W, S = case
    gen = gen_for('loss', case, int(wkd))
    vals = [-1.0, -0.5, 0.0, 0.5, 1.0]
    outs = [pick(gen, vals, (B, H, W, J)) for _ in range(S)]
    teacher, target = pick(gen, vals, (B, H, W, J)), pick(gen, vals, (B, J, H, W))
    w = pick(gen, [0.0, 0.5, 1.0], (B, J))
    w.view(-1)[0], w.view(-1)[-1] = 0.0, 0.5                        # zeros are present whatever the draw
    wk = None
    if wkd:
        wk = pick(gen, [0.0, 0.5, 1.0, 1.0], (B, J))
        wk.view(-1)[0], wk.view(-1)[-1] = 1.0, 0.0                  # ... and not where w has them
    return dict(outs=outs, teacher=teacher, target=target, w=w, wk=wk)


@functools.lru_cache(maxsize=4)
def loss_reference(case, variant):
    """-> dict(losses [2] float64 numpy, E [S] float64 (exact), grads {dtype: [S] tensors in the storage type}, w2 / w2k [B,1,1,J],
    sums: (pose, kd) per image [B] float64 = sum over stacks, pixels, joints of w^2 d^2)."""
    B, J, H, W, S = case
    nchw, wkd, null, alpha, gs = variant
    i = loss_inputs(case, wkd)
    cnt = B * J * H * W
    g, t = i['target'].permute(0, 2, 3, 1).double(), i['teacher'].double()
    w2 = (i['w'].double() ** 2)[:, None, None, :]
    w2k = w2 if i['wk'] is None else (i['wk'].double() ** 2)[:, None, None, :]
    pose_img, kd_img = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    E = []
    for o in i['outs']:
        dg, dt = o.double() - g, o.double() - t
        pose_img += (w2 * dg * dg).sum((1, 2, 3))
        kd_img += (w2k * dt * dt).sum((1, 2, 3))
        E.append((1.0 - alpha) * w2 * dg + alpha * w2k * dt)
    losses = np.array([0.5 * float(pose_img.sum()) / cnt, 0.5 * float(kd_img.sum()) / cnt])
    scale = torch.tensor(gs, dtype=torch.float32) / torch.tensor(float(cnt), dtype=torch.float32)      # RN32(grad_scale / float32(cnt))
    g32 = [scale * e.float() for e in E]                                                                # RN32(scale * E)
    return dict(losses=losses, E=E, grads={F32: g32, BF16: [x.bfloat16() for x in g32]}, w2=w2, w2k=w2k, sums=(pose_img, kd_img), cnt=cnt)


def loss_headroom(ref):
    """The exact-sum precondition: sum |addend| of a whole image, in units of 2^-6, below 2^24 (a thread's share is part of it),
    every addend a multiple of that unit, E exact in float32 and bf16-rounding-free inputs."""
    for s in ref['sums']:
        units = s * 64.0
        assert torch.equal(units, torch.round(units)), 'an addend is no multiple of 2^-6'
        assert float(units.max()) < 2.0 ** 24, 'per-image sum of %.0f units of 2^-6 is not below 2^24' % float(units.max())
    for e in ref['E']:
        assert torch.equal(e.float().double(), e), 'E is not exact in float32'


def loss_bound(ref_value, blocks, cnt):
    """0 when cnt is a power of two (every step exact), else blocks * 2^-45 + 4 ulp(ref)."""
    if cnt & (cnt - 1) == 0:
        return 0.0
    return blocks * 2.0 ** -45 + 4.0 * float(np.spacing(abs(ref_value)))


def general_loss_inputs(case, dtype):
    """The random construction of tests/test_kernels_gpu.py test_loss and its fp64 specification."""
    B, J, H, W, S = case
    gen = torch.Generator().manual_seed(13 + sum(case))
    rnd = lambda *s: torch.randn(*s, generator=gen)
    outs = [rnd(B, H, W, J).to(tdt(dtype)) for _ in range(S)]
    teacher = rnd(B, H, W, J).to(tdt(dtype))
    target = torch.rand(B, J, H, W, generator=gen)
    wgt = (torch.rand(B, J, generator=gen) * 1.5) * (torch.rand(B, J, generator=gen) < 0.8)
    alpha = 0.3
    g = target.permute(0, 2, 3, 1).double()
    w2 = (wgt.float().double() ** 2)[:, None, None, :]
    cnt = B * J * H * W
    pose = sum(0.5 * (w2 * (o.double() - g) ** 2).sum() / cnt for o in outs)
    kd = sum(0.5 * (w2 * (o.double() - teacher.double()) ** 2).sum() / cnt for o in outs)
    grads = [w2 * ((1 - alpha) * (o.double() - g) + alpha * (o.double() - teacher.double())) / cnt for o in outs]
    return dict(outs=outs, teacher=teacher, target=target, w=wgt.float(), alpha=alpha, pose=float(pose), kd=float(kd), grads=grads)


# ---------------------------------------------------------------------------------------------------------------------
# fpd_weight_prep: tables of (K, R, S, C, outputs), outputs in 'both' / 'fwd' / 'bwd'
_MODES = ('both', 'fwd', 'bwd')
WPREP_TABLES = {
    # 576 tiles against the 64-block cap; ragged in both directions; a non-square filter
    'main': [(k, r, s, c, _MODES[i % 3]) for i, (k, r, s, c) in enumerate(
        [(256, 3, 3, 256), (17, 1, 1, 16), (16, 1, 1, 128), (48, 3, 3, 96), (33, 3, 3, 31), (64, 3, 3, 3), (8, 1, 3, 40)])],
    # the largest entry has 272 elements: a grid of ONE block walks every tile of every entry
    'one_block': [(17, 1, 1, 16, 'both'), (8, 1, 3, 5, 'bwd'), (3, 3, 3, 7, 'both'), (16, 1, 1, 16, 'fwd')],
    'single': [(33, 3, 3, 31, 'both')],
}
TIES = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]      # halfway between two bf16 values: to the even one, i.e. down / up


def special_values():
    v = [s * t * sc for t in TIES for s in (1.0, -1.0) for sc in (1.0, 2.0 ** 20, 2.0 ** -20)]
    return torch.tensor(v + [0.0, -0.0], dtype=torch.float32)


def wprep_master(K, R, S, C, seed):
    """randn with the bf16 ties and +-0 planted on a quarter of the positions (at least one full set)."""
    gen = torch.Generator().manual_seed(7000 + seed)
    n = K * R * S * C
    w = torch.randn(n, generator=gen)
    sp = special_values()
    idx = torch.randperm(n, generator=gen)[:max(n // 4, len(sp))]
    w[idx] = sp[torch.arange(len(idx)) % len(sp)]
    return w.view(K, R, S, C)


def wprep_reference(w, dtype):
    """(w_fwd [K][R][S][C], w_bwd [C][R][S][K]) in the storage type: the interpreter's run_wprep."""
    return w.to(tdt(dtype)), w.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(tdt(dtype))


def bits(t):
    """Bit patterns of a float32 / bfloat16 tensor."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------------------------------
# fpd_bn_update_running
BNUPD_TABLES = {     # (C, count, num_batches_tracked given)
    'dyadic': [(16, 1, True), (48, 2, True), (257, 64, False), (384, 8192, True)],
    'general': [(16, 1, True), (48, 2, False), (257, 50, True), (384, 8192, True)],
}


def limbs(v):
    """[..] float64 -> (hi, lo) int64: executor.Arenas.stats_write / csrc/common.h stat_split."""
    hi = torch.round(v * 2.0 ** 20)
    lo = torch.round((v - hi / 2.0 ** 20) * 2.0 ** 60)
    return hi.to(torch.int64), lo.to(torch.int64)


def joined_sums(st):
    """[R][2][C] float64 replica values -> [2][C]: limbs summed over the replicas as integers, then joined (csrc/common.h stats_sum)."""
    hi, lo = limbs(st)
    return hi.sum(0).double() * (1.0 / 2.0 ** 20) + lo.sum(0).double() * (1.0 / 2.0 ** 60)


def _split(gen, total, dyadic):
    """[C] totals -> [R][C] replica shares of mixed signs that add up to them exactly."""
    C = total.numel()
    if dyadic:      # multiples of 1/16: the last share is exact
        sh = torch.randint(-2 ** 12, 2 ** 12, (RS - 1, C), generator=gen).double() / 16.0
    else:           # of the size of the total: the last share's rounding stays at 2^-52 of it
        sh = total[None] * (2.0 * torch.rand(RS - 1, C, generator=gen, dtype=torch.float64) - 1.0)
    return torch.cat([sh, (total - sh.sum(0))[None]], 0)


def bnupd_inputs(kind, k, C, count):
    """-> dict(stats [R][2][C] float64, rmean / rvar [C] float32, flat: constant-tensor channels, neg: channels built to have a
    negative raw variance)."""
    gen = torch.Generator().manual_seed(8000 + 10 * k + (0 if kind == 'dyadic' else 1))
    flat = torch.zeros(C, dtype=torch.bool)
    neg = torch.zeros(C, dtype=torch.bool)
    flat[::5] = True
    if kind == 'dyadic':
        mean = torch.randint(-1024, 1025, (C,), generator=gen).double() / 16.0       # |mean| <= 64
        mean[0], mean[5] = 64.0, -64.0
        var = torch.randint(1, 65, (C,), generator=gen).double() / 16.0
        var[flat] = 0.0
        s1, s2 = count * mean, count * (var + mean * mean)
        rmean = torch.randint(-128, 129, (C,), generator=gen).float() / 16.0
        rvar = torch.randint(1, 129, (C,), generator=gen).float() / 16.0
    else:
        mean = torch.randn(C, generator=gen, dtype=torch.float64) * 10.0 ** (3 * torch.rand(C, generator=gen, dtype=torch.float64) - 1.5)
        var = torch.rand(C, generator=gen, dtype=torch.float64) + 0.05
        var[flat] = 0.0
        s1, s2 = count * mean, count * (var + mean * mean)
        neg[5::10] = True                                                            # (constant-tensor channels, all of them)
        s2[neg] = s2[neg] * (1.0 - 2.0 ** -40)                                       # ... whose second sum came out a little low
        rmean = torch.randn(C, generator=gen)
        rvar = torch.rand(C, generator=gen) + 0.5
        rvar[neg] = 0.0      # the clamp gives 0.9 * 0 = 0 exactly; unclamped, -0.1 * 2^-40 mean^2 is 2^13 times the bound
    st = torch.stack([_split(gen, s1, kind == 'dyadic'), _split(gen, s2, kind == 'dyadic')], 1)      # [R][2][C]
    return dict(stats=st, rmean=rmean, rvar=rvar, flat=flat, neg=neg, count=count)


def bnupd_reference(i, fused=False):
    """-> (running_mean, running_var [C] float64 before the rounding to float32, raw variance [C]).  fused: the raw variance as
    ONE rounding of s2/count - mean*mean (a contracted multiply-add) instead of two."""
    s = joined_sums(i['stats'])
    count = float(i['count'])
    mom = float(np.float32(BN_MOMENTUM))
    mean = s[0] / count
    q = s[1] / count
    if fused:
        raw = torch.tensor([float(Fraction(float(a)) - Fraction(float(b)) ** 2) for a, b in zip(q, mean)], dtype=torch.float64)
    else:
        raw = q - mean * mean
    var = raw.clamp_min(0.0)
    unb = var * count / (count - 1.0) if count > 1 else var
    return (1.0 - mom) * i['rmean'].double() + mom * mean, (1.0 - mom) * i['rvar'].double() + mom * unb, raw


def bnupd_bound(i, ref64):
    """(bound on running_mean, on running_var): one float ulp of the reference, and for the variance 2^-52 mean^2 momentum on top."""
    mean = joined_sums(i['stats'])[0] / float(i['count'])
    ulp = lambda x: torch.from_numpy(np.spacing(np.abs(x.float().numpy()))).double()
    return ulp(ref64[0]), 2.0 ** -52 * mean * mean * BN_MOMENTUM + ulp(ref64[1])


# ---------------------------------------------------------------------------------------------------------------------
# fpd_cast and the layout changes
LOOP_N = 4096 * 256 + 4099           # more elements than the capped grid has threads: the loop iterates
LAYOUT_SHAPES = [(3, 3, 8, 8), (1, 32, 7, 9), (2, 17, 6, 5), (9, 16, 128, 128)]      # (N, C, H, W); the last iterates the loop


def cast_source_f32(n=LOOP_N):
    gen = torch.Generator().manual_seed(9000)
    x = torch.randn(n, generator=gen) * 10.0 ** (6 * torch.rand(n, generator=gen) - 3)
    sp = torch.cat([special_values(), torch.tensor([float('inf'), float('-inf'), float('nan'), 2.0 ** -130, -2.0 ** -140, 3.0e38])])
    idx = torch.randperm(n, generator=gen)[:n // 8]
    x[idx] = sp[torch.arange(len(idx)) % len(sp)]
    return x


def cast_source_bf16(n=LOOP_N):
    """Random bf16 bit patterns (denormals and infinities included) with every NaN pattern replaced by a finite value."""
    gen = torch.Generator().manual_seed(9001)
    b = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=gen).to(torch.int16)
    x = b.view(torch.bfloat16)
    return torch.where(torch.isnan(x), torch.full_like(x, 1.5), x)
