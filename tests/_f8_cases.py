"""Inputs, case list and reference-side checks of the bit-exact tests of the fp8 forward convolution (csrc/conv_tile_f8.hip;
tests/test_exact_f8_gpu.py on the device, tests/test_f8_cases_cpu.py for the preconditions and for the instantiations the list
reaches).  The sibling of tests/_exact_inputs.py for ops that carry w8; no device is needed to import or use this module.

Why kernel and specification (oracle/fp8_ref.py through oracle/plan_interp.py) must agree in EVERY BIT here: products of two
e4m3 values are exact in fp32, so with weights that quantise exactly under power-of-two scales and operands that are small
dyadic numbers the fp32 accumulator is exact in any grouping; scale (a power of two), bias and residual keep it exact, and the
result is rounded to bf16 once.

  weights     fp32 masters  w[k] = u * 2^(6 - e_k),  u an integer in -7..7 and e_k in {6, 7, 8} drawn per output channel: exactly
              one element of a row has |u| = 7, so amax / 448 == 2^-e_k exactly and the e4m3 value of every element is 64 u (448,
              +-64 .. +-384: all on the e4m3 grid).  The scale differs from channel to channel, so a scale read at the wrong
              column shows.  'sparse': that element and one more of +-1 .. +-6 per output channel; 'dense': every tap live, +-1.
              (The row maximum is 7 quanta of its row whatever the scale, so an operand under it weighs 49 times its square in
              the statistics: that, not the accumulator, is what bounds everything below.  e_k in {9, 10} -- a 7 / 8 or 7 / 16
              row maximum -- would put a residual of 1 at 64 or 128 quanta of the output: no room for its square.)
  operands    small() ({-1, -0.5, 0, 0.5, 1} with zeros mixed in) and, on 2 % of the elements ('dense': 1.25 %), a value that the
              e4m3 rounding CHANGES: an odd multiple 17 .. 31 of the operand's quantum qx, or twice that -- every one of them lies
              exactly between two e4m3 neighbours, half of them round down to the even neighbour and half up (qx = 1/2: 8.5 -> 8,
              9.5 -> 10, 17 -> 16, 19 -> 20).  Behind a BatchNorm prologue the element of x is chosen so that relu(bn(x)) IS that
              value.  Cases marked `big` also carry operands beyond +-448 (+-512), on the input channels hot().  The plain
              draw alone has only e4m3-representable operands and could not tell this kernel from the bf16 one.
  prologue    exact_bn() in train mode (statistics as an input, invstd == 1.0f; its coarse draw: operands on a grid of 1/2),
              exact_eval_bn() in eval mode (operands on a grid of 1/8), or none.

Statistics headroom decides how much of this a (case, weight mode) pair can carry: the sprinkled values are 17 quanta and more,
their squares add up over the pixels.  'dense' filters and maps of more than 4096 pixels use the two smallest values (17 and 19
quanta) alone, maps of more than 2048 pixels 17 .. 31; a pair that still cannot keep sum v*v below 2^24 quanta runs without
out_stats (NO_STATS below says which and why; check_f8() asserts that every other pair keeps the headroom)."""
import torch
import torch.nn.functional as F

from fpd_amd import graph as G
from oracle import fp8_ref, plan_interp as PI
from tests import _exact_inputs as X
from tests.test_exact_gpu import small

RS = X.RS
WMODES = X.WMODES

# (N, H, W, C, K, R, prologue, residual, bias, big).  The comment names the instantiation TN x BK the library reports
# (fpd_conv_f8_variant; tests/test_f8_cases_cpu.py asserts it) and what the shape is there for; no tensor has more than 8192 pixels.
F8_EXACT = [
    (2, 16, 16, 64, 64, 3, 'train', True, True, False),       # TN1 BK64
    (2, 32, 24, 32, 32, 3, 'eval', False, True, False),       # TN1 BK32; W = 24: tiles of 5 rows = 120 pixels
    (1, 64, 48, 32, 64, 1, None, False, True, False),         # TN1 BK32, 1x1; W = 48: tiles of 96 pixels
    (2, 8, 6, 256, 256, 3, None, True, True, True),           # TN1 BK64; W = 6: tiles of 21 rows spanning both images; four chunks
    (3, 12, 16, 128, 8, 1, 'eval', False, False, False),      # TN1 BK64, 1x1; K = 8, the narrowest output of the vector epilogue
    (2, 64, 64, 64, 128, 1, 'train', True, True, False),      # TN2 BK64, 1x1
    (1, 96, 72, 32, 32, 3, 'train', True, True, False),       # TN1 BK32; W = 72: one row per tile
    (1, 33, 48, 32, 32, 3, None, False, True, True),          # TN1 BK32; 33 rows in tiles of 2: the last tile ends inside the tensor
    (1, 16, 128, 32, 512, 1, 'train', False, True, False),    # TN2 BK32, 1x1
    (1, 16, 128, 32, 512, 3, None, True, False, False),       # TN2 BK32
    (1, 32, 64, 64, 512, 3, 'train', False, True, False),     # TN2 BK64
    (1, 32, 128, 32, 488, 1, None, True, False, False),       # TN4 BK32, 1x1; ragged K: 488 = 3 * 128 + 104
    (1, 43, 128, 32, 264, 3, 'train', False, True, False),    # TN4 BK32; the last channel tile is 8 wide
    (1, 64, 64, 64, 504, 3, None, True, True, False),         # TN4 BK64; ragged K
    (1, 32, 128, 64, 512, 1, 'train', False, True, False),    # TN4 BK64, 1x1
]
# (case, weight mode) pairs that run WITHOUT out_stats: sum v*v over the map leaves its headroom (dense filters behind the free
# eval-mode draw, whose operands sit on a grid of 1/8; operands of 448 under dense filters, each of which meets the row maximum
# of some output channel: 7 * 896 quanta, squared, is beyond 2^24 by itself; 288 dense taps over 6912 pixels).  Every case
# compares the statistics in its other mode.  (The free eval-mode draw reaches operands of 4 = 32 quanta: under the row maximum
# they are 224 quanta each, which 'sparse' filters carry up to some 1500 pixels -- the eval-mode cases are the small ones.)
NO_STATS = {(c, 'dense') for c in F8_EXACT if c[6] == 'eval' or c[9] or c[:6] == (1, 96, 72, 32, 32, 3)}
VARIANTS = {tn | bk << 4 for tn in (1, 2, 4) for bk in (32, 64)}      # what csrc/conv_tile_f8.hip is compiled for
assert all(c[0] * c[1] * c[2] <= 8192 for c in F8_EXACT)


def variant_name(v):
    return 'declined' if v < 0 else 'TN%d BK%d' % (v & 15, v >> 4)


def route(N, H, W, C, K, R, stride=1):
    """csrc/conv_tile_f8.hip f8_route() restated for a stride-`stride` 'same' convolution in bf16 with the plain epilogue
    -> TN | BK << 4, or -1 outside the domain."""
    rows = max(1, 128 // max(W, 1))
    bk = 64 if C % 64 == 0 else 32
    if stride != 1 or R not in (1, 3) or W > 128 or W < 2 or C % 32 or C > 512 or K % 8 or (rows + R - 1) * W * (bk // 8) > 2048:
        return -1
    mt = -(-N * H // rows)
    tn = 4 if K > 64 else (2 if K > 32 else 1)
    while tn > 1 and mt * -(-K // (32 * tn)) < 128:
        tn >>= 1
    return tn | bk << 4


def conv_struct(R, N, H, W, C, K, r, stride=1):
    """The launch as the library's host queries see it (never dereferenced)."""
    a = R.ConvT()
    a.x = a.w = a.y = 64
    a.dtype, a.epi = R.BF16, R.EPI_PLAIN
    P, Q = (H - 1) // stride + 1, (W - 1) // stride + 1
    a.N, a.H, a.W, a.C, a.K, a.R, a.S, a.stride, a.pad, a.P, a.Q = N, H, W, C, K, r, r, stride, (r - 1) // 2, P, Q
    return a


def hot(C):
    """The input channels that carry the operands beyond 448 of a `big` case."""
    return torch.arange(C) % 8 == 5


def f8_weights(gen, mode, K, R, C, big=False):
    """fp32 master weights [K, R, R, C] as the module docstring states them.  big, 'sparse': the row maximum stays off the hot()
    channels and the second tap is +-1 there (an operand of 448 is 896 quanta: times 7, squared, it alone would leave the
    statistics headroom) -- under 'dense' filters, which run without statistics, every weight meets them."""
    u = torch.zeros(K, R * R, C)
    rows = torch.arange(K)
    sign = lambda *shape: torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    if mode == 'dense':
        u = sign(K, R * R, C)
    else:
        tap2, c2 = torch.randint(0, R * R, (K,), generator=gen), torch.randint(0, C, (K,), generator=gen)
        v2 = torch.randint(1, 7, (K,), generator=gen).float()
        if big:
            v2 = torch.where(hot(C)[c2], torch.ones(K), v2)
        u[rows, tap2, c2] = v2 * sign(K)
    tap, c = torch.randint(0, R * R, (K,), generator=gen), torch.randint(0, C, (K,), generator=gen)
    if mode == 'sparse':
        c = torch.where((tap == tap2) & (c == c2), (c + 1) % C, c)            # (never on the second tap)
        if big:
            c = torch.where(hot(C)[c], (c + 2) % C, c)                        # (c % 8 == 7: not hot; the second tap's neighbour is c2 + 1)
            c = torch.where((tap == tap2) & (c == c2), (c + 1) % C, c)
    u[rows, tap, c] = 7.0 * sign(K)
    e = torch.randint(6, 9, (K,), generator=gen)
    return (u.view(K, -1) * torch.pow(2.0, 6.0 - e.float()).view(K, 1)).view(K, R, R, C)


ODD = [17.0, 19.0, 21.0, 23.0, 25.0, 27.0, 29.0, 31.0]


def f8_operand(gen, shape, density, qx, targets, rate, big, coef=None, unit=False):
    """x [N, H, W, C]: the plain draw (unit: {-1, 0, 1}) at `density` with, on `rate` of the elements, a value whose operand
    relu(gamma x + shift) (coef = (gamma, shift) per channel; None: x itself, either sign) is qx times a member of `targets`; big:
    three elements in a thousand of the hot() channels becomes an operand beyond 448."""
    x = small(gen, *shape, density=density)
    if unit:
        x = torch.randint(-1, 2, shape, generator=gen).float() * (x != 0)
    t = qx * X.pick(gen, targets, x.numel()).float().view(shape)
    if coef is None:
        t = t * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
        huge = 512.0 * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
    else:
        t = (t - coef[1].float()) / coef[0].float()
        huge = torch.full(shape, 1024.0)
    x = torch.where(torch.rand(shape, generator=gen) < rate, t, x)
    if big:
        x = torch.where((torch.rand(shape, generator=gen) < 3e-3) & hot(shape[-1]), huge, x)
    assert torch.equal(x.bfloat16().float(), x), 'an element of x is not bf16-representable'
    return x


def f8_forward(bt, case, wmode):
    """The op of tests/test_fp8_gpu.py test_conv_forward_f8 on exact inputs -> X.Built; b.h: 'op', 'op16' (the same convolution
    without w8: the bf16 specification on the same buffers), 'wm' / 'w' / 'w8' / 'w8s' (master, bf16, e4m3 weights and scales)."""
    N, H, W, C, K, R, mode, use_res, use_bias, big = case
    gen = X.seed('f8', case[:6], str(mode), use_res, use_bias, big, wmode)
    b = X.Built()
    n, pad = N * H * W, (R - 1) // 2
    dense = wmode == 'dense'
    terms = C * R * R if dense else 2
    wv = f8_weights(gen, wmode, K, R, C, big)
    # train mode: the coarse draw of exact_bn() (operands on a grid of 1/2; every channel free under sparse filters up to 2048
    # pixels, one in four up to 4096, one in ten beyond and behind dense filters, the others quiet); the free eval-mode draw leaves operands on
    # a grid of 1/8
    coarse = mode == 'train'
    bn = coef = None
    if mode == 'train':
        bn = b.bn(bt, gen, C, n, live=0.1 if dense or n > 4096 else (1.0 if n <= 2048 else 0.25))
        coef = (b.bns[bn]['gamma'], b.bns[bn]['shift'])
    elif mode == 'eval':
        bn, ex, _ = X.exact_eval_bn(bt, gen, C, 'bn')
        bn.count = n
        b.bns[bn] = ex
        coef = (ex['gamma'], ex['shift'])
    qx = 0.5 if (mode is None or coarse) else 0.125
    targets = ODD[:2] if dense else (ODD[:2] if n > 4096 else ODD if n > 2048 or mode == 'eval' else ODD + [2 * v for v in ODD])
    density = 0.6 if mode else min(0.6, 64.0 / terms)
    xv = f8_operand(gen, (N, H, W, C), density, qx, targets, 0.0125 if dense else 0.02, big, coef, unit=coarse)
    x = bt.act((N, H, W, C), xv, 'x')
    wm = bt.buf('param', (K, R, R, C), wv)
    w = bt.buf('wlp', (K, R, R, C), wv)
    w8, w8s = bt.buf('w8', (K, R, R, C)), bt.buf('w8s', (K,))
    bias = bt.buf('param', (K,), small(gen, K)) if use_bias else None
    res = bt.act((N, H, W, K), small(gen, N, H, W, K), 'res') if use_res else None
    y = bt.act((N, H, W, K), None, 'y')
    stats = (case, wmode) not in NO_STATS
    ostats = bt.buf('stats', (RS, 2, K), torch.zeros(RS, 2, K, dtype=torch.float64)) if stats else None
    kw = dict(x=x, w=w, wkey='w', bias=bias, bkey='b' if use_bias else None, residual=res, y=y, bn=bn, epi='plain', epi_x=None,
              epi_bn=None, epi_stats=None, dims=(N, H, W, C, K, R, R, 1, pad, H, W))
    op = G.Op('conv', out_stats=ostats, w8=w8, w8s=w8s, w_master=wm, **kw)
    b.ops.append(op)
    b.compare += [('y', y)] + ([('out_stats', ostats)] if stats else [])
    b.h.update(op=op, op16=G.Op('conv', out_stats=None, **kw), wm=wm, w=w, w8=w8, w8s=w8s)
    return b


# ---------------------------------------------------------------------------------------------------------------------
# the exhaustive operand sweep: every bf16 bit pattern through the quantiser, once per position of an 8-byte LDS vector
SWEEP = [(1, 32, 64, 32), (1, 16, 64, 64)]        # (N, H, W, C = K): BK32, BK64 -- 65536 elements each
SWEEP_PROLOGUES = [None, 'identity', 'identity+relu']


def sweep_bits():
    """Element i holds the bit pattern i * 0x9E37 mod 2^16 (an odd multiplier: every pattern once).  NOT in order: eight
    consecutive patterns differ in the three mantissa bits the rounding drops first, and e.g. bytes 4, 5 and 6, 7 of a packed
    vector could change places without any of them changing its e4m3 value; here neighbours differ in sign and exponent."""
    return (torch.arange(65536, dtype=torch.int64) * 0x9E37) % 65536


def sweep_patterns():
    """The 65536 bf16 bit patterns (order: sweep_bits()), NaN (254 patterns) replaced by 0 -- a NaN operand is outside the
    specification."""
    v = sweep_bits().to(torch.int16).view(torch.bfloat16).float()
    return torch.where(torch.isnan(v), torch.zeros_like(v), v)


def f8_sweep(bt, shape, prologue):
    """y[.., k] = e4m3(prologue(x[.., k])) * 7/16 through a 1x1 convolution with the master weights 7/16 * I (e4m3 byte 448 at
    scale 2^-10): exact in bf16 for every one of the 253 values of the e4m3 grid.  -> X.Built (h as f8_forward())"""
    N, H, W, C = shape
    b = X.Built()
    x = bt.act(shape, sweep_patterns().view(shape), 'x')
    wv = (0.4375 * torch.eye(C)).view(C, 1, 1, C)
    wm, w = bt.buf('param', (C, 1, 1, C), wv), bt.buf('wlp', (C, 1, 1, C), wv)
    w8, w8s = bt.buf('w8', (C, 1, 1, C)), bt.buf('w8s', (C,))
    y = bt.act(shape, None, 'y')
    bn = None
    if prologue:
        bn = G.BN('bn', 'eval', C, bt.buf('param', (C,), torch.ones(C)), bt.buf('param', (C,), torch.zeros(C)),
                  bt.buf('rstat', (C,), torch.zeros(C)), bt.buf('rstat', (C,), torch.full((C,), 1.0 - 1e-5)), bt.buf('nbt', ()),
                  relu=prologue.endswith('relu'))
        bn.count = N * H * W
    op = G.Op('conv', x=x, w=w, wkey='w', bias=None, bkey=None, residual=None, y=y, out_stats=None, bn=bn, epi='plain', epi_x=None,
              epi_bn=None, epi_stats=None, dims=(N, H, W, C, C, 1, 1, 1, 0, H, W), w8=w8, w8s=w8s, w_master=wm)
    b.ops.append(op)
    b.compare.append(('y', y))
    b.h.update(op=op, wm=wm, w=w, w8=w8, w8s=w8s)
    return b


# ---------------------------------------------------------------------------------------------------------------------
# the checks on the reference
def operand(A, op):
    """-> (the prologue result in fp32, not yet rounded; its e4m3 rounding) as the specification forms them."""
    x = PI._act(A, op.x)
    if op.bn is not None:
        scale, shift, _, _ = PI._bn_coef(A, op.bn)
        x = torch.addcmul(shift, x, scale)
        if op.bn.relu:
            x = x.clamp_min(0)
    return x, fp8_ref.quant_e4m3(x)


def ties(x, xq):
    """-> (elements that lie exactly between two e4m3 neighbours and went to the one nearer zero, ... away from zero)."""
    other = 2.0 * x.double() - xq.double()                # the neighbour on the far side, if x is a midpoint
    mid = (x != xq) & (x.abs() < fp8_ref.E4M3_MAX) & (fp8_ref.quant_e4m3(other.float()).double() == other) & (other != xq.double())
    return int((mid & (xq.abs() < x.abs())).sum()), int((mid & (xq.abs() > x.abs())).sum())


def _channel_quantum(t):
    """t [..., K] -> [K]: per channel the smallest power of two every element is a multiple of."""
    return torch.tensor([X.quantum(t[..., k]) for k in range(t.shape[-1])], dtype=torch.float64)


def check_f8(A, b, label=''):
    """The preconditions of a bit-exact comparison of an fp8 convolution, on the arenas the interpreter has run b.ops over; and
    the conditions that make the comparison worth having.  -> dict of the measured shares (for the callers' own assertions).
    Headroom is counted per OUTPUT CHANNEL in that channel's own quantum: the scales differ by channel, every sum the kernel
    forms (accumulator column, statistics) belongs to one channel."""
    op = b.h['op']
    n, h, w, C, K, R, S, stride, pad, P, Q = op.dims
    for ex in b.bns.values():
        assert not bool(((ex['shift'] == 0) & (ex['mu'] != 0)).any()), label + ': beta - mu*gamma cancels'
    if op.bn is not None and op.bn in b.bns:
        X._check_bn(A, op.bn, b.bns[op.bn], PI._act(A, op.x), label + ' prologue')
        if op.bn.mode == 'eval':                          # the device's arithmetic: eps = (double)(float)1e-5
            inv = 1.0 / torch.sqrt(A.view(op.bn.rvar).double() + X.EPS_DEVICE)
            g, ex = A.view(op.bn.gamma).double(), b.bns[op.bn]
            assert torch.equal((g * inv).float().double(), ex['gamma']), label + ': device scale not exact'
            assert torch.equal((A.view(op.bn.beta).double() - A.view(op.bn.rmean).double() * g * inv).float().double(), ex['shift']), label + ': device shift not exact'
    # weights: exact quantisation under power-of-two scales
    wm = A.view(b.h['wm']).float()
    q, scale = fp8_ref.quant_weights(wm)
    assert bool((torch.frexp(scale).mantissa == 0.5).all()), label + ': a weight scale is not a power of two'
    assert torch.equal(q * scale.view(-1, 1, 1, 1), wm), label + ': the weight quantisation is not exact'
    assert torch.equal(A.view(b.h['w']).float(), wm), label + ': the masters are not bf16-representable'
    assert bool((q.reshape(K, -1).abs().amax(1) == 448).all()) and int((q.abs() == 448).sum()) == K
    # accumulator: e4m3 operand x e4m3 weight integers, exact in any grouping; then scale, bias, residual
    x, xq = operand(A, op)
    acc = F.conv2d(X._nchw(xq.abs()).double(), X._nchw(q.abs()).double(), None, stride=stride, padding=pad).permute(0, 2, 3, 1)
    qa = X.quantum(xq) * X.quantum(q)
    X._headroom(acc, qa, label + ' accumulator')
    extra = [A.view(op.bias).double()] if op.bias is not None else []
    extra += [PI._act(A, op.residual).double()] if op.residual is not None else []
    unit = torch.minimum(qa * scale.double(), torch.tensor(min([1.0] + [X.quantum(e) for e in extra]), dtype=torch.float64))
    X._headroom((acc * scale.double() + 2.0) / unit, 1.0, label + ' scaled accumulator + bias + residual')
    y = PI._act(A, op.y).double()
    assert float(y.abs().max()) > 0, label + ': all-zero output'
    if op.out_stats is not None:
        qy = _channel_quantum(y)
        X._headroom(y.abs().sum((0, 1, 2)) / qy, 1.0, label + ' sum v')
        X._headroom((y * y).sum((0, 1, 2)) / (qy * qy), 1.0, label + ' sum v*v')
        st = A.view(op.out_stats).sum(0)
        assert float(st[0].abs().max()) > 0 and float(st[1].abs().max()) > 0, label + ': all-zero statistics'
    down, up = ties(x, xq)
    return dict(changed=float((x != xq).float().mean()), down=down, up=up, big=int((x.abs() > fp8_ref.E4M3_MAX).sum()))


def bf16_output(bt, b):
    """y of the same convolution WITHOUT w8 (the bf16 specification) on the arenas of `bt`; the fp8 result is put back."""
    yb = b.h['op'].y.buf
    keep = bt.cpu.view(yb).clone()
    PI.run(bt.cpu, [b.h['op16']])
    y16 = bt.cpu.view(yb).float().clone()
    bt.cpu.view(yb).copy_(keep)
    return y16
