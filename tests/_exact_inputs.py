"""Input constructions, op lists and case lists of the bit-exact tests of the streaming kernels, of the stem, of the halo-tile
kernels, of the wgrad3 weight gradient and of the stride-2 convolutions (tests/test_exact_stream_gpu.py, tests/test_exact_stem_gpu.py,
tests/test_exact_tile_gpu.py, tests/test_exact_wgrad3_gpu.py on the device; tests/test_exact_inputs_cpu.py for the preconditions,
tests/test_exact_variants_cpu.py for the kernel instantiations the halo-tile lists reach, tests/test_exact_wgrad3_cpu.py for the
launch geometries the wgrad3 list reaches).  No device is needed to import or use this module.

Everything here is a small dyadic rational, chosen so that the specification (oracle/plan_interp.py) is EXACT: a kernel that
groups its partial sums differently, folds its coefficients in another order or rounds an fp32 accumulator to bf16 once must
still give the same bits.

  activations / gradients   small(): {-1, -0.5, 0, 0.5, 1} with zeros mixed in
  weights                   'sparse': two non-zeros per output channel (fp32 and bf16 storage agree bit for bit);
                            'dense': every weight in {+-0.5, +-1} (every MFMA fragment position live; the accumulator is an
                            exact multiple of 1/4 or finer, far below 2^24, and is rounded to bf16 ONCE: deterministic)
  train-mode BatchNorm      exact_bn(): the statistics buffer is an input, s1 = count*mu, s2 = count*(1 - 1e-5 + mu*mu), so that
                            invstd rounds to 1.0f, scale == gamma, shift == beta - mu*gamma, mean == mu -- per channel
  BN-backward apply         exact_apply_stats(): st[0] = count*m1, st[1] = count*m2: du = gamma*(g - m1 - (u - mu)*m2) is a
                            multiple of 1/16 with few significant bits whatever the order of evaluation

Two cancellations are avoided by construction (device and interpreter form these coefficients in fp64 with an invstd that is
1 + O(1e-13) before it is rounded to 1.0f, so an exact zero would come out as a residue of unspecified sign and size ~1e-14):
shift = beta - mu*gamma is never zero unless mu is, and mu*m2 - m1 is never zero unless both terms are.

Where the table of per-channel coefficients is varied and where it is not: forward prologues behind DENSE filters and on
maps of more than 2048 pixels use the coarse draw of exact_bn() (budget() says why), and on the largest of them -- the 3x3
conv_c3 / conv_pp cases at 4096 pixels -- budget() leaves no freely drawn channel: every channel there has gamma in {0.5, 1}
and shift in {0, -1/2}.  A mis-indexed table is therefore caught by the 'sparse' mode of those shapes (all channels free),
by the smaller shapes (all ten (C, K) of conv_c1 at 512 pixels: 78-100 % of the channels free) and by every backward epilogue / folded apply (always the
free draw), not by the large dense forward cases, which are there for the tiles, strips, halos and statistics.

check_reference() asserts, ON THE INTERPRETER'S RESULT, the headroom that makes every fp32 sum exact in any grouping (sum of
|addend| in units of the common power of two below 2^24, per channel / element over the whole tensor), that no output is
degenerate, that every ReLU mask keeps 10-90 % and that more than 1 % of every normalised tensor sits exactly ON the mask
boundary (x*scale + shift == 0: `>` against `>=` is visible).

The stem (Conv2d(3, K, 7, stride 2, pad 3) on the fp32 NCHW image; tests/test_exact_stem_gpu.py): image, weights, bias and dy are
drawn from the same sets, so EVERY value is bf16-representable -- on purpose.  In a bf16 build the direct kernels (csrc/stem.hip)
multiply the unrounded fp32 image and weights, while the space-to-depth and im2col kernels (csrc/stem_s2d.hip,
csrc/stem_mfma.hip) and the interpreter round both to bf16 first; on these inputs the rounding changes nothing and all three
back ends share ONE specification.  (That difference is not touched here.)  The frozen stem's bn1 + ReLU ('act') is an
eval-mode BN with running_var = 1 - 1e-5 -- invstd == 1.0f, scale == gamma, shift == beta - mean*gamma, the cancellation rule
of exact_bn() -- and one channel in 16 has all-zero weights, zero bias and zero shift: every pixel of it sits ON the ReLU
boundary.  The s2d forward keeps its statistics per lane in fp32, SHIFTED by the channel's bias: check_reference() asserts the
headroom of those sums (|y - bias|, (y - bias)^2) beside the plain ones."""
import numpy as np
import torch
import torch.nn.functional as F

from fpd_amd import graph as G
from oracle import plan_interp as PI
from tests.test_exact_gpu import small, sparse_weights
from tests import test_conv_c1_gpu as _c1, test_conv_c3_gpu as _c3, test_kernels_gpu as _tk

RS = _tk.RS
WMODES = ['sparse', 'dense']
LIMIT = float(2 ** 24)
EPS_DEVICE = float(torch.tensor(1e-5, dtype=torch.float32))      # the device adds (double)(float)1e-5


class CpuBench:
    """tests.test_kernels_gpu.Bench without the device: the same bump allocator, arenas of the interpreter only."""

    def __init__(self, dtype):
        self.dtype, self.sizes, self.fills = dtype, {}, []

    def buf(self, arena, shape, fill=None):
        n = int(np.prod(shape)) if len(shape) else 1
        off = self.sizes.get(arena, 0)
        self.sizes[arena] = off + (n + 63) // 64 * 64
        b = G.Buf(arena, off, shape, arena)
        if fill is not None:
            self.fills.append((b, fill))
        return b

    def act(self, shape, fill=None, name='t'):
        a = G.Act(shape, name)
        a.buf = self.buf('act', shape, fill)
        return a

    def realise(self):
        self.cpu = PI.Arenas(self.sizes, torch.bfloat16 if self.dtype == 1 else torch.float32)
        for b, val in self.fills:
            v = self.cpu.view(b)
            v.copy_(val.reshape(v.shape).to(v.dtype))
        return self

    def run(self, ops):
        PI.run(self.cpu, ops)


# ---------------------------------------------------------------------------------------------------------------------
# constructions
def pick(gen, values, n):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), (n,), generator=gen)]


def weights(gen, mode, K, R, C):
    if mode == 'sparse':
        return sparse_weights(gen, K, R, C)
    sign = torch.randint(0, 2, (K, R, R, C), generator=gen).float() * 2 - 1
    return sign * torch.where(torch.rand(K, R, R, C, generator=gen) < 0.5, 0.5, 1.0)


MU = [0.0, 0.25, -0.25, 0.5, -0.5]
GAMMA = [0.5, 1.0, 2.0]
BETA = [0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0]


def exact_bn(bt, gen, C, count, name='bn', live=None):
    """-> (graph.BN in train mode with ReLU, dict of the exact per-channel fp64 values mu / gamma / beta / shift).
    live None: mu, gamma, beta drawn freely from MU, GAMMA, BETA (shift: multiples of 1/8).  One channel in 16 has mu = beta = 0.
    live in [0, 1] -- the COARSE draw for operands of large or dense convolutions, whose second statistics sum would leave its
    headroom otherwise: beta and mu*gamma are multiples of 1/2 (still members of the sets), so that with inputs in {-1, 0, 1}
    the normalised operand is a multiple of 1/2; the share `live` of the channels is otherwise free, the others are QUIET:
    gamma in {0.5, 1} and shift in {0, -1/2}, i.e. relu(bn(x)) in {0, 1/2, 1} and non-zero only where x == 1."""
    mu, gamma, beta = pick(gen, MU, C), pick(gen, GAMMA, C), pick(gen, BETA, C)
    if live is not None:
        mu = torch.where(gamma == 0.5, torch.zeros_like(mu), torch.where(gamma == 1.0, torch.round(mu * 2) / 2, mu))
        beta = torch.round(beta * 2) / 2                  # (+-0.25 -> 0)
        quiet = torch.rand(C, generator=gen) >= live
        qg = pick(gen, [0.5, 1.0], C)
        qs = pick(gen, [0.0, 0.0, -0.5], C)               # shift 0 (two in three, with mu = 0: no cancellation) or -1/2
        qmu = torch.where((qg == 1.0) & (qs != 0), pick(gen, [0.0, 0.5, -0.5], C), torch.zeros(C, dtype=torch.float64))
        qbeta = qs + qmu * qg                             # in {0, -0.5, -1}
        mu, gamma, beta = torch.where(quiet, qmu, mu), torch.where(quiet, qg, gamma), torch.where(quiet, qbeta, beta)
    on = torch.randperm(C, generator=gen)[:max(1, C // 16)]      # shift == 0 exactly: every zero input sits ON the mask boundary
    mu[on], beta[on] = 0.0, 0.0
    if live is not None:
        gamma[on] = qg[on]
    cancel = (mu != 0) & (beta == mu * gamma)             # beta == mu*gamma != 0: take -beta (in the set), shift = -2 mu gamma
    beta = torch.where(cancel, -beta, beta)
    st = torch.zeros(RS, 2, C, dtype=torch.float64)
    st[0, 0] = count * mu
    st[0, 1] = count * (1.0 - 1e-5 + mu * mu)
    bn = G.BN(name, 'train', C, bt.buf('param', (C,), gamma.float()), bt.buf('param', (C,), beta.float()),
              bt.buf('rstat', (C,), torch.zeros(C)), bt.buf('rstat', (C,), torch.ones(C)), bt.buf('nbt', ()), relu=True)
    bn.count = count
    bn.stats = bt.buf('stats', (RS, 2, C), st)
    return bn, dict(mu=mu, gamma=gamma, beta=beta, shift=beta - mu * gamma)


M1 = [0.0, 0.25, -0.25, 0.5, -0.5]
M2 = [0.0, 0.5, -0.5]


def exact_apply_stats(bt, gen, C, count, mu):
    """The two sums a BN-backward apply reads, as an input: st[0] = count*m1, st[1] = count*m2.  -> (Buf, m1, m2)"""
    m1, m2 = pick(gen, M1, C), pick(gen, M2, C)
    cancel = (m1 != 0) & (mu * m2 == m1)                  # mu*m2 == m1 != 0: take -m1, so mu*m2 - m1 = 2 mu m2
    m1 = torch.where(cancel, -m1, m1)
    st = torch.zeros(RS, 2, C, dtype=torch.float64)
    st[0, 0], st[0, 1] = count * m1, count * m2
    return bt.buf('stats', (RS, 2, C), st), m1, m2


def _limbs(v):
    """A statistics value as the device holds it (csrc/common.h stat_split / stat_join, executor.Arenas.stats_write)."""
    hi = torch.round(v * 2.0 ** 20)
    lo = torch.round((v - hi / 2.0 ** 20) * 2.0 ** 60)
    return hi * (1.0 / 2.0 ** 20) + lo * (1.0 / 2.0 ** 60)


def device_bn_coef(st, gamma, beta, count, eps=EPS_DEVICE):
    """csrc/common.h bn_resolve on [R][2][C] fp64 statistics that went through the limb split -> scale, shift, mean, invstd (fp32)."""
    s = _limbs(st).sum(0)
    m = s[0] / count
    var = (s[1] / count - m * m).clamp_min(0)
    inv = 1.0 / torch.sqrt(var + eps)
    g = gamma.double()
    return (g * inv).float(), (beta.double() - m * g * inv).float(), m.float(), inv.float()


def device_fold_coef(st, bst, gamma, count, eps=EPS_DEVICE):
    """The folded BN-backward apply as conv_c1 / conv_c3 / conv_pp form it: du = A g + B u + D  -> A, B, D (fp32)."""
    s, b = _limbs(st).sum(0), _limbs(bst).sum(0)
    mu = s[0] / count
    var = (s[1] / count - mu * mu).clamp_min(0)
    inv = 1.0 / torch.sqrt(var + eps)
    gi = gamma.double() * inv
    m1, m2 = b[0] / count, b[1] / count
    return gi.float(), (-gi * inv * m2).float(), (gi * (mu * inv * m2 - m1)).float()


class Built:
    """ops: the op list; compare: [(label, Buf or Act)] to check bit for bit; bns: {graph.BN: exact values}; applies: {apply op: (m1, m2)}"""

    def __init__(self):
        self.ops, self.compare, self.bns, self.applies, self.h = [], [], {}, {}, {}

    def bn(self, bt, gen, C, count, name='bn', live=None):
        bn, ex = exact_bn(bt, gen, C, count, name, live)
        self.bns[bn] = ex
        return bn


def budget(n, terms, use_bn):
    """-> (input density, share of freely drawn BN channels or None) of a forward convolution with `terms` non-zero taps per
    output channel over n pixels, so that the second statistics sum keeps its headroom: sum v*v / q^2 < 2^24, i.e.
    mean v*v < 2^24 q^2 / n per channel.  An eighth of that is budgeted (the bound holds per channel; bias, residual and the
    channel means of the operand, which add up coherently over the pixels, weigh on single channels); mean v*v ~ terms * E[w*w] * E[a*a], E[w*w] = 0.625.
      no prologue    v is a multiple of q = 1/4; E[a*a] ~ d / 2 for a raw operand of density d: d follows, at most 0.6
      BN prologue    two taps per channel on up to 2048 pixels: the free draw, v a multiple of 1/16;
                     else the coarse draw of exact_bn() on inputs in {-1, 0, 1} of density 0.6: v a multiple of 1/4, E[a*a] ~ 0.09
                     on a quiet channel (the ReLU keeps 17 % of it) and ~ 4 on a free one (mean included): the share of free channels follows
    (estimates only: the bound itself is asserted by check_reference() on the interpreter's result)"""
    A = 0.125 * 2.0 ** 24 / 16.0 / n / (terms * 0.625)
    if not use_bn:
        return min(0.6, 4.0 * A), None
    if terms == 2 and n <= 2048:
        return 0.6, None
    return 0.6, max(0.0, min(1.0, (A - 0.09) / 4.0))


def forward(bt, gen, dims, wmode, use_bn, use_res, b=None, stride=1):
    """conv (R x R, pad (R - 1) / 2, `stride`) + bias (+ residual) + output statistics, behind an exact train-mode BN+ReLU
    prologue or none."""
    N, H, W, C, K, R = dims
    b = b or Built()
    pad = (R - 1) // 2
    P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    density, live = budget(N * P * Q, C * R * R if wmode == 'dense' else 2, use_bn)
    xv = small(gen, N, H, W, C, density=density)
    if live is not None:                                  # coarse draw: {-1, 0, 1}
        xv = torch.randint(-1, 2, (N, H, W, C), generator=gen).float() * (xv != 0)
    x = bt.act((N, H, W, C), xv, 'x')
    w = bt.buf('wlp', (K, R, R, C), weights(gen, wmode, K, R, C))
    bias = bt.buf('param', (K,), small(gen, K))
    res = bt.act((N, P, Q, K), small(gen, N, P, Q, K), 'res') if use_res else None
    y = bt.act((N, P, Q, K), None, 'y')
    bn = b.bn(bt, gen, C, N * H * W, live=live) if use_bn else None
    ostats = bt.buf('stats', (RS, 2, K), torch.zeros(RS, 2, K, dtype=torch.float64))
    op = G.Op('conv', x=x, w=w, wkey='w', bias=bias, bkey='b', residual=res, y=y, out_stats=ostats, bn=bn, epi='plain',
              epi_x=None, epi_bn=None, epi_stats=None, dims=(N, H, W, C, K, R, R, stride, pad, P, Q))
    b.ops.append(op)
    b.compare += [('y', y), ('out_stats', ostats)]
    return b, op


def wgrad_only(bt, gen, dims, use_bn, stride=1, bias=True):
    """A weight gradient as a launch of its own: dw, dbias of conv(relu(bn(x))) (exact per-channel train-mode prologue, or
    none: the raw x) against dy.  dims = (N, H, W, C, K, R) of the forward convolution.  bias False: dbias = None (a convolution
    without a bias: the launch forms dw alone)."""
    N, H, W, C, K, R = dims
    b = Built()
    pad = (R - 1) // 2
    P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    x = bt.act((N, H, W, C), small(gen, N, H, W, C, density=0.6 if use_bn else 0.3), 'x')
    dy = bt.act((N, P, Q, K), small(gen, N, P, Q, K, density=0.3), 'dy')
    bn = b.bn(bt, gen, C, N * H * W) if use_bn else None
    dw, db = bt.buf('grad', (K, R, R, C), torch.zeros(K, R, R, C)), (bt.buf('grad', (K,), torch.zeros(K)) if bias else None)
    b.ops.append(G.Op('wgrad', x=x, dy=dy, dw=dw, dbias=db, bn=bn, dims=(N, H, W, C, K, R, R, stride, pad, P, Q)))
    b.compare += [('dw', dw)] + ([('dbias', db)] if bias else [])
    return b


def dgrad(bt, gen, dims, wmode, fold, fuse, b=None):
    """The op list of tests.test_conv_c1_gpu._dgrad_ops on exact inputs: forward convolution u = conv(relu(bn(x))), C -> K (R x R);
    its BatchNorm-backward data gradient (K -> C, flipped weights through 'wprep'), optionally behind the folded backward apply
    of the BN on u, and its weight / bias gradient (fused into the data gradient's launch where the kernel offers it)."""
    N, H, W, C, K, R = dims
    b = b or Built()
    pad, cnt = (R - 1) // 2, N * H * W
    x = bt.act((N, H, W, C), small(gen, N, H, W, C), 'x')
    wm = bt.buf('param', (K, R, R, C), weights(gen, wmode, K, R, C))
    wb = bt.buf('wlp', (C, R, R, K))
    dz = bt.act((N, H, W, C), None, 'dz')
    bn = b.bn(bt, gen, C, cnt)
    bst = bt.buf('stats', (RS, 2, C), torch.zeros(RS, 2, C, dtype=torch.float64))
    dw = bt.buf('grad', (K, R, R, C), torch.zeros(K, R, R, C))
    db = bt.buf('grad', (K,), torch.zeros(K))
    b.ops.append(G.Op('wprep', entries=[{'w': wm, 'w_fwd': None, 'w_bwd': wb}]))
    b.compare += [('dz', dz), ('bn-backward sums', bst), ('dw', dw), ('dbias', db)]
    ap = None
    if fold:
        u = bt.act((N, H, W, K), small(gen, N, H, W, K), 'u')
        # (half magnitudes: |g - m1 - (u - mu) m2| <= 1.75, so that the sum of two 'sparse' taps of du stays within 8 bits)
        g = bt.act((N, H, W, K), 0.5 * small(gen, N, H, W, K), 'g')
        du = bt.act((N, H, W, K), None, 'du')
        bn2 = b.bn(bt, gen, K, cnt, 'bn2')
        bst2, m1, m2 = exact_apply_stats(bt, gen, K, cnt, b.bns[bn2]['mu'])
        dgam, dbet = bt.buf('grad', (K,), torch.zeros(K)), bt.buf('grad', (K,), torch.zeros(K))
        ap = G.Op('ew', op='bn_bwd_apply', dims=(N, H, W, K), x=u, x2=None, dy=g, add=None, y=du, out_stats=None, bstats=bst2,
                  dgamma=dgam, dbeta=dbet, bn=bn2)
        b.applies[ap] = (m1, m2)
        b.ops.append(ap)
        dy = du
        b.compare += [('dgamma', dgam), ('dbeta', dbet)]
        b.h['du'] = du
    else:
        dy = bt.act((N, H, W, K), small(gen, N, H, W, K), 'dy')
    wg = G.Op('wgrad', x=x, dy=dy, dw=dw, dbias=db, bn=bn, dims=(N, H, W, C, K, R, R, 1, pad, H, W))
    dg = G.Op('conv', x=dy, w=wb, wkey='w', bias=None, bkey=None, residual=None, y=dz, out_stats=None, bn=None,
              epi='bnrelu_bwd', epi_x=x, epi_bn=bn, epi_stats=bst, dims=(N, H, W, K, C, R, R, 1, R - 1 - pad, H, W))
    if fold:
        dg.fold_apply, dg.fold_wgrad = ap, wg
    if fuse:
        dg.fused_wgrad = wg
    b.ops += [dg, wg]
    b.h['dg'] = dg
    return b


def pair(bt, gen, dims, wmode, use_bn, epi):
    """'conv2': the same convolution at full and at half resolution in one launch, forward ('plain': bias + output statistics,
    optionally an exact BN prologue) or as a BatchNorm-backward data gradient ('bnrelu_bwd')."""
    N, H, W, C, K, R = dims
    b = Built()
    subs = []
    for (h, w_) in ((H, W), (H // 2, W // 2)):
        if epi == 'plain':
            _, op = forward(bt, gen, (N, h, w_, C, K, R), wmode, use_bn, False, b)
            b.ops.pop()
        else:
            x = bt.act((N, h, w_, C), small(gen, N, h, w_, C), 'x')
            wt = bt.buf('wlp', (K, R, R, C), weights(gen, wmode, K, R, C))
            y = bt.act((N, h, w_, K), None, 'y')
            ex = bt.act((N, h, w_, K), small(gen, N, h, w_, K), 'ex')
            ebn = b.bn(bt, gen, K, N * h * w_, 'ebn')
            est = bt.buf('stats', (RS, 2, K), torch.zeros(RS, 2, K, dtype=torch.float64))
            op = G.Op('conv', x=x, w=wt, wkey='', bias=None, bkey='', residual=None, y=y, bn=None, out_stats=None, epi='bnrelu_bwd',
                      epi_x=ex, epi_bn=ebn, epi_stats=est, dims=(N, h, w_, C, K, R, R, 1, (R - 1) // 2, h, w_))
            b.compare += [('dz', y), ('bn-backward sums', est)]
        subs.append(op)
    b.ops.append(G.Op('conv2', a=subs[0], b=subs[1]))
    return b


def stem_dims(N, H, W, K):
    return N, H, W, K, (H - 1) // 2 + 1, (W - 1) // 2 + 1


def exact_eval_bn(bt, gen, C, name='bn1'):
    """-> (graph.BN in eval mode with ReLU, dict of the exact per-channel fp64 values, `on`: the channels with shift == 0).
    running_var = 1 - 1e-5 (in fp32: 1 - 168 * 2^-24): invstd rounds to 1.0f.  The draw and the cancellation rule of exact_bn()."""
    mu, gamma, beta = pick(gen, MU, C), pick(gen, GAMMA, C), pick(gen, BETA, C)
    on = torch.randperm(C, generator=gen)[:max(1, C // 16)]
    mu[on], beta[on] = 0.0, 0.0
    cancel = (mu != 0) & (beta == mu * gamma)
    beta = torch.where(cancel, -beta, beta)
    bn = G.BN(name, 'eval', C, bt.buf('param', (C,), gamma.float()), bt.buf('param', (C,), beta.float()),
              bt.buf('rstat', (C,), mu.float()), bt.buf('rstat', (C,), torch.full((C,), 1.0 - 1e-5)), bt.buf('nbt', ()), relu=True)
    return bn, dict(mu=mu, gamma=gamma, beta=beta, shift=beta - mu * gamma), on


def stem(bt, gen, dims, wmode, stats, act=False):
    """The stem's forward on the fp32 NCHW image: y (+ output statistics), or -- act -- behind it the eval-mode bn1 + ReLU that
    the frozen network's launch applies in its epilogue (graph: stem_fwd.act_ew); compared is then the activation alone."""
    N, H, W, K, P, Q = dims
    b = Built()
    wv, bv = weights(gen, wmode, K, 7, 3), small(gen, K)
    img = bt.buf('image', (N, 3, H, W), small(gen, N, 3, H, W))
    y = bt.act((N, P, Q, K), None, 'stem')
    st = bt.buf('stats', (RS, 2, K), torch.zeros(RS, 2, K, dtype=torch.float64)) if stats else None
    if act:
        bn, ex, on = exact_eval_bn(bt, gen, K)
        wv[on], bv[on] = 0.0, 0.0                         # y == 0 and shift == 0: the whole channel sits on the ReLU boundary
        bn.count = N * P * Q
        b.h['act'] = ex
    op = G.Op('stem_fwd', image=img, w=bt.buf('param', (K, 7, 7, 3), wv), bias=bt.buf('param', (K,), bv), y=y, out_stats=st, dims=dims)
    b.ops.append(op)
    if act:
        a = bt.act((N, P, Q, K), None, 'stem_act')
        op.act_ew = G.Op('ew', op='bnrelu_fwd', dims=(N, P, Q, K), y=a, out_stats=None, x=y, x2=None, dy=None, add=None, bstats=None,
                         dgamma=None, dbeta=None, bn=bn)
        b.ops.append(op.act_ew)
        b.compare += [('stem act', a)]
    else:
        b.compare += [('y', y)] + ([('out_stats', st)] if stats else [])
    b.h['stem'] = op
    return b


def stem_weight_gradient(bt, gen, dims):
    N, H, W, K, P, Q = dims
    b = Built()
    img = bt.buf('image', (N, 3, H, W), small(gen, N, 3, H, W))
    dy = bt.act((N, P, Q, K), small(gen, N, P, Q, K, density=0.3), 'dy')
    dw, db = bt.buf('grad', (K, 7, 7, 3), torch.zeros(K, 7, 7, 3)), bt.buf('grad', (K,), torch.zeros(K))
    b.ops.append(G.Op('stem_wgrad', image=img, dy=dy, dw=dw, dbias=db, dims=dims))
    b.compare += [('dw', dw), ('dbias', db)]
    b.h['stem'] = b.ops[0]
    return b


# ---------------------------------------------------------------------------------------------------------------------
# the checks on the reference
def quantum(t):
    """Smallest power of two that every element of t is a multiple of (1.0 for an all-zero tensor)."""
    t = t.double().reshape(-1)
    t = t[t != 0]
    q = 1.0
    while t.numel() and not torch.equal(t / q, torch.round(t / q)):
        q *= 0.5
        assert q > 2.0 ** -40, 'not a small dyadic tensor'
    return q


def _headroom(total, q, label):
    worst = float(total.max()) / q if total.numel() else 0.0
    assert worst < LIMIT, '%s: sum |addend| = %.0f units of 2^%d -- not below 2^24, the fp32 sums are not exact in every grouping' % (
        label, worst, int(np.log2(q)))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _check_bn(A, bn, ex, xv, label):
    scale, shift, mean, invstd = PI._bn_coef(A, bn)
    assert torch.equal(scale.double(), ex['gamma']) and torch.equal(shift.double(), ex['shift']), label + ': scale / shift not exact'
    assert torch.equal(mean.double(), ex['mu']) and bool((invstd == 1.0).all()), label + ': mean / invstd not exact'
    if xv is None:
        return
    z = torch.addcmul(shift, xv, scale)
    on = float((z == 0).float().mean())
    assert on > 0.01, '%s: only %.2f %% of the elements sit on the mask boundary' % (label, 100 * on)
    keep = float((z > 0).float().mean())
    assert 0.1 <= keep <= 0.9, '%s: the ReLU mask keeps %.1f %%' % (label, 100 * keep)


def _check_conv(A, b, op, label):
    n, h, w, C, K, R, S, stride, pad, P, Q = op.dims
    x = PI._act(A, op.x)
    if op.bn is not None:
        _check_bn(A, op.bn, b.bns[op.bn], x, label + ' prologue')
        x = PI._prologue(A, x, op.bn)
    wt = A.view(op.w).float()
    acc = F.conv2d(_nchw(x.abs()).double(), _nchw(wt.abs()).double(), None, stride=stride, padding=pad)
    extra = [A.view(op.bias).double()] if op.bias is not None else []
    extra += [PI._act(A, op.residual).double()] if op.residual is not None else []
    q = min([quantum(x) * quantum(wt)] + [quantum(e) for e in extra])
    _headroom(acc + 2.0, q, label + ' accumulator')       # (+ |bias| + |residual| <= 2)
    y = PI._act(A, op.y).double()
    assert float(y.abs().max()) > 0, label + ': all-zero output'
    if op.epi == 'bnrelu_bwd':
        xv = PI._act(A, op.epi_x)
        _check_bn(A, op.epi_bn, b.bns[op.epi_bn], xv, label + ' epilogue')
        xhat = (xv.double() - b.bns[op.epi_bn]['mu'])
        _headroom(y.abs().sum((0, 1, 2)), quantum(y), label + ' sum dz')
        _headroom((y * xhat).abs().sum((0, 1, 2)), quantum(y) * quantum(xhat), label + ' sum dz*xhat')
        st = A.view(op.epi_stats).sum(0)
        assert float(st[0].abs().max()) > 0 and float(st[1].abs().max()) > 0, label + ': all-zero sums'
    elif op.out_stats is not None:
        _headroom(y.abs().sum((0, 1, 2)), quantum(y), label + ' sum v')
        _headroom((y * y).sum((0, 1, 2)), quantum(y) ** 2, label + ' sum v*v')


def _check_wgrad(A, b, op, label):
    n, h, w, C, K, R, S, stride, pad, P, Q = op.dims
    if op.bn is not None:
        _check_bn(A, op.bn, b.bns[op.bn], PI._act(A, op.x), label + ' prologue')
    a = PI._prologue(A, PI._act(A, op.x), op.bn).double()
    dy = PI._act(A, op.dy).double()
    tot = torch.nn.grad.conv2d_weight(_nchw(a.abs()), (K, C, R, S), _nchw(dy.abs()), stride=stride, padding=pad)
    _headroom(tot, quantum(a) * quantum(dy), label + ' dw')
    assert float(A.view(op.dw).abs().max()) > 0, label + ': all-zero gradient'
    if op.dbias is not None:                              # (a launch without a bias gradient forms dw alone)
        _headroom(dy.abs().sum((0, 1, 2)), quantum(dy), label + ' dbias')
        assert float(A.view(op.dbias).abs().max()) > 0, label + ': all-zero bias gradient'


def _check_apply(A, b, op, label):
    m1, m2 = b.applies[op]
    ex = b.bns[op.bn]
    _check_bn(A, op.bn, ex, None, label + ' folded BN')       # (coefficients only: a backward apply has no ReLU)
    u, g = PI._act(A, op.x).double(), PI._act(A, op.dy).double()
    du = ex['gamma'] * (g - m1 - (u - ex['mu']) * m2)
    assert torch.equal(PI._act(A, op.y).double(), du), label + ': du is not the exact value'
    assert torch.equal(du, torch.round(du * 16) / 16) and float(du.abs().max()) <= 4.5
    assert torch.equal(A.view(op.dgamma).double(), op.bn.count * m2) and torch.equal(A.view(op.dbeta).double(), op.bn.count * m1)
    assert not bool(((ex['mu'] * m2 - m1 == 0) & (m1 != 0)).any()), label + ': mu*m2 - m1 cancels'


def _stem_operands(A, op, label):
    img, wt = A.view(op.image), (A.view(op.w) if op.kind == 'stem_fwd' else None)
    for t in (img, wt):                                   # one specification for the rounding and the non-rounding back ends
        assert t is None or torch.equal(t.bfloat16().float(), t), label + ': an operand is not bf16-representable'
    return img.double(), (wt.permute(0, 3, 1, 2).double() if wt is not None else None)


def _check_stem(A, b, op, label):
    N, H, W, K, P, Q = op.dims
    img, wt = _stem_operands(A, op, label)
    bias = A.view(op.bias).double()
    acc = F.conv2d(img.abs(), wt.abs(), None, stride=2, padding=3) + bias.abs().view(1, K, 1, 1)
    _headroom(acc, min(quantum(img) * quantum(wt), quantum(bias)), label + ' accumulator')
    y = PI._act(A, op.y).double()
    assert float(y.abs().max()) > 0, label + ': all-zero output'
    if op.out_stats is not None:
        d = y - bias                                      # what the space-to-depth kernel adds up per lane, in fp32
        qy, qd = quantum(y), min(quantum(y), quantum(bias))
        _headroom(y.abs().sum((0, 1, 2)), qy, label + ' sum y')
        _headroom((y * y).sum((0, 1, 2)), qy * qy, label + ' sum y*y')
        _headroom(d.abs().sum((0, 1, 2)), qd, label + ' sum (y - bias)')
        _headroom((d * d).sum((0, 1, 2)), qd * qd, label + ' sum (y - bias)^2')
        st = A.view(op.out_stats).sum(0)
        assert float(st[0].abs().max()) > 0 and float(st[1].abs().max()) > 0, label + ': all-zero statistics'
    ae = op.act_ew
    if ae is None:
        return
    ex, bn = b.h['act'], ae.bn
    assert not bool(((ex['shift'] == 0) & (ex['mu'] != 0)).any()), label + ': beta - mean*gamma cancels'
    scale, shift, mean, invstd = PI._bn_coef(A, bn)
    assert torch.equal(scale.double(), ex['gamma']) and torch.equal(shift.double(), ex['shift']), label + ': scale / shift not exact'
    assert torch.equal(mean.double(), ex['mu']) and bool((invstd == 1.0).all()), label + ': mean / invstd not exact'
    # the device's arithmetic (csrc/common.h bn_resolve, eval mode): fp32 running estimates, eps = (double)(float)1e-5
    inv = 1.0 / torch.sqrt(A.view(bn.rvar).double() + EPS_DEVICE)
    g = A.view(bn.gamma).double()
    assert torch.equal((g * inv).float().double(), ex['gamma']), label + ': device scale not exact'
    assert torch.equal((A.view(bn.beta).double() - A.view(bn.rmean).double() * g * inv).float().double(), ex['shift']), label + ': device shift not exact'
    z = torch.addcmul(shift, PI._act(A, op.y), scale)
    on, keep = float((z == 0).float().mean()), float((z > 0).float().mean())
    assert on > 0.01, '%s: only %.2f %% of the elements sit on the mask boundary' % (label, 100 * on)
    assert 0.1 <= keep <= 0.9, '%s: the ReLU mask keeps %.1f %%' % (label, 100 * keep)
    dead = (ex['shift'] == 0) & (A.view(op.w).abs().sum((1, 2, 3)) == 0) & (A.view(op.bias) == 0)
    assert bool(dead.any()) and bool((z[..., dead] == 0).all()), label + ': no channel lies on the boundary as a whole'
    assert float(PI._act(A, ae.y).abs().max()) > 0, label + ': all-zero activation'


def _check_stem_wgrad(A, b, op, label):
    N, H, W, K, P, Q = op.dims
    img, _ = _stem_operands(A, op, label)
    dy = _nchw(PI._act(A, op.dy).double())
    tot = torch.nn.grad.conv2d_weight(img.abs(), (K, 3, 7, 7), dy.abs(), stride=2, padding=3)
    _headroom(tot, quantum(img) * quantum(dy), label + ' dw')
    _headroom(dy.abs().sum((0, 2, 3)), quantum(dy), label + ' dbias')
    assert float(A.view(op.dw).abs().max()) > 0 and float(A.view(op.dbias).abs().max()) > 0, label + ': all-zero gradient'


def check_reference(A, b, label=''):
    """The preconditions of a bit-exact comparison, asserted on the arenas the interpreter has run `b.ops` over."""
    for ex in b.bns.values():
        assert not bool(((ex['shift'] == 0) & (ex['mu'] != 0)).any()), label + ': beta - mu*gamma cancels'
    for op in b.ops:
        for o in ((op.a, op.b) if op.kind == 'conv2' else (op,)):
            if o.kind == 'conv':
                _check_conv(A, b, o, label + ' conv')
            elif o.kind == 'wgrad':
                _check_wgrad(A, b, o, label + ' wgrad')
            elif o.kind == 'stem_fwd':                    # (with its act_ew, the 'ew' op behind it)
                _check_stem(A, b, o, label + ' stem')
            elif o.kind == 'stem_wgrad':
                _check_stem_wgrad(A, b, o, label + ' stem wgrad')
            elif o.kind == 'ew' and o.op == 'bn_bwd_apply':
                _check_apply(A, b, o, label + ' apply')


# ---------------------------------------------------------------------------------------------------------------------
# case lists (shapes of the random-input tests of the same kernels, capped at 4 x 32 x 32 x 128 elements per tensor)
def _cap(N, H, W, ch):
    """At most 2^19 elements and 4096 pixels: the maps keep their width (the tile geometry), lose images, then rows."""
    while N > 1 and (N * H * W * ch > 2 ** 19 or N * H * W > 4096):
        N -= 1
    while N * H * W * ch > 2 ** 19 or N * H * W > 4096:
        H //= 2
    return N, H, W


# conv_c1 forward: (N, H, W, C, K, blocks).  Every (C, K) of the random-input cases at 16 tiles with ONE block (two rounds in a
# loop), the ragged / idle-block shapes, more blocks than rounds, an uneven split of 8 rounds (3 / 3 / 2)
C1_FWD = [(2, 16, 16, c, k, 1) for c, k in sorted({(c[3], c[4]) for c in _c1.FWD_CASES})] + [
    (1, 4, 40, 128, 64, 2), (3, 4, 8, 64, 128, 1), (1, 8, 52, 64, 64, 3), (2, 32, 32, 32, 128, 256), (2, 32, 32, 128, 64, 3)]
C1_FWD_VARIANTS = [(True, True), (True, False), (False, True), (False, False)]      # (BN prologue, residual)
# conv_c1 data gradient: forward convolution C -> K.  (N, H, W, C, K, blocks)
C1_BWD = [(1, 4, 40, 64, 128, 2), (3, 4, 8, 128, 64, 1), (1, 8, 52, 64, 128, 3), (2, 32, 32, 128, 64, 3), (4, 32, 32, 64, 128, 5)]
# ... of the score (128 -> 16) and fc_ (128 -> 128) convolutions: taken unfolded, weight gradient a launch of its own
C1_BWD_UNFUSED = [(3, 16, 16, 128, 16, 2), (2, 32, 32, 128, 16, 3), (3, 16, 16, 128, 128, 2), (2, 32, 32, 128, 128, 3)]
C1_PAIR = [c[:5] + (c[5] is not None, c[6], c[7]) for c in _c1.PAIR_CASES]          # (N, H, W, C, K, bn, epi, blocks)


def _c3_cap(N, H, W):
    return (1 if H * W == 64 * 64 else N), H, W


# conv_c3 (C = K = 64, 3x3): (N, H, W, bn, blocks) / (N, H, W, blocks); 64 x 64 maps at N = 1
C3_FWD = [_c3_cap(*c[:3]) + (c[3] is not None, c[5]) for c in _c3.FWD_CASES]
C3_BWD = [_c3_cap(*c[:3]) + (c[3],) for c in _c3.BWD_CASES]
# (the pair shapes of tests/test_conv_c3_gpu.py test_c3_pair)  (N, H, W, bn, epi, blocks)
C3_PAIR = [(1, 64, 64, True, 'plain', 6), (3, 32, 32, True, 'plain', 3), (1, 64, 64, False, 'bnrelu_bwd', 5)]
# forced conv_pp: (N, H, W, C, K, R, bn, residual, blocks)
PP_FWD = [_cap(c[0], c[1], c[2], max(c[3], c[4])) + (c[3], c[4], c[5], c[6] is not None, c[7], c[8]) for c in _tk.PP_CASES]
# ... data gradient with fold and fused weight gradient: two 1x1 rows of FOLD_CASES.  (N, H, W, C, K, blocks)
PP_BWD = [c[:5] + (c[6],) for c in _tk.FOLD_CASES if c in ((3, 20, 48, 64, 32, 1, 3, True), (2, 32, 32, 128, 64, 1, 4, True))]
assert (len(PP_BWD), len(C1_PAIR), len(C3_FWD), len(C3_BWD), len(PP_FWD)) == (2, 4, 8, 5, 12), 'a case list this module derives from has changed'


# The halo-tile kernels (csrc/conv_tile.hip, csrc/wgrad_tile.hip; tests/test_exact_tile_gpu.py with conv_c1 / conv_c3 / conv_pp
# off, both storage types).  conv_tile is compiled for T x BK {64, 32, 16} x TN {1, 2, 4} x ALLW x FOLD; which instantiation a
# shape launches is the library's answer (fpd_conv_tile_variant), and tests/test_exact_variants_cpu.py asserts that these lists
# reach every instantiation a launch can reach.  The comments name the bf16 variant; fp32 storage chunks by 32 or 16 channels.
BOTH, BF16, F32 = (1, 0), (1,), (0,)
# forward: (N, H, W, C, K, R, BN prologue, residual, storage types)
TILE_FWD = [c + v + (BF16 if c[2] == 128 else BOTH,) for c, v in [
    ((2, 8, 6, 16, 16, 1), (True, True)),          # BK16 TN1, the smallest of everything
    ((3, 16, 12, 48, 48, 3), (True, False)),       # BK16 TN1, three chunks, tiles of 10 rows straddling images
    ((4, 64, 48, 48, 48, 3), (True, True)),        # BK16 TN2: HRNet-W48 branch 1
    ((4, 64, 48, 48, 96, 3), (True, False)),       # BK16 TN4, 96 of 128 accumulator columns live
    ((3, 16, 12, 96, 192, 3), (True, True)),       # BK32 TN1
    ((4, 64, 48, 32, 48, 1), (True, True)),        # BK32 TN2
    ((4, 64, 48, 32, 48, 3), (False, True)),       # BK32 TN2; fp32: one chunk, ALLW at TN2
    ((4, 64, 48, 96, 192, 1), (True, False)),      # BK32 TN4
    ((2, 8, 6, 64, 16, 3), (True, True)),          # BK64 TN1 ALLW
    ((2, 8, 6, 384, 96, 3), (True, True)),         # BK64 TN1, six chunks
    ((4, 64, 48, 64, 48, 3), (True, False)),       # BK64 TN2 ALLW
    ((2, 64, 48, 128, 128, 3), (True, False)),     # BK64 TN2
    ((2, 64, 48, 192, 256, 1), (True, True)),      # BK64 TN4, all 128 columns live
    ((2, 44, 48, 48, 384, 3), (True, True)),       # BK16 TN4 with three channel tiles of 128; 44 rows: the last tile of an image ends early
    ((2, 64, 48, 16, 192, 1), (False, False)),     # BK16 TN4 without a prologue
    ((1, 6, 128, 64, 64, 3), (True, False)),       # the 64-channel halo of 128-wide rows does not fit: BK32 (fp32: no narrower chunk, declined)
    ((3, 20, 48, 32, 64, 3), (True, True)),        # ragged tiles; fp32: ALLW at TN1
    ((5, 7, 6, 384, 96, 3), (False, True)),        # tiles of 21 rows over images of 7
    ((2, 32, 24, 64, 64, 3), (True, True)),        # tiles of 5 rows straddling images
]]
# data gradient: forward convolution (N, H, W, C, K, R): the gradient reads K channels (the chunk) and writes C (the n-tiling).
# Each runs unfolded and with the fold asked for; FOLD is compiled for TN <= 2 and C, K <= 128 -- (4, 64, 48, 128, 64, 1) runs at
# TN4: the route declines the fold, the stand-alone apply runs, the result is the same
TILE_BWD = [
    (4, 64, 48, 48, 32, 3),       # BK32 TN2 (fp32: ALLW)
    (4, 64, 48, 64, 128, 1),      # BK64 TN2
    (2, 64, 48, 128, 64, 3),      # BK64 TN2 ALLW
    (3, 16, 12, 96, 48, 3),       # BK16 TN1
    (2, 32, 24, 48, 96, 3),       # BK32 TN1
    (4, 64, 48, 64, 16, 1),       # BK16 TN2
    (3, 16, 12, 32, 128, 3),      # BK64 TN1, two chunks
    (2, 8, 6, 32, 64, 3),         # BK64 TN1 ALLW
    (3, 16, 12, 48, 32, 3),       # BK32 TN1 (fp32: ALLW)
    (4, 64, 48, 128, 64, 1),      # BK64 TN4: no FOLD variant
]
TILE_BWD_TN4 = (4, 64, 48, 128, 64, 1)
assert TILE_BWD_TN4 in TILE_BWD
# pairs (full and half resolution in one launch): (N, H, W, C, K, R, BN prologue, epilogue)
TILE_PAIR = [c + v for c in [(2, 32, 32, 64, 64, 3), (2, 32, 24, 48, 96, 3), (3, 16, 12, 96, 48, 1)]
             for v in ((True, 'plain'), (False, 'bnrelu_bwd'))]
# wgrad_tile_kernel<T, R, TP, H4, SMALL>: (N, H, W, C, K, R, BN prologue, storage types).  bf16 3x3 cases stay outside wgrad3's
# domain (C = K in {32, 64}, power-of-two width, with slabs: W3_WGRAD below is the list inside it); each runs with slabs and, up
# to 8192 pixels, with the single-block flush
TILE_WGRAD = [
    (2, 16, 48, 128, 64, 3, True, BOTH),       # <T, 3, 128>: two (bf16) / four (fp32) channel tiles -- the table is indexed c0 + c
    (1, 16, 16, 192, 64, 3, True, BOTH),       # three channel tiles, a power-of-two width
    (2, 16, 48, 48, 96, 3, True, BOTH),        # cn < CW; K tail (96 = 64 + 32)
    (2, 32, 24, 64, 64, 3, True, BOTH),        # <bf16, 3, 128, H4> (fp32: rows of 24 are k-step aligned, the plain kernel)
    (3, 16, 12, 128, 32, 3, True, BF16),       # H4 at W = 12, two channel tiles
    (2, 64, 48, 32, 32, 3, True, BOTH),        # <bf16, 3, 128, false, SMALL>
    (2, 32, 24, 64, 128, 1, True, BOTH),       # <T, 1, 128>, KSPLIT, an HRNet width
    (2, 16, 48, 192, 96, 1, True, BOTH),       # ... three channel tiles, K tail
    (3, 16, 48, 64, 64, 1, False, BOTH),       # ... without a prologue
    (16, 64, 64, 16, 16, 1, True, BOTH),       # <T, 1, 256>: from 65536 pixels with 256 % W == 0 -- the smallest such shape
]


def wgrad_flushes(case):
    """The flushes a TILE_WGRAD case runs with: slabs (True) and, on a small problem, the single block per (k, c) tile (False)."""
    return (True, False) if case[0] * case[1] * case[2] <= 8192 else (True,)


# wgrad3 (csrc/wgrad3.hip, the specialised-wave kernel; bf16, 3x3, C = K in {32, 64}, W in {16, 32, 64, 128}, with slabs;
# tests/test_exact_wgrad3_gpu.py): (N, H, W, C, K, BN prologue).  A tile is 256 pixels = nrows = 256 / W flat image rows, the
# N*H / nrows tiles are cut into contiguous ranges, a block owns one 32 x 32 piece of one range and keeps the halo in a ring of
# 2 nrows + 2 rows.  The comments give tiles, ranges and the tiles per range as w3_geometry() below -- the restatement of the
# library's launch geometry -- finds them; tests/test_exact_wgrad3_cpu.py asserts the restatement against the library's answers
# and that the list reaches the geometries named here.  No tensor has more than 65536 pixels.
W3_WGRAD = [
    (1, 16, 16, 64, 64, True),       # 1, 1, {1}: one tile = one image, both halo rows outside; 28 of 32 blocks idle
    (2, 16, 16, 64, 64, True),       # 2, 1, {2}: the prefetch of tile i + 2 finds nothing; an image change between the tiles
    (3, 16, 16, 64, 64, False),      # 3, 1, {3}: no prologue; two image changes
    (2, 24, 16, 64, 64, True),       # 3, 1, {3}: H % nrows != 0 -- the middle tile STRADDLES two images (rows 16..23 | 0..7)
    (2, 12, 32, 32, 32, True),       # ... at nrows = 8, one piece
    (2, 6, 64, 64, 64, True),        # ... at nrows = 4
    (1, 8, 32, 64, 64, True),        # 1, 1, {1}: H == nrows at every width
    (1, 4, 64, 64, 64, True),
    (1, 2, 128, 64, 64, True),       # ... W = 128: the two leading rows are staged as four vectors per thread
    (3, 2, 128, 32, 32, True),       # 3, 1, {3}: W = 128, every tile a whole image, one piece
    (1, 14, 128, 32, 32, True),      # 7, 1, {7}: the ring of 6 rows wraps three times
    (3, 6, 128, 64, 64, True),       # 9, 2, {4, 5}: uneven cut; the second range starts in the middle of an image
    (5, 24, 32, 32, 32, False),      # 15, 3, {5}: one piece, 3 of 8 blocks live, start slots {0, 4, 8}
    (17, 16, 16, 32, 32, True),      # 17, 4, {4, 5}: start slots {0, 30, 26, 22} of a ring of 34; four image changes in a range
    (3, 40, 64, 32, 32, True),       # 30, 7, {4, 5}: 7 ranges in a grid of 8 -- one idle block in a full group
    (2, 64, 64, 64, 64, True),       # 32, 8, {4}: the first full group, 4 pieces x 8 ranges, no idle block
    (9, 32, 32, 64, 64, True),       # 36, 8, {4, 5}: 9 ranges rounded down to 8; start slots {0, 14}
    (5, 40, 64, 64, 64, True),       # 50, 8, {6, 7}: image changes in the middle of the ranges
    (5, 52, 64, 64, 64, True),       # 65, 16, {4, 5}: a second group of eight with an uneven cut
    (9, 40, 32, 32, 32, True),       # 45, 8, {5, 6}: eight distinct start slots
    (1, 64, 128, 32, 32, True),      # 32, 8, {4}: W = 128 at 8 ranges
    (2, 40, 128, 32, 32, True),      # 40, 8, {5}
    (2, 128, 128, 32, 32, True),     # 128, 32, {4}: the shape class of the student's layer1 -- 32 ranges, four groups, one piece
    (16, 64, 64, 32, 32, False),     # 256, 64, {4}: the largest grid a one-piece launch gets; 65536 pixels, the cap of TILE_WGRAD
]
# ... and one launch without a bias gradient, at 4 pieces: the bias lanes of the ct == 0 pieces are there and stay unused
W3_NO_BIAS = (9, 32, 32, 64, 64, True)
assert W3_NO_BIAS in W3_WGRAD and all(c[0] * c[1] * c[2] <= 65536 for c in W3_WGRAD)


def w3_geometry(N, H, W, C, K, ranges=32):
    """csrc/wgrad3.hip w3_grid() and the kernel's block map restated (ranges: FPD_WGRAD3_RANGES, default 32) -> None where the
    kernel declines, else a dict: nrows, ring, mtiles, npieces, nranges, blocks, cuts (fpd_cut: range i walks tiles
    cuts[i] .. cuts[i + 1] - 1), live = {block: (range, piece)} of the blocks that do not return at once."""
    if not ((C, K) in ((64, 64), (32, 32)) and W in (16, 32, 64, 128)):
        return None
    nrows = 256 // W
    if (N * H) % nrows != 0 or nrows > H:
        return None
    mtiles, npieces = N * H // nrows, (K // 32) * (C // 32)
    r = min(ranges * 4 // npieces, max(1, mtiles // 4))
    if r >= 8:
        r = r // 8 * 8
    nranges = max(1, min(r, mtiles))
    blocks = (nranges + 7) // 8 * 8 * npieces
    live = {}
    for b in range(blocks):
        q = b >> 3
        rng = (q // npieces) * 8 + (b & 7)
        if rng < nranges:
            live[b] = (rng, q % npieces)
    return dict(nrows=nrows, ring=2 * nrows + 2, mtiles=mtiles, npieces=npieces, nranges=nranges, blocks=blocks,
                cuts=[i * mtiles // nranges for i in range(nranges + 1)], live=live)


# stride 2 (3x3, pad 1; HRNet's transitions and fuse layers, the 3 -> 64 stem convolution): conv_mfma / conv_smallc / conv_naive
# and their weight gradients.  (N, H, W, C, K) of tests/test_hrnet_gpu.py S2; a BN prologue where C % 8 == 0
S2 = [(2, 16, 12, 32, 64), (2, 32, 24, 16, 16), (1, 64, 48, 64, 128), (3, 8, 6, 8, 8), (2, 64, 64, 3, 64)]


# the stem: (N, H, W, K, blocks) with P = (H - 1) / 2 + 1, Q = (W - 1) / 2 + 1; at most 4096 output pixels.  blocks = the
# "stem_blocks" option of the launch (0: the kernels' defaults); tiles are 128 output pixels = 128 / Q whole rows
def _even(N, P, Q, K, blocks):
    return N, 2 * P, 2 * Q, K, blocks


# space-to-depth kernels (bf16, H = 2P, W = 2Q, Q a power of two in 16..128):
STEM_S2D = [
    _even(2, 8, 16, 8, 1),         # two images, one tile each, one block: full reload at the image change; smallest K
    _even(1, 24, 16, 24, 1),       # three continuing tiles: the 19-row ring wraps; weight rows beyond K zeroed
    _even(3, 16, 16, 32, 2),       # 6 tiles split 3 / 3: the second block starts in the middle of an image (its halo above is real rows)
    _even(2, 8, 32, 32, 3),        # 4 tiles over 3 blocks (uneven fpd_cut)
    _even(1, 12, 32, 40, 1),       # two channel tiles, the second half-live
    _even(2, 6, 64, 64, 2),        # 6 tiles over 2 blocks, Q = 64
    _even(2, 3, 128, 64, 1),       # one row per tile: a ring of 5 that wraps every tile
    _even(1, 5, 128, 16, 7),       # cap above the tile count
    _even(2, 8, 16, 32, 0),        # the default grid
]
STEM_ACT = [c for c in STEM_S2D if c[3] in (8, 32, 40, 64)]
# the same (P, Q) with an odd size: the space-to-depth form declines, the im2col kernels (csrc/stem_mfma.hip) serve
STEM_MFMA = [(2, 15, 32, 8, 0), (1, 32, 63, 32, 0), (2, 7, 127, 40, 0), (1, 5, 255, 64, 0), (2, 15, 63, 64, 0)]
# direct kernels (csrc/stem.hip; 8 x 16 tiles): (N, H, W, K, dtype, backend) -- tiles ragged in both directions with an odd K;
# Q = 24; Q = 96 with P = 9; each in both storage types; a space-to-depth shape in fp32 and under the direct back end
STEM_DIRECT = [c + (dt, 0) for c in ((2, 21, 37, 5), (1, 16, 48, 16), (1, 18, 192, 64)) for dt in (1, 0)] + [
    (2, 16, 32, 32, 0, 0), (2, 16, 32, 32, 1, 1)]
# weight gradient: (N, H, W, K, blocks, dtype); blocks = the cap of the third mode of the device test (an uneven split of the
# tiles wherever there are more than two).  space-to-depth: K <= 32; im2col <32>: the odd shapes with K <= 32; im2col <64>:
# K = 40 and 64, even and odd sizes; direct (K divides 256): Q in {24, 96} and fp32
STEM_WGRAD_S2D = [_even(2, 8, 16, 8, 1), _even(1, 24, 16, 24, 2), _even(3, 16, 16, 32, 4), _even(2, 8, 32, 32, 3), _even(1, 5, 128, 16, 2),
                  _even(2, 8, 16, 32, 1)]
STEM_WGRAD_MFMA = [(2, 15, 32, 8, 1), (1, 32, 63, 32, 3), _even(1, 12, 32, 40, 2), _even(2, 6, 64, 64, 4), _even(2, 3, 128, 64, 4),
                   (2, 7, 127, 40, 3)]
STEM_WGRAD_DIRECT = [(1, 16, 48, 16, 1, 1), (1, 16, 48, 16, 1, 0), (3, 16, 48, 16, 4, 1), (1, 18, 192, 64, 5, 1), (1, 18, 192, 64, 5, 0),
                     (2, 16, 32, 8, 1, 0)]
STEM_WGRAD = [c + (1,) for c in STEM_WGRAD_S2D + STEM_WGRAD_MFMA] + STEM_WGRAD_DIRECT
assert all(c[0] * stem_dims(*c[:4])[4] * stem_dims(*c[:4])[5] <= 4096 for c in STEM_S2D + STEM_MFMA + STEM_DIRECT + STEM_WGRAD)


def seed(*parts):
    """A generator seeded by the case (ints, bools and short strings)."""
    s = 0
    for p in parts:
        for v in (p if isinstance(p, tuple) else (p,)):
            s = (s * 31 + (sum(map(ord, v)) if isinstance(v, str) else int(v))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(1000 + s)


# ---------------------------------------------------------------------------------------------------------------------
# one builder per test family: (bench, parameters...) -> Built.  FAMILIES lists every parameter tuple of every family, for the
# device tests and for the precondition tests alike
def c1_forward(bt, case, wmode, variant):
    return forward(bt, seed('c1f', case, wmode, variant), case[:5] + (1,), wmode, *variant)[0]


def c1_dgrad(bt, case, wmode, fold, fuse):
    return dgrad(bt, seed('c1b', case, wmode, fold, fuse), case[:5] + (1,), wmode, fold, fuse)


def c1_dgrad_unfused(bt, case, wmode):
    return dgrad(bt, seed('c1u', case, wmode), case[:5] + (1,), wmode, False, True)


def c1_pair(bt, case, wmode):
    return pair(bt, seed('c1p', case, wmode), case[:5] + (1,), wmode, case[5], case[6])


def c3_forward(bt, case, wmode):
    return forward(bt, seed('c3f', case, wmode), case[:3] + (64, 64, 3), wmode, case[3], False)[0]


def c3_dgrad(bt, case, wmode, fold):
    return dgrad(bt, seed('c3b', case, wmode, fold), case[:3] + (64, 64, 3), wmode, fold, False)


def c3_pair(bt, case, wmode):
    return pair(bt, seed('c3p', case, wmode), case[:3] + (64, 64, 3), wmode, case[3], case[4])


def pp_forward(bt, case, wmode):
    return forward(bt, seed('ppf', case, wmode), case[:6], wmode, case[6], case[7])[0]


def pp_dgrad(bt, case, wmode):
    return dgrad(bt, seed('ppb', case, wmode), case[:5] + (1,), wmode, True, True)


def stem_forward(bt, case, wmode, stats):
    return stem(bt, seed('stf', case[:4], wmode, stats), stem_dims(*case[:4]), wmode, stats)


def stem_act(bt, case, wmode):
    return stem(bt, seed('sta', case[:4], wmode), stem_dims(*case[:4]), wmode, False, act=True)


def stem_wgrad(bt, case):
    return stem_weight_gradient(bt, seed('stw', case[:4]), stem_dims(*case[:4]))


def tile_forward(bt, case, wmode):
    return forward(bt, seed('tf', case[:8], wmode), case[:6], wmode, case[6], case[7])[0]


def tile_dgrad(bt, case, wmode, fold):
    return dgrad(bt, seed('tb', case, wmode, fold), case, wmode, fold, False)


def tile_pair(bt, case, wmode):
    return pair(bt, seed('tp', case, wmode), case[:6], wmode, case[6], case[7])


def tile_wgrad(bt, case):
    return wgrad_only(bt, seed('tw', case[:7]), case[:6], case[6])


def w3_wgrad(bt, case, bias=True):
    return wgrad_only(bt, seed('w3', case, bias), case[:5] + (3,), case[5], bias=bias)


def s2_forward(bt, case, wmode):
    return forward(bt, seed('s2f', case, wmode), case + (3,), wmode, case[3] % 8 == 0, False, stride=2)[0]


def s2_wgrad(bt, case):
    return wgrad_only(bt, seed('s2w', case), case + (3,), case[3] % 8 == 0, stride=2)


_STEM_FWD = STEM_S2D + STEM_MFMA + sorted({c[:4] + (0,) for c in STEM_DIRECT} - set(STEM_S2D))
_STEM_WG = sorted({c[:4] for c in STEM_WGRAD})
FAMILIES = [
    (c1_forward, [(c, m, v) for c in C1_FWD for m in WMODES for v in C1_FWD_VARIANTS]),
    (c1_dgrad, [(c, m, fo, fu) for c in C1_BWD for m in WMODES for fo in (False, True) for fu in (False, True)]),
    (c1_dgrad_unfused, [(c, m) for c in C1_BWD_UNFUSED for m in WMODES]),
    (c1_pair, [(c, m) for c in C1_PAIR for m in WMODES]),
    (c3_forward, [(c, m) for c in C3_FWD for m in WMODES]),
    (c3_dgrad, [(c, m, fo) for c in C3_BWD for m in WMODES for fo in (False, True)]),
    (c3_pair, [(c, m) for c in C3_PAIR for m in WMODES]),
    (pp_forward, [(c, m) for c in PP_FWD for m in WMODES]),
    (pp_dgrad, [(c, m) for c in PP_BWD for m in WMODES]),
    (stem_forward, [(c, m, s) for c in _STEM_FWD for m in WMODES for s in (True, False)]),
    (stem_act, [(c, m) for c in STEM_ACT for m in WMODES]),
    (stem_wgrad, [(c,) for c in _STEM_WG]),
    (tile_forward, [(c, m) for c in TILE_FWD for m in WMODES]),
    (tile_dgrad, [(c, m, fo) for c in TILE_BWD for m in WMODES for fo in (False, True)]),
    (tile_pair, [(c, m) for c in TILE_PAIR for m in WMODES]),
    (tile_wgrad, [(c,) for c in TILE_WGRAD]),
    (w3_wgrad, [(c, True) for c in W3_WGRAD] + [(W3_NO_BIAS, False)]),
    (s2_forward, [(c, m) for c in S2 for m in WMODES]),
    (s2_wgrad, [(c,) for c in S2]),
]
