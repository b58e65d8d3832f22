"""Cases, input constructions and the grid arithmetic of the tests that drive the two persistent kernels of the frozen teacher
(csrc/bneck_fused.hip, csrc/head_fused.hip) with SEVERAL TILES PER BLOCK: tests/test_teacher_persistent_gpu.py on the device,
tests/test_teacher_cases_cpu.py for the preconditions.  No device is needed to import or use this module.

Both kernels launch under a grid cap (fpd_set_option("bneck_blocks" / "head_blocks", n); defaults 128 / 160).  A tensor with more
128-pixel tiles than the cap makes a Bottleneck block walk a contiguous RANGE of tiles (the a2 ring, the `incr` branch) and a head
block a STRIDED set of them.  The tables below pair small shapes with small caps; every row names the properties it is there for
and check_bneck_row() / check_pair_row() / check_head_row() verify them on a restatement of the launch arithmetic, so that an
edited table cannot drift back to one tile per block.

Exact inputs (the storage-equality test proves fp32 storage == bf16 storage in the interpreter, bit for bit):
  Bottleneck   as tests/test_exact_gpu.py test_bottleneck_fused_exact: small() activations, sparse_weights(), unit BNs
  head         y0, x: small();  w_fc, w_fc2: sparse_weights() (two non-zeros in {+-1, +-0.5} per output);  w_score, w_score2: two
               non-zeros per output, +-1 ONLY;  biases: small().  Then a = relu(fc + b) is a multiple of 1/4 with |a| <= 3; score a
               multiple of 1/4 with |score| <= 7; next = x + fc_(a) + score_(score) + b + b' a multiple of 1/8 with
               |next| <= 1 + 6 + 14 + 2 = 23, i.e. at most 184 units of 1/8: below 2^8, so every value has a bf16 of its own
               (with +-0.5 allowed in w_score or w_score2 the unit would be 1/16 and 23 * 16 = 368 needs nine bits)."""
import torch
import torch.nn.functional as F

from fpd_amd import graph as G
from oracle import plan_interp as PI
from tests import test_exact_gpu as _ex, test_kernels_gpu as _tk
from tests._exact_inputs import CpuBench, seed  # noqa: F401  (CpuBench: re-exported for the tests)
from tests.test_exact_gpu import small, sparse_weights

HEAD_C, HEAD_J = 256, 16
BNECK_DEFAULT_CAP, HEAD_DEFAULT_CAP = 128, 160


def _bind():
    """make_bn() / unit_bn() build graph.BN through the module global their files bind in setup_module (on a device); the same
    module is bound here, so that the constructions also run without one."""
    for m in (_tk, _ex):
        if m.G is None:
            m.G = G


# ---------------------------------------------------------------------------------------------------------------------
# the launch arithmetic, restated (csrc/conv_dispatch.h fpd_balanced_blocks, csrc/bneck_fused.hip launch_bneck_pair /
# bneck_eval_body, csrc/common.h fpd_cut, csrc/head_fused.hip fpd_head_fused_launch / head_eval_kernel)
def cdiv(a, b):
    return (a + b - 1) // b


def ntiles(N, H, W):
    return cdiv(N * H * W, 128)


def bneck_blocks(tiles, cap):
    return tiles if tiles <= cap else cdiv(tiles, cdiv(tiles, cap))


def bneck_ranges(tiles, nblk):
    """[t_beg, t_end) of every block: fpd_cut(i, n, d) = i * n / d."""
    return [(i * tiles // nblk, (i + 1) * tiles // nblk) for i in range(nblk)]


def pair_split(ta, tb, cap):
    """-> (na, nb): blocks of the two Bottlenecks of a 'bneck2' launch"""
    if ta + tb <= cap:
        return ta, tb
    capb = max(1, cap * tb // (ta + tb))
    nb = bneck_blocks(tb, capb)
    return bneck_blocks(ta, max(1, cap - nb)), nb


def head_blocks(tiles, cap):
    return tiles if tiles <= cap else cdiv(tiles, cdiv(tiles, cap))


def head_walk(tiles, nblk):
    """The tiles every block visits, in order: tile = block, block + nblk, ..., permuted when the tile count is a multiple of 8."""
    perm = (lambda t: (t & 7) * (tiles >> 3) + (t >> 3)) if tiles % 8 == 0 else (lambda t: t)
    return [[perm(t) for t in range(b, tiles, nblk)] for b in range(nblk)]


def bneck_props(N, H, W, cap):
    """The set of property names the launch of a fused Bottleneck on (N, H, W) under `cap` (None: the default) has."""
    tiles = ntiles(N, H, W)
    ranges = bneck_ranges(tiles, bneck_blocks(tiles, BNECK_DEFAULT_CAP if cap is None else cap))
    assert ranges[0][0] == 0 and ranges[-1][1] == tiles and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    whole = 128 % (H * W) == 0
    nrows = 128 // W
    lens = [e - b for b, e in ranges]
    first_row = lambda t: (t * nrows) % H                  # row (within its image) of the tile's first pixel row
    incr = [[(not whole) and t > b and first_row(t) != 0 for t in range(b, e)] for b, e in ranges]
    p = set()
    if min(lens) >= 2:
        p.add('several tiles in every block')
    if cap is None:
        p.add('default cap')
    if len(ranges) == 1:
        p.add('single block')
    if len(set(lens)) > 1:
        p.add('uneven ranges')
    p.add('ntiles % 8 == 0' if tiles % 8 == 0 else 'ntiles % 8 != 0')
    if whole:
        p.add('whole-image tiles')
        if (N * H * W) % 128 != 0 and lens[-1] >= 2:
            p.add('ragged tile ends a multi-tile range')
    else:
        if any(any(i) for i in incr):
            p.add('incr')                                  # halo rows 0 and 1 come from the ring
        if any((t * nrows) % (2 * nrows) != 0 for (b, e), inc in zip(ranges, incr) for t, i in zip(range(b, e), inc) if i):
            p.add('ring wraps')                            # an incremental tile that starts in the second half-slot
        if any(first_row(b) != 0 for b, e in ranges):
            p.add('range starts mid-image')
        if any(first_row(t) == 0 for b, e in ranges for t in range(b + 1, e)):
            p.add('range crosses an image boundary')       # incr must be false there although tile > t_beg
        if all(sum(i) == len(i) - 1 for i in incr) and all((e - b) * 128 * 4 == H * W for b, e in ranges):
            p.add('block = quarter image')
        if H * W == 256:
            p.add('two tiles per image')
            if any(first_row(b) != 0 for b, e in ranges):
                p.add('range starts on the second tile of an image')
    return p


def pair_props(a, b, cap):
    ta, tb = ntiles(*a), ntiles(*b)
    na, nb = pair_split(ta, tb, cap)
    p = set()
    if ta + tb > cap:
        p.add('proportional split')
    if nb == 1 and tb >= 2:
        p.add('b: one block for all its tiles')
    if min(ta // na, tb // nb) >= 2:
        p.add('several tiles in every block')
    if na + nb <= cap:
        p.add('grid within the cap')
    return p


def head_props(N, H, W, cap):
    tiles = ntiles(N, H, W)
    nblk = head_blocks(tiles, HEAD_DEFAULT_CAP if cap is None else cap)
    walk = head_walk(tiles, nblk)
    assert sorted(t for w in walk for t in w) == list(range(tiles))
    lens = [len(w) for w in walk]
    last_valid = N * H * W - (tiles - 1) * 128
    p = set()
    if min(lens) >= 2:
        p.add('several tiles in every block')
    if max(lens) == 1:
        p.add('one tile per block')
    if cap is None:
        p.add('default cap')
    if nblk == 1:
        p.add('single block')
    if len(set(lens)) > 1:
        p.add('uneven strided ranges')
    p.add('permutation' if tiles % 8 == 0 else 'no permutation')
    if last_valid < 128:
        p.add('last tile has %d valid pixels' % last_valid)
        if any(len(w) >= 2 and w[-1] == tiles - 1 for w in walk):
            p.add('ragged tile is not the first of its block')
    return p


# ---------------------------------------------------------------------------------------------------------------------
# case tables: (shape, cap or None = the default, widths P to run or None = both, properties the row is there for)
BNECK_CASES = [
    ((2, 64, 64), 8, None, ['several tiles in every block', 'incr', 'ring wraps', 'block = quarter image', 'ntiles % 8 == 0']),
    ((3, 32, 32), 5, None, ['several tiles in every block', 'incr', 'ring wraps', 'range starts mid-image',
                            'range crosses an image boundary', 'uneven ranges']),
    ((5, 16, 16), 3, None, ['several tiles in every block', 'incr', 'ring wraps', 'two tiles per image',
                            'range starts on the second tile of an image', 'range crosses an image boundary', 'uneven ranges',
                            'ntiles % 8 != 0']),
    ((7, 16, 16), 1, None, ['several tiles in every block', 'single block', 'incr', 'range crosses an image boundary']),
    ((65, 4, 4), 2, None, ['several tiles in every block', 'whole-image tiles', 'ragged tile ends a multi-tile range']),
    ((12, 8, 8), 2, None, ['several tiles in every block', 'whole-image tiles']),
    ((5, 64, 64), None, (128,), ['several tiles in every block', 'default cap', 'incr', 'ring wraps']),
]
# 'bneck2': (shape a, shape b, P, cap, properties)
PAIR_CASES = [
    ((3, 32, 32), (3, 16, 16), 128, 8, ['proportional split', 'b: one block for all its tiles', 'several tiles in every block',
                                        'grid within the cap']),
    ((2, 64, 64), (2, 32, 32), 64, 8, ['proportional split', 'b: one block for all its tiles', 'several tiles in every block',
                                       'grid within the cap']),
]
HEAD_CASES = [
    ((2, 32, 32), 3, ['several tiles in every block', 'permutation', 'uneven strided ranges']),
    ((5, 16, 16), 4, ['several tiles in every block', 'no permutation', 'uneven strided ranges']),
    ((3, 8, 8), 1, ['several tiles in every block', 'single block', 'last tile has 64 valid pixels',
                    'ragged tile is not the first of its block']),
    ((1, 20, 20), 2, ['several tiles in every block', 'last tile has 16 valid pixels', 'ragged tile is not the first of its block']),
    # the shapes of tests/test_kernels_gpu.py test_head_fused: the head had no exact test, even with one tile per block
    ((2, 16, 16), None, ['one tile per block', 'default cap']),
    ((3, 8, 8), None, ['one tile per block', 'default cap', 'last tile has 64 valid pixels']),
    ((1, 64, 64), None, ['one tile per block', 'default cap', 'permutation']),
    ((6, 64, 64), None, ['several tiles in every block', 'default cap', 'permutation']),
]
WIDTHS = (64, 128)


def bneck_params():
    """(shape, cap, P) of every single-Bottleneck launch of the tests"""
    return [(shape, cap, P) for shape, cap, ps, _ in BNECK_CASES for P in (ps or WIDTHS)]


def check_bneck_row(row):
    shape, cap, _, want = row
    have = bneck_props(*shape, cap)
    assert set(want) <= have, 'Bottleneck %r under cap %r lacks %s (has %s)' % (shape, cap, sorted(set(want) - have), sorted(have))


def check_pair_row(row):
    a, b, _, cap, want = row
    have = pair_props(a, b, cap)
    assert set(want) <= have, 'pair %r + %r under cap %r lacks %s (has %s)' % (a, b, cap, sorted(set(want) - have), sorted(have))


def check_head_row(row):
    shape, cap, want = row
    have = head_props(*shape, cap)
    assert set(want) <= have, 'head %r under cap %r lacks %s (has %s)' % (shape, cap, sorted(set(want) - have), sorted(have))


# ---------------------------------------------------------------------------------------------------------------------
# constructions.  exact = True: the dyadic inputs; False: seeded random inputs as in test_bottleneck_fused / test_head_fused
class Case:
    """ops: the op list; members: the 'bneck' / 'head' ops in it; compare: [(label, Act)] outputs to check"""

    def __init__(self):
        self.ops, self.members, self.compare = [], [], []


def _bneck_op(bt, gen, shape, P, exact):
    _bind()
    N, H, W = shape
    C = 2 * P
    rnd, make_bn = _tk.rnd, _tk.make_bn
    if exact:
        x = bt.act((N, H, W, C), small(gen, N, H, W, C), 'x')
        y = bt.act((N, H, W, C), torch.zeros(N, H, W, C), 'y')
        w1 = bt.buf('wlp', (P, 1, 1, C), sparse_weights(gen, P, 1, C))
        w2 = bt.buf('wlp', (P, 3, 3, P), sparse_weights(gen, P, 3, P))
        w3 = bt.buf('wlp', (C, 1, 1, P), sparse_weights(gen, C, 1, P))
        b1, b2, b3 = (bt.buf('param', (n,), small(gen, n)) for n in (P, P, C))
        bns = [_ex.unit_bn(bt, C, 'bn1'), _ex.unit_bn(bt, P, 'bn2'), _ex.unit_bn(bt, P, 'bn3')]
    else:
        x = bt.act((N, H, W, C), rnd(gen, N, H, W, C), 'x')
        y = bt.act((N, H, W, C), torch.zeros(N, H, W, C), 'y')
        w1 = bt.buf('wlp', (P, 1, 1, C), rnd(gen, P, 1, 1, C, scale=(2.0 / C) ** 0.5))
        w2 = bt.buf('wlp', (P, 3, 3, P), rnd(gen, P, 3, 3, P, scale=(2.0 / (9 * P)) ** 0.5))
        w3 = bt.buf('wlp', (C, 1, 1, P), rnd(gen, C, 1, 1, P, scale=(2.0 / P) ** 0.5))
        b1, b2, b3 = (bt.buf('param', (n,), 0.1 * rnd(gen, n)) for n in (P, P, C))
        bns = [make_bn(bt, gen, C, 'eval', 'bn1'), make_bn(bt, gen, P, 'eval', 'bn2'), make_bn(bt, gen, P, 'eval', 'bn3')]
    return G.Op('bneck', x=x, y=y, dims=(N, H, W, C, P), w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, bn1=bns[0], bn2=bns[1], bn3=bns[2])


def _fold(bt, op, n):
    """tables folded once by fpd_bottleneck_fold() / fpd_head_fold() instead of by every block"""
    op.folded = bt.buf('fold', (n,), torch.full((n,), float('nan')))
    return G.Op(op.kind + '_fold', target=op)


def bneck_case(bt, shape, P, fold, exact):
    c = Case()
    op = _bneck_op(bt, seed('tb', shape, P, exact), shape, P, exact)
    c.ops = ([_fold(bt, op, 6 * P + 4 * P)] if fold else []) + [op]
    c.members, c.compare = [op], [('y', op.y)]
    return c


def pair_case(bt, a, b, P, fold, exact):
    c = Case()
    gen = seed('tp', a, b, P, exact)
    subs = [_bneck_op(bt, gen, s, P, exact) for s in (a, b)]
    c.ops = ([_fold(bt, s, 10 * P) for s in subs] if fold else []) + [G.Op('bneck2', a=subs[0], b=subs[1])]
    c.members, c.compare = subs, [('y of a', subs[0].y), ('y of b', subs[1].y)]
    return c


def head_case(bt, shape, has_next, fold, exact):
    _bind()
    N, H, W = shape
    C, J = HEAD_C, HEAD_J
    gen = seed('th', shape, has_next, exact)
    rnd = _tk.rnd
    nx = lambda f: f() if has_next else None              # last stack: no x, next, fc_, score_
    if exact:
        pm1 = lambda K, Cin: sparse_weights(gen, K, 1, Cin).sign()
        y0 = bt.act((N, H, W, C), small(gen, N, H, W, C), 'y0')
        x = nx(lambda: bt.act((N, H, W, C), small(gen, N, H, W, C), 'x'))
        w_fc = bt.buf('wlp', (C, 1, 1, C), sparse_weights(gen, C, 1, C))
        w_sc = bt.buf('wlp', (J, 1, 1, C), pm1(J, C))
        w_fc2 = nx(lambda: bt.buf('wlp', (C, 1, 1, C), sparse_weights(gen, C, 1, C)))
        w_sc2 = nx(lambda: bt.buf('wlp', (C, 1, 1, J), pm1(C, J)))
        b_fc, b_sc = bt.buf('param', (C,), small(gen, C)), bt.buf('param', (J,), small(gen, J))
        b_fc2, b_sc2 = nx(lambda: bt.buf('param', (C,), small(gen, C))), nx(lambda: bt.buf('param', (C,), small(gen, C)))
        bn = _ex.unit_bn(bt, C, 'fcbn')
    else:
        y0 = bt.act((N, H, W, C), rnd(gen, N, H, W, C), 'y0')
        x = nx(lambda: bt.act((N, H, W, C), rnd(gen, N, H, W, C), 'x'))
        w_fc = bt.buf('wlp', (C, 1, 1, C), rnd(gen, C, 1, 1, C, scale=(2.0 / C) ** 0.5))
        w_sc = bt.buf('wlp', (J, 1, 1, C), rnd(gen, J, 1, 1, C, scale=(1.0 / C) ** 0.5))
        w_fc2 = nx(lambda: bt.buf('wlp', (C, 1, 1, C), rnd(gen, C, 1, 1, C, scale=(1.0 / C) ** 0.5)))
        w_sc2 = nx(lambda: bt.buf('wlp', (C, 1, 1, J), rnd(gen, C, 1, 1, J, scale=(1.0 / J) ** 0.5)))
        b_fc, b_sc = bt.buf('param', (C,), 0.1 * rnd(gen, C)), bt.buf('param', (J,), 0.1 * rnd(gen, J))
        b_fc2, b_sc2 = nx(lambda: bt.buf('param', (C,), 0.1 * rnd(gen, C))), nx(lambda: bt.buf('param', (C,), 0.1 * rnd(gen, C)))
        bn = _tk.make_bn(bt, gen, C, 'eval', 'fcbn')
    score = bt.act((N, H, W, J), torch.zeros(N, H, W, J), 'score')
    nxt = nx(lambda: bt.act((N, H, W, C), torch.zeros(N, H, W, C), 'next'))
    op = G.Op('head', y0=y0, x=x, score=score, next=nxt, dims=(N, H, W, C, J), w_fc=w_fc, b_fc=b_fc, w_score=w_sc, b_score=b_sc,
              w_fc2=w_fc2, b_fc2=b_fc2, w_score2=w_sc2, b_score2=b_sc2, bn=bn)
    c = Case()
    c.ops = ([_fold(bt, op, 3 * C + 32)] if fold else []) + [op]
    c.members, c.compare = [op], [('score', score)] + ([('next', nxt)] if has_next else [])
    return c


# ---------------------------------------------------------------------------------------------------------------------
# what the ReLUs of a case see (the interpreter's arithmetic, restated with the intermediates kept)
def _conv(A, v, wbuf, pad):
    wt = A.view(wbuf).float().permute(0, 3, 1, 2)
    return F.conv2d(v.permute(0, 3, 1, 2), wt, None, stride=1, padding=pad).permute(0, 2, 3, 1)


def _pre(A, v, bn, bias):
    scale, shift, _, _ = PI._bn_coef(A, bn)
    if bias is not None:
        shift = torch.addcmul(shift, scale, A.view(bias))
    return torch.addcmul(shift, v, scale)


def relu_inputs(A, op):
    """-> [(label, pre-activation tensor)] of every ReLU of a 'bneck' / 'head' op over the arenas A"""
    rn = lambda v: PI._rnd(A, v.clamp_min(0))
    if op.kind == 'head':
        return [('relu(bn(fc))', _pre(A, _conv(A, PI._act(A, op.y0), op.w_fc, 0), op.bn, op.b_fc))]
    z1 = _pre(A, PI._act(A, op.x), op.bn1, None)
    z2 = _pre(A, _conv(A, rn(z1), op.w1, 0), op.bn2, op.b1)
    z3 = _pre(A, _conv(A, rn(z2), op.w2, 1), op.bn3, op.b2)
    return [('relu(bn1(x))', z1), ('relu(bn2(conv1))', z2), ('relu(bn3(conv2))', z3)]


def clamp_shares(A, c):
    """-> [(label, share of the pre-activations the ReLU clamps (< 0))] over every member op of the case"""
    return [(label, float((z < 0).float().mean())) for op in c.members for label, z in relu_inputs(A, op)]
