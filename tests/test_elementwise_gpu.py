"""The plain elementwise kernels of csrc/elementwise.hip (ew_kernel / ew_body in its ten ops, two storage types, aliased and
non-aliased instantiations; ew_pair_kernel; affsum_kernel) on the MI355X, where tests/test_kernels_gpu.py::test_elementwise_ops
cannot see them go wrong:

* several trips of the grid-stride pixel loop per thread (option "ew_blocks": tests/_ew_cases.py says which launches make >= 3
  trips with a ragged last one; tests/test_ew_cases_cpu.py asserts it), byte-identical to the default grid;
* statistics against EXACT sums (below) instead of a per-pixel tolerance: a dropped or doubled pixel is an error of ~1/npix
  >= 1e-3 of the sum, seven orders above the bound;
* the in-place instantiation (NA = false), byte-identical to the out-of-place run;
* the variants no kernel test launched (no ReLU, eval-mode BN, no statistics, no add / dgamma / dbeta, sums without a store);
* C = 8, 48, 384 and 512 = FPD_MAXC.

Every output tensor is filled with NaN before the run: an element no thread wrote fails Bench.compare's finiteness check.

Bounds of the statistics checks.  The kernels accumulate, per thread and channel, the fp64 sum of addends that are exact in
fp64 (r and r*r of a stored value r: <= 48 significant bits), split it into integer limbs (<= 2^-61 lost per contribution) and
add limbs, which is associative.  Against fp64 sums over the tensor THE GPU STORED ("statistics of the rounded, stored
values") the only errors are the per-thread fp64 accumulation (<= trips * 2^-53 relative to sum |addend|), the limb split and
the reference's own fp64 summation:
    out_stats, and sum dz of bstats:   |got - want| <= 1e-10 * sum |addend| + 1e-10       (about four orders of margin)
    sum dz * xhat of bstats:           |got - want| <= 2^-20 * sum |dz * xhat| + 1e-10
the latter against fp64 sum dz * (x - mean) * invstd with mean / invstd in fp64 from the same input statistics: the kernel
forms xhat in fp32 from fp32 mean and invstd (the roundings of mean, invstd, the subtraction and the product: <= 4 * 2^-24
relative for |mean| <~ |x - mean|; 2^-20 is x4 over that).  dgamma / dbeta of bn_bwd_apply are float32 of the two sums as the
device holds them, bit for bit.  (Measured on the MI355X, every case of this file: the 1e-10 bounds are used to at most 4e-6
of their width -- most sums come out exact --, the 2^-20 bound to at most 0.11.)"""
import functools

import pytest
import torch

from tests import _ew_cases as K
from tests import _ew_merge_ops as M
from tests import test_kernels_gpu as tk
from tests.test_kernels_gpu import RS, TOL, Bench, make_bn, rnd, tensor_stats

pytestmark = pytest.mark.gpu

setup_module = tk.setup_module

EXACT = dict(atol=0, rtol=0)      # ops that only copy or select


def q(dtype, t):
    return t.to(torch.bfloat16).float() if dtype == 1 else t


def nan(shape):
    return torch.full(tuple(shape), float('nan'))


def ew(name, dims, **kw):
    f = dict(x=None, x2=None, dy=None, add=None, y=None, out_stats=None, bstats=None, dgamma=None, dbeta=None, bn=None)
    f.update(kw)
    return tk.G.Op('ew', op=name, dims=tuple(dims), **f)


def joined(limbs):
    """[2 sums][2 limbs][C] int64 -> [2][C] float64, the way the kernels join them (common.h stat_join)."""
    return limbs[:, 0, :].double() * 2.0 ** -20 + limbs[:, 1, :].double() * 2.0 ** -60


class Case:
    """One Bench, one op list, and what to check of it afterwards."""

    def __init__(self, dtype, shape, seed):
        self.dtype, self.shape = dtype, shape
        self.bt = Bench(dtype)
        self.gen = torch.Generator().manual_seed(seed + sum(shape))
        self.ops = []
        self.outs = []        # (label, Act, exact): compared with the interpreter, and byte for byte between runs
        self.ostats = []      # (label, statistics Buf, Act whose stored values it sums)
        self.bsums = []       # (label, statistics Buf, dz: Act (as stored) or CPU tensor, BN input on the storage grid)
        self.grads = []       # (label, dgamma Buf, dbeta Buf, the bstats Buf they are read from)

    # ---- builders ----
    def act(self, shape, val, name):
        return self.bt.act(shape, val, name)

    def out(self, label, shape, exact=False, act=None):
        a = act if act is not None else self.bt.act(shape, nan(shape), label)
        self.outs.append((label, a, exact))
        return a

    def zstats(self, C):
        return self.bt.buf('stats', (RS, 2, C), torch.zeros(RS, 2, C, dtype=torch.float64))

    def train_bn(self, x_val, name, relu=True, like=None):
        """Train-mode BN over x_val ([N,H,W,C], any values: rounded to the storage grid here); like: share that BN's statistics."""
        C = x_val.shape[-1]
        bn = make_bn(self.bt, self.gen, C, 'train', name, relu=relu)
        bn.count = x_val.shape[0] * x_val.shape[1] * x_val.shape[2]
        bn.stats = like.stats if like is not None else self.bt.buf('stats', (RS, 2, C), tensor_stats(q(self.dtype, x_val)))
        return bn

    def apply(self, dims, with_add, name):
        """A bn_bwd_apply with consistent, pre-filled sums (tests/_ew_merge_ops._apply); its y poisoned."""
        op, _ = M._apply(self.bt, self.gen, dims, q(self.dtype, rnd(self.gen, *dims)), with_add, name)
        self.bt.fills.append((op.y.buf, nan(dims)))
        self.grads.append((name, op.dgamma, op.dbeta, op.bstats))
        return op

    # ---- running ----
    def run(self, blocks=0):
        R = tk.R
        prev = R.set_option('ew_blocks', blocks)
        try:
            self.bt.realise().run(self.ops, 0)
        finally:
            R.set_option('ew_blocks', prev)
        g = self.bt.gpu
        self.raw = {}
        for label, a, _ in self.outs:
            v = g.view(a.buf).cpu()
            self.raw[label] = v.view(torch.int16 if v.element_size() == 2 else torch.int32).clone()
        self.limbs = {label: g.view(buf).cpu().sum(0) for label, buf in
                      [(l, b) for l, b, _ in self.ostats] + [(l, b) for l, b, _, _ in self.bsums]}
        # exact references of the statistics: label -> (statistics Buf, want [2][C], sum |addend| [2][C], relative bound of each sum)
        self.sref = {}
        for label, buf, y in self.ostats:
            yd = g.view(y.buf).cpu().double().reshape(-1, y.shape[-1])
            adds = (yd, yd * yd)
            self.sref[label] = (buf, torch.stack([a.sum(0) for a in adds]), torch.stack([a.abs().sum(0) for a in adds]), (1e-10, 1e-10))
        for label, buf, dz, xq in self.bsums:
            C = xq.shape[-1]
            dzd = (g.view(dz.buf).cpu() if isinstance(dz, tk.G.Act) else dz).double().reshape(-1, C)
            xd = xq.double().reshape(-1, C)
            st = tensor_stats(xq)[0]
            mean = st[0] / xd.shape[0]
            invstd = 1.0 / torch.sqrt((st[1] / xd.shape[0] - mean * mean).clamp_min(0) + tk.G.BN_EPS)
            a1, a2 = dzd, dzd * (xd - mean) * invstd
            self.sref[label] = (buf, torch.stack([a1.sum(0), a2.sum(0)]), torch.stack([a1.abs().sum(0), a2.abs().sum(0)]), (1e-10, 2.0 ** -20))
        return self

    # ---- checks ----
    def check_interp(self, only=None):
        for label, a, exact in self.outs:
            if only is None or label in only:
                self.bt.compare(a, label='%s %s' % (label, self.shape), **(EXACT if exact else TOL[self.dtype]))

    def check_stats(self):
        assert self.sref or not (self.ostats or self.bsums)
        for label, (buf, want, mag, rel) in self.sref.items():
            got = self.bt.gpu.stats_read(buf).cpu().sum(0)
            assert torch.isfinite(got).all(), label
            err = (got - want).abs()
            bound = torch.stack([rel[0] * mag[0] + 1e-10, rel[1] * mag[1] + 1e-10])
            print('%s %s dtype %d: max err/bound %.3e (sum 1), %.3e (sum 2)' % (
                label, self.shape, self.dtype, float((err[0] / bound[0]).max()), float((err[1] / bound[1]).max())))
            bad = ~(err <= bound)      # a NaN in the stored tensor makes the reference NaN: that fails too
            assert not bad.any(), '%s %s: %d sums off, worst %.3e against a bound of %.3e (value %.6e)' % (
                label, self.shape, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()), float(want[bad][0]))

    def check_grads(self):
        g = self.bt.gpu
        for label, dg, db, bst in self.grads:
            s = joined(g.view(bst).cpu().sum(0)).float()
            for name, buf, want in (('dgamma', dg, s[1]), ('dbeta', db, s[0])):
                got = g.view(buf).cpu()
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), '%s %s %s: not float32 of the device sums (%d of %d differ)' % (
                    label, self.shape, name, int((got != want).sum()), got.numel())


def build_all(dtype, shape, full):
    """Every op of the elementwise launcher on one shape; full: plus the variants, the four-term affsum and the apply pair."""
    c = Case(dtype, shape, 101)
    bt, gen = c.bt, c.gen
    N, H, W, C = shape
    hs = K.half(shape)
    x_val, xp_val, dy_val = rnd(gen, *shape), M.tie_grid(gen, shape), rnd(gen, *shape)
    c.tie = M.max_tie_fraction(xp_val)
    x, xp, dy = c.act(shape, x_val, 'x'), c.act(shape, xp_val, 'xp'), c.act(shape, dy_val, 'dy')
    lo, dyh = c.act(hs, rnd(gen, *hs), 'lo'), c.act(hs, rnd(gen, *hs), 'dyh')
    acc, acch = c.act(shape, rnd(gen, *shape), 'acc'), c.act(hs, rnd(gen, *hs), 'acch')
    xq = q(dtype, x_val)
    bn = c.train_bn(x_val, 'bn')
    s1, s4, s6, bst = c.zstats(C), c.zstats(C), c.zstats(C), c.zstats(C)
    dg, dbt = bt.buf('grad', (C,), nan((C,))), bt.buf('grad', (C,), nan((C,)))
    y1, y2, y3 = c.out('bnrelu_fwd', shape), c.out('bnrelu_bwd_r', shape), c.out('bn_bwd_apply', shape)
    y4, y5, y6 = c.out('maxpool_fwd', hs, exact=True), c.out('maxpool_bwd', shape), c.out('upadd_fwd', shape)
    y7, y8 = c.out('sumpool', hs), c.out('add', shape)
    y9, y10 = c.out('relu_mask', shape, exact=True), c.out('dilate2', shape, exact=True)
    y11 = c.out('maxpool_bwd without add', shape, exact=True)
    c.ops += [
        ew('bnrelu_fwd', shape, x=x, y=y1, bn=bn, out_stats=s1),
        ew('bnrelu_bwd_r', shape, x=x, dy=dy, y=y2, bn=bn, bstats=bst),
        ew('bn_bwd_apply', shape, x=x, dy=y2, add=acc, y=y3, bn=bn, bstats=bst, dgamma=dg, dbeta=dbt),
        ew('maxpool_fwd', shape, x=xp, y=y4, out_stats=s4),
        ew('maxpool_bwd', shape, x=xp, dy=dyh, add=acc, y=y5),
        ew('upadd_fwd', shape, x=x, x2=lo, y=y6, out_stats=s6),
        ew('sumpool', shape, x=dy, add=acch, y=y7),
        ew('add', shape, x=x, x2=dy, y=y8),
        ew('relu_mask', shape, x=x, dy=dy, y=y9),
        ew('dilate2', shape, x=lo, y=y10),
        ew('maxpool_bwd', shape, x=xp, dy=dyh, y=y11),
    ]
    c.ostats += [('out_stats bnrelu_fwd', s1, y1), ('out_stats maxpool_fwd', s4, y4), ('out_stats upadd_fwd', s6, y6)]
    c.bsums += [('bstats bnrelu_bwd_r', bst, y2, xq)]
    c.grads += [('bn_bwd_apply', dg, dbt, bst)]
    c.variants = []
    if not full:
        return c
    # ---- variants no kernel test launched ----
    n0 = len(c.outs)
    bn_nr = c.train_bn(x_val, 'bn_nr', relu=False, like=bn)
    bn_ev = make_bn(bt, gen, C, 'eval', 'bn_ev')
    bn_ev.count = N * H * W
    sv1, sv2, bst_nr, bst_ns = c.zstats(C), c.zstats(C), c.zstats(C), c.zstats(C)
    v1, v2 = c.out('bnrelu_fwd, no ReLU', shape), c.out('bnrelu_fwd, eval-mode BN', shape)
    v3, v4 = c.out('bnrelu_fwd without statistics', shape), c.out('maxpool_fwd without statistics', hs, exact=True)
    v5, v6 = c.out('upadd_fwd without statistics', shape), c.out('bnrelu_bwd_r, no ReLU', shape, exact=True)
    v7 = c.out('bn_bwd_apply without add, dgamma, dbeta', shape)
    mk_val = rnd(gen, *shape)
    mk = c.act(shape, mk_val, 'mk')
    c.ops += [
        ew('bnrelu_fwd', shape, x=x, y=v1, bn=bn_nr, out_stats=sv1),
        ew('bnrelu_fwd', shape, x=x, y=v2, bn=bn_ev, out_stats=sv2),
        ew('bnrelu_fwd', shape, x=x, y=v3, bn=bn),
        ew('maxpool_fwd', shape, x=xp, y=v4),
        ew('upadd_fwd', shape, x=x, x2=lo, y=v5),
        ew('bnrelu_bwd_r', shape, x=x, dy=dy, y=v6, bn=bn_nr, bstats=bst_nr),
        ew('bn_bwd_apply', shape, x=x, dy=y2, y=v7, bn=bn, bstats=bst),
        ew('bnrelu_bwd_r', shape, x=x, x2=mk, dy=dy, y=None, bn=bn, bstats=bst_ns),      # the two sums only; mask source x2: exact
    ]
    c.ostats += [('out_stats bnrelu_fwd, no ReLU', sv1, v1), ('out_stats bnrelu_fwd, eval-mode BN', sv2, v2)]
    dz_ns = torch.where(q(dtype, mk_val) > 0, q(dtype, dy_val), torch.zeros(1))
    c.bsums += [('bstats bnrelu_bwd_r, no ReLU', bst_nr, v6, xq), ('bstats bnrelu_bwd_r, no store', bst_ns, dz_ns, xq)]
    c.variants = [l for l, _, _ in c.outs[n0:]]
    # ---- affsum: identity + train-BN up x2 + eval-BN up x2 + a plain (eval-BN, ReLU) term, ReLU ----
    x1_val = rnd(gen, *hs) + 0.2
    a0, a1 = c.act(shape, rnd(gen, *shape), 'a0'), c.act(hs, x1_val, 'a1')
    a2, a3 = c.act(hs, rnd(gen, *hs), 'a2'), c.act(shape, rnd(gen, *shape), 'a3')
    b1 = c.train_bn(x1_val, 'b1', relu=False)
    b2, b3 = make_bn(bt, gen, C, 'eval', 'b2', relu=False), make_bn(bt, gen, C, 'eval', 'b3', relu=True)
    ya = c.out('affsum', shape)
    c.ops.append(tk.G.Op('affsum', terms=[(a0, None, 1), (a1, b1, 2), (a2, b2, 2), (a3, b3, 1)], y=ya, relu=True, out_stats=None,
                         dims=shape, extra_in=[a0, a1, a2, a3]))
    # ---- the pair launch: two bn_bwd_apply, full and half resolution ----
    pa, pb = c.apply(shape, True, 'pair.a'), c.apply(hs, False, 'pair.b')
    c.out('pair, full resolution', shape, act=pa.y)
    c.out('pair, half resolution', hs, act=pb.y)
    c.ops.append(tk.G.Op('ew2', a=pa, b=pb))
    return c


def build_inplace(dtype, shape, inplace):
    """Ops whose result goes into one of their inputs (inplace) or, on the same values, into a tensor of its own."""
    c = Case(dtype, shape, 211)
    bt, gen = c.bt, c.gen
    N, H, W, C = shape
    hs = K.half(shape)

    def res(label, src, shp):      # the result tensor of an op: `src` itself, or a poisoned tensor
        return c.out(label, shp, act=src) if inplace else c.out(label, shp)
    # `add` is y (the header's promise for every op that has one)
    ap = c.apply(shape, True, 'apply')
    if inplace:
        ap.y = ap.add
    c.out('bn_bwd_apply', shape, act=ap.y)
    xp_val = M.tie_grid(gen, shape)
    c.tie = M.max_tie_fraction(xp_val)
    xp, dyh = c.act(shape, xp_val, 'xp'), c.act(hs, rnd(gen, *hs), 'dyh')
    acc, g, acch = c.act(shape, rnd(gen, *shape), 'acc'), c.act(shape, rnd(gen, *shape), 'g'), c.act(hs, rnd(gen, *hs), 'acch')
    # x is y (per-pixel ops: a thread reads the element it then writes)
    xa, xb, xu, lo = (c.act(shape, rnd(gen, *shape), 'xa'), c.act(shape, rnd(gen, *shape), 'xb'), c.act(shape, rnd(gen, *shape), 'xu'),
                      c.act(hs, rnd(gen, *hs), 'lo'))
    xn_val = rnd(gen, *shape)
    xn = c.act(shape, xn_val, 'xn')
    bn = c.train_bn(xn_val, 'bn')
    su, sn = c.zstats(C), c.zstats(C)
    yu, yn = res('upadd_fwd, x is y', xu, shape), res('bnrelu_fwd, x is y', xn, shape)
    c.ops += [
        ap,
        ew('maxpool_bwd', shape, x=xp, dy=dyh, add=acc, y=res('maxpool_bwd', acc, shape)),
        ew('sumpool', shape, x=g, add=acch, y=res('sumpool', acch, hs)),
        ew('add', shape, x=xa, x2=xb, y=res('add, x is y', xa, shape)),
        ew('upadd_fwd', shape, x=xu, x2=lo, y=yu, out_stats=su),
        ew('bnrelu_fwd', shape, x=xn, y=yn, bn=bn, out_stats=sn),
    ]
    c.ostats += [('out_stats upadd_fwd', su, yu), ('out_stats bnrelu_fwd', sn, yn)]
    return c


@functools.lru_cache(maxsize=None)
def run_all(dtype, shape, blocks):
    return build_all(dtype, shape, shape == K.MULTI).run(blocks)


@functools.lru_cache(maxsize=None)
def run_out_of_place(dtype, shape):
    return build_inplace(dtype, shape, False).run(0)


def assert_same_bytes(ref, got, what):
    assert list(ref.raw) == list(got.raw)
    for label in ref.raw:
        ne = int((ref.raw[label] != got.raw[label]).sum())
        assert ne == 0, '%s: %d/%d elements of %s differ in their bytes' % (what, ne, ref.raw[label].numel(), label)


def assert_same_stats(ref, got, what):
    """Limb addition is associative; only the grouping of the per-thread fp64 partial sums depends on the grid."""
    assert list(ref.limbs) == list(got.limbs) and len(ref.limbs) > 0
    for label in ref.limbs:
        bound = 1e-10 * ref.sref[label][2] + 1e-10      # sum dz * xhat too: both runs add the same fp32 xhat
        err = (joined(ref.limbs[label]) - joined(got.limbs[label])).abs()
        assert (err <= bound).all(), '%s: %s differs by %.3e between the grids' % (what, label, float(err.max()))


@pytest.mark.parametrize('dtype', K.DTYPES)
@pytest.mark.parametrize('shape', K.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_all_ops_default_grid(shape, dtype):
    """Every op against the interpreter (ops that only copy or select: exactly), statistics against exact sums, dgamma / dbeta
    bit for bit.  One trip per thread (tests/test_ew_cases_cpu.py): arithmetic, idle threads, the ragged last block."""
    c = run_all(dtype, shape, 0)
    assert c.tie > 0.25, 'too few windows with equal maxima: %.3f' % c.tie
    c.check_interp()
    c.check_stats()
    c.check_grads()


@pytest.mark.parametrize('blocks', K.CAPS)
@pytest.mark.parametrize('dtype', K.DTYPES)
def test_multi_trip_equals_default_grid(dtype, blocks):
    """ew_blocks = 1 / 3 on (3, 12, 10, 64): every thread walks several pixels, the last trip is ragged, the pair launch splits
    (b first, a second) over one or three blocks each.  The per-pixel arithmetic does not depend on which block does it."""
    ref, c = run_all(dtype, K.MULTI, 0), run_all(dtype, K.MULTI, blocks)
    c.check_interp()
    c.check_stats()
    c.check_grads()
    what = 'ew_blocks %d against the default grid' % blocks
    assert_same_bytes(ref, c, what)
    assert_same_stats(ref, c, what)


@pytest.mark.parametrize('blocks', [0, 1])
@pytest.mark.parametrize('dtype', K.DTYPES)
@pytest.mark.parametrize('shape', K.INPLACE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_in_place_equals_out_of_place(shape, dtype, blocks):
    """include/fpd_amd.h fpd_ew_t: `add` may alias y; for BNRELU_FWD, UPADD_FWD and ADD so may x.  The host then launches the
    instantiation without __restrict__ (NA = false), which nothing else runs."""
    ref = run_out_of_place(dtype, shape)
    c = build_inplace(dtype, shape, True).run(blocks)
    assert c.tie > 0.25
    for o in c.ops:
        assert o.y.buf is (o.add if o.op in ('bn_bwd_apply', 'maxpool_bwd', 'sumpool') else o.x).buf
    c.check_interp()
    c.check_stats()
    c.check_grads()
    ref.check_interp()
    assert_same_bytes(ref, c, 'in place (ew_blocks %d) against out of place' % blocks)
    assert_same_stats(ref, c, 'in place (ew_blocks %d) against out of place' % blocks)


@pytest.mark.parametrize('dtype', K.DTYPES)
def test_variants(dtype):
    """No ReLU, eval-mode BN, no statistics (the 2048-cap path without an LDS flush), constant mask, no add / dgamma / dbeta,
    sums without a store -- at the default grid; test_multi_trip_equals_default_grid walks them too."""
    c = run_all(dtype, K.MULTI, 0)
    assert len(c.variants) == 7
    c.check_interp(only=c.variants)
    assert {'out_stats bnrelu_fwd, no ReLU', 'out_stats bnrelu_fwd, eval-mode BN', 'bstats bnrelu_bwd_r, no ReLU',
            'bstats bnrelu_bwd_r, no store'} <= set(c.sref)
    c.check_stats()


def test_option_hygiene():
    R = tk.R
    prev = R.set_option('ew_blocks', 7)
    try:
        assert prev == 0                                     # the default
        assert R.set_option('ew_blocks', 2) == 7
        assert R.set_option('ew_blocks', -5) == 2            # ignored ...
        assert R.set_option('ew_blocks', -1) == 2            # ... the value stands
        assert R.set_option('ew_blocks', 0) == 2             # 0 restores the default rule
        assert R.set_option('ew_blocks', -1) == 0
        c = Case(0, (1, 4, 6, 48), 307)                      # and a launch after all that has a grid: every element written
        a, b = c.act(c.shape, rnd(c.gen, *c.shape), 'a'), c.act(c.shape, rnd(c.gen, *c.shape), 'b')
        c.ops.append(ew('add', c.shape, x=a, x2=b, y=c.out('add', c.shape)))
        R.set_option('ew_blocks', -1)
        c.bt.realise().run(c.ops, 0)
        c.check_interp()
    finally:
        R.set_option('ew_blocks', prev)
    assert R.set_option('ew_blocks', -1) == prev
