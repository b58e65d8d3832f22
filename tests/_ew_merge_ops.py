"""Op lists of the two groups executor.Lowering.plan_ew_merge fuses (include/fpd_amd.h fpd_ew_merge_t), built on
tests/test_kernels_gpu.Bench like tests/_fold_ops.py, and a runner that lowers a list with or without the pass.

pattern 1: [apply pair (full || half resolution) or a lone half-resolution apply, maxpool_bwd]
pattern 2: [apply, sumpool]"""
import torch


def tie_grid(gen, shape):
    """Multiples of 0.5 in [-2, 2] with a heavy boundary (a clipped, rounded normal): equal maxima inside a 2x2 window are frequent."""
    return torch.clamp(torch.round(torch.randn(*shape, generator=gen) * 6.0) / 2.0, -2.0, 2.0)


def max_tie_fraction(x):
    """Share of the (window, channel) pairs of x [N,H,W,C] whose maximum is attained more than once."""
    n, h, w, c = x.shape
    win = x.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    return float(((win == win.max(1, keepdim=True).values).sum(1) >= 2).float().mean())


def _apply(bt, gen, dims, u_val, with_add, name):
    """A 'bn_bwd_apply' over the BN input u_val (already on the storage grid) with consistent statistics and sums."""
    from tests import test_kernels_gpu as tk
    G, RS, rnd, make_bn, tensor_stats = tk.G, tk.RS, tk.rnd, tk.make_bn, tk.tensor_stats
    q = (lambda t: t.to(torch.bfloat16).float()) if bt.dtype == 1 else (lambda t: t)
    N, H, W, C = dims
    u = bt.act(dims, u_val, name + '.u')
    uq = q(u_val)
    g_val = q(rnd(gen, *dims, scale=0.1))
    g = bt.act(dims, g_val, name + '.g')
    add = bt.act(dims, rnd(gen, *dims), name + '.add') if with_add else None
    bn = make_bn(bt, gen, C, 'train', name=name)
    bn.count = N * H * W
    bn.stats = bt.buf('stats', (RS, 2, C), tensor_stats(uq))
    mean, var = uq.double().mean((0, 1, 2)), uq.double().var((0, 1, 2), unbiased=False)
    xhat = (uq.double() - mean) / torch.sqrt(var + G.BN_EPS)
    sums = torch.zeros(RS, 2, C, dtype=torch.float64)
    sums[0, 0], sums[0, 1] = g_val.double().sum((0, 1, 2)), (g_val.double() * xhat).sum((0, 1, 2))
    bst = bt.buf('stats', (RS, 2, C), sums)
    dgam, dbet = bt.buf('grad', (C,), torch.zeros(C)), bt.buf('grad', (C,), torch.zeros(C))
    y = bt.act(dims, None, name + '.y')
    op = G.Op('ew', op='bn_bwd_apply', dims=dims, x=u, x2=None, dy=g, add=add, y=y, out_stats=None, bstats=bst,
              dgamma=dgam, dbeta=dbet, bn=bn)
    return op, u


def pool_bwd_ops(bt, gen, shape, has_full=True, add_full=True, add_half=True):
    """-> (ops, output buffers, buffers only the un-merged launches write, x value).  has_full False: the lone half-resolution apply; add_full then says whether the pool backward
    has an (ordinary) `add`."""
    from tests import test_kernels_gpu as tk
    G, rnd = tk.G, tk.rnd
    N, H, W, C = shape
    half = (N, H // 2, W // 2, C)
    x_val = tie_grid(gen, shape)
    b, _ = _apply(bt, gen, half, rnd(gen, *half), add_half, 'b')
    y = bt.act(shape, None, 'y')
    if has_full:
        a, x = _apply(bt, gen, shape, x_val, add_full, 'a')
        first, padd = G.Op('ew2', a=a, b=b), a.y
    else:
        a, x = None, bt.act(shape, x_val, 'x')
        first, padd = b, (bt.act(shape, rnd(gen, *shape), 'acc') if add_full else None)
    pool = G.Op('ew', op='maxpool_bwd', dims=shape, x=x, x2=None, dy=b.y, add=padd, y=y, out_stats=None, bstats=None,
                dgamma=None, dbeta=None, bn=None)
    outs = [y.buf] + [t for m in (a, b) if m is not None for t in (m.dgamma, m.dbeta)]
    hidden = [m.y.buf for m in (a, b) if m is not None]      # written only by the un-merged launches
    return [first, pool], outs, hidden, x_val


def sumpool_ops(bt, gen, shape, add_low=True, add_apply=True):
    from tests import test_kernels_gpu as tk
    G, rnd = tk.G, tk.rnd
    N, H, W, C = shape
    half = (N, H // 2, W // 2, C)
    ap, _ = _apply(bt, gen, shape, rnd(gen, *shape), add_apply, 'ap')
    low = bt.act(half, rnd(gen, *half), 'low') if add_low else None
    y = bt.act(half, None, 'ylow')
    pool = G.Op('ew', op='sumpool', dims=shape, x=ap.y, x2=None, dy=None, add=low, y=y, out_stats=None, bstats=None,
                dgamma=None, dbeta=None, bn=None)
    return [ap, pool], [ap.y.buf, y.buf, ap.dgamma, ap.dbeta], [], None


def run_gpu(bt, ops, outs, hidden, merge, blocks=None):
    """Lower `ops` (with the merge pass or as today's launches), poison the outputs with NaN, run once; -> (number of merged
    launches, raw copies of the outputs)."""
    from tests import test_kernels_gpu as tk
    E, R = tk.E, tk.R
    for top in ops:
        for m in ((top.a, top.b) if top.kind == 'ew2' else (top,)):
            for k in ('ewm_kind', 'ewm_full', 'ewm_half', 'ewm_absorbed'):
                m.__dict__.pop(k, None)
    prev = R.set_option('ew_merge', 1 if merge else 0)
    prev_b = R.set_option('ew_merge_blocks', blocks) if blocks else None
    try:
        low = E.Lowering(bt.gpu, bt.dtype)
        if merge:
            low.plan_ew_merge(ops)
        lowered = [low.op(o) for o in ops]
        plan = R.Plan()
        for code, st in lowered:
            plan.add(code, st)
        for b in outs + hidden:
            bt.gpu.view(b).fill_(float('nan'))
        plan.run(0, len(plan))
        torch.cuda.synchronize()
    finally:
        R.set_option('ew_merge', prev)
        if blocks:
            R.set_option('ew_merge_blocks', prev_b)
    raw = [bt.gpu.view(b).clone().view(torch.int16 if bt.gpu.view(b).element_size() == 2 else torch.int32) for b in outs]
    return sum(1 for c, _ in lowered if c == R.OP_EW_MERGE), raw
