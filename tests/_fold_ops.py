"""Op list of a 'data gradient behind a BN-backward apply' (shared by test_kernels_gpu.py and test_dispatch_gpu.py): the
forward convolution u = conv(a(x)), C -> K, followed by a train-mode BN on u.  Backward: the apply of that BN turns the
masked gradient g into du; the data gradient of the convolution reads du (ReLU mask + sums of the BN in front of it, a(x));
the weight gradient reads x and du.  fold / fuse attach the apply and the weight gradient to the data gradient, as
graph.HourglassGraph does (the lowering then decides, by asking the library, whether the launch takes them)."""
import numpy as np
import torch


def bn_backward_dgrad_ops(bt, gen, N, H, W, C, K, Rr, bias, fold=True, fuse=None):
    """-> (ops, handles).  ops = [wprep, apply, data gradient, weight gradient]; fuse defaults to 1x1."""
    from tests import test_kernels_gpu as tk
    G, RS, rnd, make_bn, tensor_stats = tk.G, tk.RS, tk.rnd, tk.make_bn, tk.tensor_stats
    pad = (Rr - 1) // 2
    x_val = rnd(gen, N, H, W, C)
    x = bt.act((N, H, W, C), x_val, 'x')                  # forward input of the convolution (pre BN+ReLU)
    u_val = rnd(gen, N, H, W, K)
    u = bt.act((N, H, W, K), u_val, 'u')                  # its output = input of the next BN
    g_val = rnd(gen, N, H, W, K, scale=0.1)
    g = bt.act((N, H, W, K), g_val, 'g')                  # masked gradient that reached that BN
    wm = bt.buf('param', (K, Rr, Rr, C), rnd(gen, K, Rr, Rr, C, scale=1.0 / np.sqrt(C * Rr * Rr)))
    wb = bt.buf('wlp', (C, Rr, Rr, K))
    du = bt.act((N, H, W, K), None, 'du')
    dz = bt.act((N, H, W, C), None, 'dz')
    bn = make_bn(bt, gen, C, 'train')                     # BN in front of the convolution (mask + sums of the data gradient)
    bn.count = N * H * W
    bn.stats = bt.buf('stats', (RS, 2, C), tensor_stats(x_val.to(torch.bfloat16).float()))
    bn2 = make_bn(bt, gen, K, 'train')                    # the BN whose backward is folded
    bn2.count = N * H * W
    bn2.stats = bt.buf('stats', (RS, 2, K), tensor_stats(u_val.to(torch.bfloat16).float()))
    gq, uq = g_val.to(torch.bfloat16).float(), u_val.to(torch.bfloat16).float()
    mean, var = uq.mean((0, 1, 2)), uq.var((0, 1, 2), unbiased=False)
    xhat = (uq - mean) / torch.sqrt(var + 1e-5)
    sums = torch.zeros(RS, 2, K, dtype=torch.float64)
    sums[0, 0], sums[0, 1] = gq.double().sum((0, 1, 2)), (gq.double() * xhat.double()).sum((0, 1, 2))
    bst2 = bt.buf('stats', (RS, 2, K), sums)
    dgam, dbet = bt.buf('grad', (K,), torch.zeros(K)), bt.buf('grad', (K,), torch.zeros(K))
    bst = bt.buf('stats', (RS, 2, C), torch.zeros(RS, 2, C, dtype=torch.float64))
    dw = bt.buf('grad', (K, Rr, Rr, C), torch.zeros(K, Rr, Rr, C))
    db = bt.buf('grad', (K,), torch.zeros(K)) if bias else None
    ap = G.Op('ew', op='bn_bwd_apply', dims=(N, H, W, K), x=u, x2=None, dy=g, add=None, y=du, out_stats=None, bstats=bst2,
              dgamma=dgam, dbeta=dbet, bn=bn2)
    wg = G.Op('wgrad', x=x, dy=du, dw=dw, dbias=db, bn=bn, dims=(N, H, W, C, K, Rr, Rr, 1, pad, H, W))
    dg = G.Op('conv', x=du, w=wb, wkey='w', bias=None, bkey=None, residual=None, y=dz, out_stats=None, bn=None,
              epi='bnrelu_bwd', epi_x=x, epi_bn=bn, epi_stats=bst, dims=(N, H, W, K, C, Rr, Rr, 1, Rr - 1 - pad, H, W))
    if fold:
        dg.fold_apply, dg.fold_wgrad = ap, wg
    if fuse if fuse is not None else Rr == 1:
        dg.fused_wgrad = wg
    wprep = G.Op('wprep', entries=[{'w': wm, 'w_fwd': None, 'w_bwd': wb}])
    ops = [wprep, ap, dg, wg]
    return ops, dict(wprep=wprep, ap=ap, dg=dg, wg=wg, dz=dz, du=du, bst=bst, dgam=dgam, dbet=dbet, dw=dw, db=db)
