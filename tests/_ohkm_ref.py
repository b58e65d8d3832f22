"""CPU restatement (float64 numpy) of JointsOHKMMSELoss as the fused step evaluates it (include/fpd_amd.h fpd_loss_ohkm_t).

Per criterion call with maps p, reference maps r and weights w[n,j]:
    rows[n,j] = w[n,j]^2 * sum_x (p - r)^2            (what launch 1 of csrc/loss_ohkm.hip accumulates)
    L[n,j]    = 0.5 / HW * rows[n,j]
    sel(n)    = the k joints with the largest L[n,:]; among equal L the LOWER joint index wins
    loss      = 1 / (B k) * sum_n sum_{j in sel(n)} L[n,j]
    dloss/dp  = [j in sel(n)] * w^2 (p - r) / (B k HW)
All arrays are NCHW ([B,J,H,W]); weights are [B,J]."""
import numpy as np


def select(rows, k):
    """bool [B,J]: the k largest of every row, ties to the lower index."""
    B, J = rows.shape
    if not 1 <= k <= J:
        raise ValueError('topk %d outside [1, %d]' % (k, J))
    sel = np.zeros((B, J), bool)
    for n in range(B):
        order = sorted(range(J), key=lambda j: (-rows[n, j], j))
        sel[n, order[:k]] = True
    return sel


def mask_words(sel):
    """uint32 [B]: bit j = joint j kept."""
    return (sel.astype(np.uint64) << np.arange(sel.shape[1], dtype=np.uint64)[None, :]).sum(1).astype(np.uint32)


def criterion(p, r, w, k):
    """One criterion call -> dict(rows, sel, loss, grad); k = J is JointsMSELoss."""
    p, r, w = np.asarray(p, np.float64), np.asarray(r, np.float64), np.asarray(w, np.float64)
    B, J, H, W = p.shape
    w2 = (w * w)[:, :, None, None]
    d = p - r
    rows = (w2 * d * d).reshape(B, J, -1).sum(2)
    sel = select(rows, k)
    loss = (0.5 / (H * W) * rows)[sel].sum() / (B * k)
    grad = sel[:, :, None, None] * w2 * d / (B * k * H * W)
    return {'rows': rows, 'sel': sel, 'loss': loss, 'grad': grad}


def fused(outs, target, teacher, w_pose, w_kd, k_pose, k_kd, alpha, grad_scale=1.0):
    """The fused loss over S stacks (lib/core/function.py:128-134 of the reference with OHKM criteria): selection per
    (stack, term, sample).  -> dict(rows [S,2,B,J], masks uint32 [S,2,B], pose, kd, grads: S x [B,J,H,W])."""
    rows, masks, grads, pose, kd = [], [], [], 0.0, 0.0
    for p in outs:
        a = criterion(p, target, w_pose, k_pose)
        b = criterion(p, teacher, w_kd, k_kd)
        rows.append(np.stack([a['rows'], b['rows']]))
        masks.append(np.stack([mask_words(a['sel']), mask_words(b['sel'])]))
        pose += a['loss']
        kd += b['loss']
        grads.append(grad_scale * ((1.0 - alpha) * a['grad'] + alpha * b['grad']))
    return {'rows': np.stack(rows), 'masks': np.stack(masks), 'pose': pose, 'kd': kd, 'grads': grads}
