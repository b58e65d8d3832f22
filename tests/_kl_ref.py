"""CPU restatement (float64 numpy, closed form) of JointsKLDLoss as the fused step evaluates it (include/fpd_amd.h fpd_loss_kl_t).

Per criterion call with maps s, reference maps r, weights w[n,j] and temperature T > 0, over the hw pixels of one map:
    p = softmax(s/T),  q = softmax(r/T)                      (both subtract the row maximum)
    L[n,j] = w[n,j] T^2 sum_x q_x ((r_x - s_x)/T - lse(r/T) + lse(s/T))
    loss   = 1 / (B J) * sum L[n,j]
    dloss/ds_x = w[n,j] T (p_x - q_x) / (B J)
The weight enters once.  q_x == 0 contributes an exact 0; no logarithm of a probability is taken.
All arrays are NCHW ([B,J,H,W]); weights are [B,J].  mse() is the JointsMSELoss term a KL term can be paired with."""
import numpy as np


def _lse_softmax(y):
    """y [R, n] -> (lse [R, 1], softmax [R, n]) with the row maximum subtracted"""
    m = y.max(1, keepdims=True)
    e = np.exp(y - m)
    z = e.sum(1, keepdims=True)
    return m + np.log(z), e / z


def criterion(s, r, w, T):
    """One criterion call -> dict(rows L[n,j] / w (the plain KL of every map, times T^2), loss, grad)."""
    s, r, w = np.asarray(s, np.float64), np.asarray(r, np.float64), np.asarray(w, np.float64)
    if not T > 0:
        raise ValueError('temperature %r is not positive' % (T,))
    B, J, H, W = s.shape
    s2, r2 = s.reshape(B * J, H * W), r.reshape(B * J, H * W)
    ls, p = _lse_softmax(s2 / T)
    lr, q = _lse_softmax(r2 / T)
    with np.errstate(invalid='ignore'):
        term = q * ((r2 - s2) / T - lr + ls)
    term = np.where(q == 0, 0.0, term)           # (0 * finite; spelled out so that an overflowing bracket cannot leak a NaN)
    rows = (T * T * term.sum(1)).reshape(B, J)
    loss = (w * rows).sum() / (B * J)
    grad = (w.reshape(B * J, 1) * T * (p - q) / (B * J)).reshape(B, J, H, W)
    return {'rows': rows, 'loss': loss, 'grad': grad}


def mse(p, r, w):
    """JointsMSELoss (include/fpd_amd.h fpd_loss_t): 0.5/(B J hw) sum w^2 (p - r)^2 -> dict(loss, grad)"""
    p, r, w = np.asarray(p, np.float64), np.asarray(r, np.float64), np.asarray(w, np.float64)
    B, J, H, W = p.shape
    w2 = (w * w)[:, :, None, None]
    d = p - r
    return {'loss': 0.5 * (w2 * d * d).sum() / (B * J * H * W), 'grad': w2 * d / (B * J * H * W)}


def fused(outs, target, teacher, w_pose, w_kd, T_pose, T_kd, alpha, grad_scale=1.0):
    """The fused loss over S stacks: each term MSE (its T None) or KL.  -> dict(pose, kd, grads: S x [B,J,H,W])"""
    grads, pose, kd = [], 0.0, 0.0
    for o in outs:
        a = mse(o, target, w_pose) if T_pose is None else criterion(o, target, w_pose, T_pose)
        b = mse(o, teacher, w_kd) if T_kd is None else criterion(o, teacher, w_kd, T_kd)
        pose += a['loss']
        kd += b['loss']
        grads.append(grad_scale * ((1.0 - alpha) * a['grad'] + alpha * b['grad']))
    return {'pose': pose, 'kd': kd, 'grads': grads}


def torch_composition(s, r, w, T, dtype):
    """The F.kl_div composition of the definition and its autograd, evaluated by torch on the CPU in `dtype`
    -> (loss float, grad float64 numpy [B,J,H,W])"""
    import torch
    import torch.nn.functional as F
    s = torch.as_tensor(np.asarray(s)).to(dtype).requires_grad_(True)
    r, w = torch.as_tensor(np.asarray(r)).to(dtype), torch.as_tensor(np.asarray(w)).to(dtype)
    B, J, H, W = s.shape
    s2, r2 = s.reshape(B * J, H * W), r.reshape(B * J, H * W)
    rows = F.kl_div(F.log_softmax(s2 / T, 1), F.softmax(r2 / T, 1), reduction='none').sum(1)
    loss = T * T * (w.reshape(-1) * rows).sum() / (B * J)
    loss.backward()
    return float(loss.detach().double()), s.grad.double().numpy()
