#!/usr/bin/env python
"""Golden vectors of JointsOHKMMSELoss, produced by the REFERENCE's own lib/core/loss.py:42-84 (imported from
/root/reference) in float64 with autograd.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ohkm.py        (build container only)

Cases: B=3 J=16 8x8 topk 8; B=2 J=17 12x9 topk 1 and 17; each with and without target weights, some weights 0.
torch.topk leaves the order of equal values open, and a selection that hangs on the last bits of L would differ between
fp64, fp32 and bf16: a seed is accepted only if, in every sample, the k-th and (k+1)-th largest per-joint loss differ by
at least 1e-3 relative (checked here, on the CPU, when the fixture is made)."""
import os
import sys

import numpy as np
import torch

REF = '/root/reference/lib'
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
from core.loss import JointsOHKMMSELoss  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GAP = 1e-3


def inputs(seed, b, j, h, w):
    rng = np.random.RandomState(seed)
    out = rng.standard_normal((b, j, h, w)) * rng.uniform(0.2, 1.0, (b, j, 1, 1))      # joints of different difficulty
    tg = rng.uniform(0.0, 1.0, (b, j, h, w))
    wt = rng.uniform(0.3, 1.5, (b, j, 1))
    wt[rng.uniform(size=(b, j, 1)) < 0.2] = 0.0
    # stored as float32 (what the loader delivers); the reference runs on the same values widened to float64
    return out.astype(np.float32), tg.astype(np.float32), wt.astype(np.float32)


def gap_ok(out, tg, wt, use_w, k):
    """relative gap between the k-th and (k+1)-th largest L of every sample >= GAP (k = J: nothing to separate)"""
    b, j = out.shape[:2]
    if k == j:
        return True
    w2 = (wt.astype(np.float64) ** 2) if use_w else np.ones((b, j, 1))
    L = 0.5 * w2[:, :, 0] * ((out.astype(np.float64) - tg) ** 2).reshape(b, j, -1).mean(2)
    s = -np.sort(-L, 1)
    return bool(np.all(s[:, k - 1] - s[:, k] >= GAP * s[:, k - 1]) and np.all(s[:, k - 1] > 0))


def run(out, tg, wt, use_w, k):
    o = torch.tensor(out, dtype=torch.float64, requires_grad=True)
    loss = JointsOHKMMSELoss(use_w, topk=k)(o, torch.tensor(tg, dtype=torch.float64), torch.tensor(wt, dtype=torch.float64))
    loss.backward()
    return np.float64(loss.item()), o.grad.numpy()


def main():
    res = {}
    for name, (b, j, h, w, ks) in {'j16': (3, 16, 8, 8, (8,)), 'j17': (2, 17, 12, 9, (1, 17))}.items():
        seed = 0
        while True:
            out, tg, wt = inputs(seed, b, j, h, w)
            if all(gap_ok(out, tg, wt, use_w, k) for use_w in (True, False) for k in ks):
                break
            seed += 1
        assert all(gap_ok(out, tg, wt, use_w, k) for use_w in (True, False) for k in ks)
        res[name + '/output'], res[name + '/target'], res[name + '/weight'] = out, tg, wt
        res[name + '/seed'], res[name + '/topk'] = np.int64(seed), np.array(ks, np.int64)
        for use_w in (True, False):
            for k in ks:
                loss, grad = run(out, tg, wt, use_w, k)
                key = '%s/w%d/k%d' % (name, int(use_w), k)
                res[key + '/loss'], res[key + '/grad'] = loss, grad
                print(key, 'seed', seed, 'loss', loss)
    np.savez_compressed(os.path.join(HERE, 'ohkm_small.npz'), **res)


if __name__ == '__main__':
    main()
