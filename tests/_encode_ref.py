"""The numpy restatement of DARK's unbiased target encoding (include/fpd_amd.h, fpd_targets_unbiased_t), the reference's
integer-centred form beside it for comparison, and the cases the encode tests share.

`place` restates the per-joint decisions (centre, 3-sigma box corners, outside, weight, drawn) in float64, `unbiased` the
whole launch: float32(exp(float64 expression)) over the whole map.  `biased` is generate_target as fpd_render_targets_w
renders it (centre int(joint / stride + 0.5), the float32 patch pasted clipped).  `within` is the tolerance of the
specification, derived there and not measured.

Unpinned: the DarkPose source is not available to these tests, so everything here equals the written specification, not a
run of the authors' code."""
import numpy as np

# (B, J, H, W, sigma) of the GPU tests
SHAPES = {'E1': (2, 3, 16, 12, 1), 'E2': (2, 5, 20, 28, 2), 'E3': (1, 17, 64, 48, 2), 'E4': (1, 2, 128, 128, 3),
          'E5': (3, 2, 7, 5, 1)}
TINY = 2.0 ** -126                   # float32's smallest normal
ACCURACY_SEED = 20261020             # the seeded centres of the accuracy condition


def trunc(v):
    """Python's int() of float64 values, element-wise (toward zero); saturating beyond +-2^30 like csrc/encode_math.h, so
    that no comparison against a map size changes.  Not defined for NaN (the caller decides `outside` first)."""
    v = np.clip(np.asarray(v, np.float64), -2.0 ** 30, 2.0 ** 30)
    return np.trunc(np.where(np.isnan(v), 0.0, v)).astype(np.int64)


def place(joints, vis, size, stride, sigma, joints_weight=None):
    """joints [B,J,3] float64, vis [B,J] float32, size (W, H), stride (sx, sy) -> dict of mu [B,J,2] float64, ul / br [B,J,2]
    int, outside / drawn [B,J] bool, w / weight [B,J] float32."""
    joints, vis = np.asarray(joints, np.float64), np.asarray(vis, np.float32)
    w_, h_ = size
    tmp = np.float64(3 * sigma)
    mu = np.stack([joints[..., 0] / np.float64(stride[0]), joints[..., 1] / np.float64(stride[1])], -1)
    finite = np.isfinite(mu).all(-1)
    ul, br = trunc(mu - tmp), trunc(mu + tmp + 1.0)
    outside = ~finite | (ul[..., 0] >= w_) | (ul[..., 1] >= h_) | (br[..., 0] < 0) | (br[..., 1] < 0)
    w = np.where(outside, np.float32(0), vis).astype(np.float32)
    weight = w if joints_weight is None else (w * np.asarray(joints_weight, np.float32)[None, :]).astype(np.float32)
    return dict(mu=mu, ul=ul, br=br, outside=outside, w=w, weight=weight, drawn=~outside & (w > np.float32(0.5)))


def exact(mu, size, sigma):
    """The float64 value of every pixel: exp(-((x - mu_x)^2 + (y - mu_y)^2) / (2 sigma^2)) for mu [..., 2] -> [..., H, W]."""
    w_, h_ = size
    x = np.arange(w_, dtype=np.float64)[None, :]
    y = np.arange(h_, dtype=np.float64)[:, None]
    mx, my = mu[..., 0, None, None], mu[..., 1, None, None]
    with np.errstate(under='ignore'):
        return np.exp(-((x - mx) ** 2 + (y - my) ** 2) / (2 * sigma ** 2))


def unbiased(joints, vis, size, stride, sigma, joints_weight=None):
    """-> (target [B,J,H,W] float32, weight [B,J] float32, exact float64 values [B,J,H,W] (0 where nothing is drawn), place)."""
    p = place(joints, vis, size, stride, sigma, joints_weight)
    with np.errstate(invalid='ignore'):
        e = exact(np.where(p['drawn'][..., None], p['mu'], 0.0), size, sigma) * p['drawn'][..., None, None]
    with np.errstate(under='ignore'):
        return e.astype(np.float32), p['weight'], e, p


def biased(joints, vis, size, stride, sigma, joints_weight=None):
    """generate_target of the reference (JointsDataset.py:233-289) as fpd_render_targets_w renders it -> (target, weight)."""
    joints, vis = np.asarray(joints, np.float64), np.asarray(vis, np.float32)
    w_, h_ = size
    b, j = vis.shape
    tmp = 3 * sigma
    n = 2 * tmp + 1
    gx = np.arange(0, n, 1, np.float32)
    g = np.exp(-((gx - n // 2) ** 2 + (gx[:, None] - n // 2) ** 2) / (2 * sigma ** 2))
    target, weight = np.zeros((b, j, h_, w_), np.float32), vis.copy()
    for a in range(b):
        for k in range(j):
            mx, my = int(joints[a, k, 0] / stride[0] + 0.5), int(joints[a, k, 1] / stride[1] + 0.5)
            ul, br = (mx - tmp, my - tmp), (mx + tmp + 1, my + tmp + 1)
            if ul[0] >= w_ or ul[1] >= h_ or br[0] < 0 or br[1] < 0:
                weight[a, k] = 0
                continue
            if weight[a, k] > 0.5:
                x0, x1, y0, y1 = max(0, ul[0]), min(br[0], w_), max(0, ul[1]), min(br[1], h_)
                target[a, k, y0:y1, x0:x1] = g[y0 - ul[1]:y1 - ul[1], x0 - ul[0]:x1 - ul[0]]
    if joints_weight is not None:
        weight = (weight * np.asarray(joints_weight, np.float32)[None, :]).astype(np.float32)
    return target, weight


def within(got, e):
    """(ok, number of values that are not bit-equal to float32(e), worst distance in float32 steps where e is normal, worst
    absolute distance below) of float32 `got` against the float64 values `e` under the tolerance of the specification: one
    float32 step where e >= 2^-126, an absolute 2^-126 below."""
    got = np.ascontiguousarray(got, np.float32)
    with np.errstate(under='ignore'):
        ref = np.ascontiguousarray(e.astype(np.float32))
    normal = e >= TINY
    steps = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))      # positive floats order like their bits
    small = np.abs(got.astype(np.float64) - e)
    ok = bool(np.isfinite(got).all() and (got >= 0).all() and (steps[normal] <= 1).all() and (small[~normal] <= TINY).all())
    return (ok, int((got.view(np.int32) != ref.view(np.int32)).sum()), int(steps[normal].max()) if normal.any() else 0,
            float(small[~normal].max()) if (~normal).any() else 0.0)


def random_case(name, seed=None):
    """(joints [B,J,3] float64, vis [B,J] float32, joints_weight [J] float32, size (W, H), stride, sigma) of shape `name`:
    centres anywhere from 2 tmp left of the map to 2 tmp right of it (so some are outside, some cut by the border),
    visibility in {0, 0.5, 1}, a stride that is no power of two in y."""
    b, j, h, w, sigma = SHAPES[name]
    rng = np.random.RandomState(sum(map(ord, name)) * 977 + h * 131 + w if seed is None else seed)
    stride = (4.0, 3.0)
    tmp = 3 * sigma
    mu = np.stack([rng.uniform(-2 * tmp, w + 2 * tmp, (b, j)), rng.uniform(-2 * tmp, h + 2 * tmp, (b, j))], -1)
    inside = rng.rand(b, j) < 0.6                                  # most centres inside the map, where every pixel matters
    mu = np.where(inside[..., None], np.stack([rng.uniform(0, w - 1, (b, j)), rng.uniform(0, h - 1, (b, j))], -1), mu)
    joints = np.concatenate([mu * np.array(stride), np.zeros((b, j, 1))], -1)
    vis = rng.choice(np.array([0, 0.5, 1, 1, 1], np.float32), (b, j))
    vis[0, 0], joints[0, 0, 0:2] = 1.0, np.array([0.3 * w * stride[0], 0.6 * h * stride[1]])      # at least one map is drawn
    return joints, vis, rng.uniform(0.5, 1.5, j).astype(np.float32), (w, h), stride, sigma


def designed_case(w=12, h=16, sigma=1):
    """(joints [1,J,3], vis [1,J], names, size, stride, sigma): centres on both sides of every guard, in x and in y, each with
    the other coordinate mid-map, and the three visibilities.  stride 1: the joint is the centre, exactly."""
    tmp = 3 * sigma
    rows = []
    for axis, n in (('x', w), ('y', h)):
        for nm, v in (('%s: mu = size + tmp (outside)' % axis, n + tmp), ('%s: mu = size + tmp - 2^-20 (inside)' % axis, n + tmp - 2.0 ** -20),
                      ('%s: mu = -tmp - 2 (outside)' % axis, -tmp - 2.0), ('%s: mu = -tmp - 1.5 (inside under truncation)' % axis, -tmp - 1.5)):
            rows.append((nm, (v, h / 2 + 0.25) if axis == 'x' else (w / 2 - 0.25, v), 1.0))
    for v in (0.0, 0.5, 1.0):
        rows.append(('vis = %g' % v, (w / 2 + 0.3, h / 2 - 0.4), v))
    joints = np.array([[r[1][0], r[1][1], 0.0] for r in rows], np.float64)[None]
    vis = np.array([r[2] for r in rows], np.float32)[None]
    return joints, vis, [r[0] for r in rows], (w, h), (1.0, 1.0), sigma


def designed_expectation(names):
    """(outside, drawn) per designed case, from its name alone."""
    outside = np.array(['(outside)' in n for n in names])
    drawn = np.array([not o and n not in ('vis = 0', 'vis = 0.5') for o, n in zip(outside, names)])
    return outside, drawn


def accuracy_case(size, n=200, seed=ACCURACY_SEED, stride=4.0):
    """n seeded sub-pixel centres in [4, W-5] x [4, H-5] as one [1,n] batch -> (joints, vis, centres [1,n,2])."""
    w, h = size
    rng = np.random.RandomState(seed + 1000 * w + h)
    cen = np.stack([rng.uniform(4, w - 5, (1, n)), rng.uniform(4, h - 5, (1, n))], -1)
    return np.concatenate([cen * stride, np.zeros((1, n, 1))], -1), np.ones((1, n), np.float32), cen
