"""numpy restatement of the augmentation half of `JointsDataset.__getitem__` (/root/reference/lib/dataset/JointsDataset.py:
137-181, half_body_transform :65-108, utils/transforms.py:32-110), shared by the CPU and GPU augmentation tests, plus the
inputs of the cases pinned in tests/golden/augment_ref.npz (written by tests/golden/make_golden_augment.py from the
reference's own __getitem__).

Every intermediate has the dtype numpy (>= 2) gives it in the reference; the cases where promotion decides:
  * half_body_transform: float32 scalar `op` Python float / int stays float32 (aspect_ratio, 1.0, 1.5, pixel_std)
  * `s * np.clip(...)`: np.clip of a Python float is a numpy float64 scalar, so a float32 scale becomes float64
  * `width - c[0] - 1` is float32 when c is float32 (half-body centre, COCO boxes)
  * `scale * 200.0` stays float32 for a float32 scale (validation mode with COCO boxes)
  * `center + src_dir` is float64 (src_dir is a list of float64), rounded when stored into the float32 point array
"""
import numpy as np

from oracle import infer_ref

IMAGE_SIZE, HEATMAP_SIZE, SIGMA = (48, 64), (12, 16), 2
ASPECT = IMAGE_SIZE[0] * 1.0 / IMAGE_SIZE[1]
DRAWS = ('u_half', 'n_half', 'n_scale', 'n_rot', 'u_rot', 'u_flip')
MPII_PAIRS = [[0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13]]
MPII_UPPER = (7, 8, 9, 10, 11, 12, 13, 14, 15)
COCO_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
COCO_UPPER = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
COCO_WEIGHT = np.array([1., 1., 1., 1., 1., 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5], np.float32)

# group -> dataset configuration.  seed: chosen so that every sample meets the two preconditions (check_preconditions)
GROUPS = {
    'coco_train': dict(J=17, train=True, seed=0, weight=True, sf=0.25, rf=30, prob_half=0.3, num_half=2, flip=True),
    'mpii_train': dict(J=16, train=True, seed=24, weight=False, sf=0.35, rf=40.0, prob_half=0.3, num_half=2, flip=True),
    'coco_valid': dict(J=17, train=False, seed=0, weight=True, sf=0.25, rf=30, prob_half=0.3, num_half=2, flip=True),
    'mpii_valid': dict(J=16, train=False, seed=0, weight=False, sf=0.25, rf=30, prob_half=0.3, num_half=2, flip=True),
}

# one recipe per sample of a training group: draw overrides + how the annotations are bent
TRAIN_RECIPES = [
    dict(),                                                                       # rotation on, no flip, no half-body
    dict(u_flip=0.2),                                                             # flip
    dict(u_half=0.1, n_half=-0.3, u_flip=0.4, shape=(300, 420)),                  # half-body upper + flip, largest image
    dict(u_half=0.1, n_half=1.2, layout='wide'),                                  # half-body lower, w > ar*h
    dict(u_half=0.1, n_half=1.2, layout='tall', keep_lower=2),                    # <= 2 lower joints: falls back to upper; w < ar*h
    dict(u_half=0.1, n_half=0.1, keep_lower=2, keep_upper=1),                     # 1 upper joint selected: rejected, c and s kept
    dict(u_rot=0.7, n_scale=4.0, far_joint=True, shape=(61, 97)),                 # rotation gate off, scale clipped high,
                                                                                  # a visible joint whose patch misses the map
    dict(n_scale=-4.0, n_rot=3.0),                                                # scale clipped low, rotation clipped high
    dict(n_rot=-3.0, u_flip=0.5, drop=(0, 3, 8, 12)),                             # rotation clipped low, flip at the gate's
                                                                                  # edge (<= 0.5), invisible joints
    dict(u_half=0.1, keep_lower=1, keep_upper=1),                                 # 2 visible <= num_half: half-body not entered
]
VALID_RECIPES = [dict(), dict(shape=(61, 97), drop=(1, 5)), dict(shape=(300, 420), far_joint=True), dict(layout='wide')]


def tables(J):
    return (COCO_PAIRS, COCO_UPPER) if J == 17 else (MPII_PAIRS, MPII_UPPER)


def box2cs(x, y, w, h, dtype):
    """coco.py:223-242."""
    center = np.zeros((2,), dtype=dtype)
    center[0], center[1] = x + w * 0.5, y + h * 0.5
    if w > ASPECT * h:
        h = w * 1.0 / ASPECT
    elif w < ASPECT * h:
        w = h * ASPECT
    return center, np.array([w * 1.0 / 200, h * 1.0 / 200], dtype=dtype) * 1.25


def group_inputs(name, seed=None):
    """The inputs of one group: dict of shapes [B,2] (h, w), joints [B,J,3] f64, vis [B,J] f64, center / scale [B,2] (float32
    for 17 joints like coco.py, float64 for 16 like mpii.py), draws [B,6] f64."""
    g = GROUPS[name]
    J = g['J']
    rng = np.random.RandomState(1000 + (g['seed'] if seed is None else seed) * 7 + J)
    recipes = TRAIN_RECIPES if g['train'] else VALID_RECIPES
    dtype = np.float32 if J == 17 else np.float64
    upper = tables(J)[1]
    B = len(recipes)
    out = dict(shapes=np.zeros((B, 2), np.int64), joints=np.zeros((B, J, 3)), vis=np.zeros((B, J)),
               center=np.zeros((B, 2), dtype), scale=np.zeros((B, 2), dtype), draws=np.zeros((B, 6)))
    for i, rc in enumerate(recipes):
        h, w = rc.get('shape', (int(rng.randint(61, 301)), int(rng.randint(97, 421))))
        bw, bh = rng.uniform(0.4, 0.7) * w, rng.uniform(0.5, 0.8) * h
        bx, by = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
        u = rng.uniform(0.05, 0.95, (J, 2))
        if rc.get('layout') == 'wide':
            u[:, 1] = 0.45 + 0.1 * u[:, 1]
        if rc.get('layout') == 'tall':
            u[:, 0] = 0.45 + 0.1 * u[:, 0]
        xy = np.array([bx, by]) + u * np.array([bw, bh])
        v = np.ones(J)
        for k in rc.get('drop', ()):
            v[k] = 0
        for key, want_upper in (('keep_lower', False), ('keep_upper', True)):
            if key in rc:
                ids = [k for k in range(J) if (k in upper) == want_upper]
                for k in ids[rc[key]:]:
                    v[k] = 0
        if rc.get('far_joint'):
            far = max(k for k in range(J) if v[k] > 0)
            xy[far] = [w - 1.5 if bx + bw * 0.5 < w * 0.5 else 1.5, by + 0.5 * bh]
            bw, bx = 0.3 * bw, (bx if bx + bw * 0.5 < w * 0.5 else bx + 0.7 * bw)     # a narrow box on the other side
        out['shapes'][i] = (h, w)
        out['joints'][i, :, 0:2] = xy * v[:, None]
        out['vis'][i] = v
        out['center'][i], out['scale'][i] = box2cs(bx, by, bw, bh, dtype)
        d = dict(u_half=0.9, n_half=0.0, n_scale=float(rng.standard_normal()), n_rot=float(rng.standard_normal()),
                 u_rot=0.3, u_flip=0.9)
        d.update({k: rc[k] for k in DRAWS if k in rc})
        out['draws'][i] = [d[k] for k in DRAWS]
    return out


# ---- the restatement ----
def half_body(joints, vis, upper_ids, n_half):
    """JointsDataset.py:65-108 -> (center f32 [2], scale f32 [2]) or None."""
    sel_u = [joints[k] for k in range(len(vis)) if vis[k] > 0 and k in upper_ids]
    sel_l = [joints[k] for k in range(len(vis)) if vis[k] > 0 and k not in upper_ids]
    sel = sel_u if (n_half < 0.5 and len(sel_u) > 2) else (sel_l if len(sel_l) > 2 else sel_u)
    if len(sel) < 2:
        return None
    sel = np.array(sel, dtype=np.float32)
    acc = np.zeros(3, np.float32)
    for row in sel:                                    # sequential float32 sum in joint order
        acc = acc + row
    center = (acc.astype(np.float64) / len(sel)).astype(np.float32)[:2]
    lt, rb = sel.min(axis=0), sel.max(axis=0)
    w, h = rb[0] - lt[0], rb[1] - lt[1]
    ar = np.float32(ASPECT)
    if w > ar * h:
        h = w * np.float32(1.0) / ar
    elif w < ar * h:
        w = h * ar
    scale = np.array([w * np.float32(1.0) / np.float32(200), h * np.float32(1.0) / np.float32(200)], np.float32)
    return center, scale * np.float32(1.5)


def solve3(src, dst):
    """cv::getAffineTransform: the 6x6 system of the three point pairs, float64."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    a, b = np.zeros((6, 6)), np.zeros(6)
    for i in range(3):
        a[i, 0:2], a[i, 2] = src[i], 1
        a[i + 3, 3:5], a[i + 3, 5] = src[i], 1
        b[i], b[i + 3] = dst[i, 0], dst[i, 1]
    return np.linalg.solve(a, b).reshape(2, 3)


def affine(c, s, r, out_size=IMAGE_SIZE):
    """transforms.py:57-89; c, s arrays in the dtype they have at the call, r float64 degrees."""
    st = s * np.float32(200.0) if s.dtype == np.float32 else s * 200.0
    src_w = st[0]
    rad = np.pi * float(r) / 180
    sn, cs = np.sin(rad), np.cos(rad)
    up = np.float64(src_w) * -0.5
    d = np.array([0 * cs - up * sn, 0 * sn + up * cs])
    dw, dh = float(out_size[0]), float(out_size[1])
    src, dst = np.zeros((3, 2), np.float32), np.zeros((3, 2), np.float32)
    src[0] = c.astype(np.float64)
    src[1] = c.astype(np.float64) + d
    dst[0] = [dw * 0.5, dh * 0.5]
    dst[1] = np.array([dw * 0.5, dh * 0.5]) + np.array([0, dw * -0.5], np.float32)
    for p in (src, dst):
        e = p[0] - p[1]
        p[2] = p[1] + np.array([-e[1], e[0]], np.float32)
    return solve3(src, dst)


def augment(inp, i, g):
    """Sample i of a group -> dict(center, scale, rotation, flipped, trans, joints [J,3], vis [J])."""
    J = g['J']
    pairs, upper = tables(J)
    joints, vis = inp['joints'][i].copy(), inp['vis'][i].copy()
    c, s = inp['center'][i].copy(), inp['scale'][i].copy()
    width = int(inp['shapes'][i, 1])
    d = dict(zip(DRAWS, inp['draws'][i]))
    r, flipped = 0.0, 0
    if g['train']:
        if vis.sum() > g['num_half'] and d['u_half'] < g['prob_half']:
            hb = half_body(joints, vis, upper, d['n_half'])
            if hb is not None:
                c, s = hb
        sf, rf = g['sf'], g['rf']
        s = s.astype(np.float64) * min(max(d['n_scale'] * sf + 1, 1 - sf), 1 + sf)
        r = min(max(d['n_rot'] * rf, -rf * 2), rf * 2) if d['u_rot'] <= 0.6 else 0.0
        if g['flip'] and d['u_flip'] <= 0.5:
            flipped = 1
            joints[:, 0] = width - joints[:, 0] - 1
            for a, b in pairs:
                joints[[a, b]] = joints[[b, a]]
                vis[[a, b]] = vis[[b, a]]
            joints = joints * vis[:, None]
            c[0] = (np.float32(width) - c[0]) - np.float32(1) if c.dtype == np.float32 else width - c[0] - 1
    trans = affine(c, s, r)
    for k in range(J):
        if vis[k] > 0.0:
            joints[k, 0:2] = np.dot(trans, np.array([joints[k, 0], joints[k, 1], 1.]))
    joints[:, 2] = 0
    return dict(center=c.astype(np.float64), scale=s.astype(np.float64), rotation=float(r), flipped=flipped, trans=trans,
                joints=joints, vis=vis)


def targets(joints, vis, weight):
    """generate_target (JointsDataset.py:233-289) -> target [J,h,w] f32, target_weight [J,1] f32."""
    jv = np.stack([vis, vis, np.zeros_like(vis)], -1)
    tg, tw = infer_ref.generate_target(joints, jv, np.array(IMAGE_SIZE), np.array(HEATMAP_SIZE), SIGMA)
    if weight is not None:
        tw = np.multiply(tw, weight.reshape(-1, 1))
    return tg, tw.astype(np.float32)


def group_weight(g):
    return COCO_WEIGHT if g['weight'] else None


def check_preconditions(joints, vis, trans):
    """Conditions on the inputs (not tolerances) that make the integer decisions downstream independent of last-place
    differences in `trans`: (1) the value int(joint / stride + 0.5) truncates lies >= 1e-3 from an integer, for visible
    joints; (2) every argument of cvRound in the crop's coordinate terms lies >= 1e-6 from a half-integer.  -> the two
    smallest distances."""
    stride = np.array(IMAGE_SIZE) / np.array(HEATMAP_SIZE)
    v = (joints[:, 0:2] / stride + 0.5)[vis > 0]
    d1 = np.abs(v - np.rint(v)).min() if v.size else 1.0
    m = infer_ref.invert_affine(trans)
    xs, ys = np.arange(IMAGE_SIZE[0], dtype=np.float64), np.arange(IMAGE_SIZE[1], dtype=np.float64)
    args = np.concatenate([m[0, 0] * xs * 1024, m[1, 0] * xs * 1024, (m[0, 1] * ys + m[0, 2]) * 1024, (m[1, 1] * ys + m[1, 2]) * 1024])
    d2 = np.abs(args - np.floor(args) - 0.5).min()
    return d1, d2


def scene(seed, h, w):
    """A deterministic uint8 [h,w,3] test image: low-frequency waves plus per-pixel noise (the crop tests compare bit for
    bit, so the content only has to vary everywhere)."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 80 * np.sin(0.031 * (c + 1) * x + 0.017 * (3 - c) * y + c) for c in range(3)], -1)
    return np.clip(img + rng.randint(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)
