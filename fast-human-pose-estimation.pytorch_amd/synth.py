"""Synthetic MPII/COCO-shaped batches for benchmarking and smoke tests (there is no dataset on the box).

Same recipe as SURVEY.md section 8(d): N(0,1) "ImageNet-normalised" crops, J joints uniform in the image,
Bernoulli(0.85) visibility, un-normalised sigma=2 Gaussian heat-map targets rendered the way
/root/reference/lib/dataset/JointsDataset.py:233-289 (generate_target) does: centre int(x/stride+0.5),
(6*sigma+1)^2 patch clipped at the border, weight 0 when the patch is fully outside."""
import numpy as np
import torch


def gaussian_targets(xy, vis, image_size, heatmap_size, sigma):
    """xy [B,J,2] pixels, vis [B,J] -> target [B,J,h,w] f32, target_weight [B,J,1] f32."""
    B, J = vis.shape
    wh, hh = heatmap_size
    rad = 3 * sigma
    size = 2 * rad + 1
    ax = np.arange(size, dtype=np.float32) - rad
    patch = np.exp(-(ax[None, :] ** 2 + ax[:, None] ** 2) / (2.0 * sigma ** 2)).astype(np.float32)
    target = np.zeros((B, J, hh, wh), np.float32)
    weight = vis.astype(np.float32).copy()
    mu_x = (xy[..., 0] / (image_size[0] / wh) + 0.5).astype(np.int64)
    mu_y = (xy[..., 1] / (image_size[1] / hh) + 0.5).astype(np.int64)
    for b in range(B):
        for j in range(J):
            x0, y0 = mu_x[b, j] - rad, mu_y[b, j] - rad
            x1, y1 = x0 + size, y0 + size
            if x0 >= wh or y0 >= hh or x1 < 0 or y1 < 0:
                weight[b, j] = 0.0
                continue
            if weight[b, j] <= 0.5:
                continue
            cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, wh), min(y1, hh)
            target[b, j, cy0:cy1, cx0:cx1] = patch[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
    return target, weight[..., None]


def make_batch(seed, batch, num_joints, image_size=(256, 256), heatmap_size=(64, 64), sigma=2, p_vis=0.85):
    """(input [B,3,H,W], target [B,J,h,w], target_weight [B,J,1]) as CPU float tensors."""
    rng = np.random.RandomState(seed)
    w, h = image_size
    inp = rng.standard_normal((batch, 3, h, w)).astype(np.float32)
    xy = np.stack([rng.uniform(0, w, (batch, num_joints)), rng.uniform(0, h, (batch, num_joints))], -1)
    vis = (rng.uniform(0, 1, (batch, num_joints)) < p_vis).astype(np.float32)
    tg, tw = gaussian_targets(xy, vis, image_size, heatmap_size, sigma)
    return torch.from_numpy(inp), torch.from_numpy(tg), torch.from_numpy(tw)


# ---- scenes for the on-device augmentation pipeline (lib/dataset/device_dataset.py) ----
MPII_FLIP_PAIRS = [[0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13]]                                   # mpii.py:32
MPII_UPPER_BODY = (7, 8, 9, 10, 11, 12, 13, 14, 15)                                                        # mpii.py:35
COCO_FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]                  # coco.py:93-94
COCO_UPPER_BODY = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)                                                       # coco.py:96
COCO_JOINTS_WEIGHT = (1., 1., 1., 1., 1., 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5)          # coco.py:99-104


def skeleton(num_joints):
    """(flip_pairs, upper_body_ids, joints_weight or None): MPII's tables for 16 joints, COCO's for 17."""
    if num_joints == 16:
        return MPII_FLIP_PAIRS, MPII_UPPER_BODY, None
    if num_joints == 17:
        return COCO_FLIP_PAIRS, COCO_UPPER_BODY, np.array(COCO_JOINTS_WEIGHT, np.float32)
    return [], tuple(range(num_joints // 2)), None


def box2cs(x, y, w, h, aspect_ratio, dtype=np.float32, pixel_std=200):
    """coco.py:223-242 (_box2cs / _xywh2cs): box -> (center, scale), the box grown to the aspect ratio, then by 1.25."""
    center = np.zeros((2,), dtype=dtype)
    center[0] = x + w * 0.5
    center[1] = y + h * 0.5
    if w > aspect_ratio * h:
        h = w * 1.0 / aspect_ratio
    elif w < aspect_ratio * h:
        w = h * aspect_ratio
    scale = np.array([w * 1.0 / pixel_std, h * 1.0 / pixel_std], dtype=dtype)
    if center[0] != -1:
        scale = scale * 1.25
    return center, scale


def scene_image(rng, h, w, joints=None, vis=None, radius=4):
    """uint8 [h,w,3]: a smooth background (one low-frequency wave per channel) plus a disc per visible joint."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.empty((h, w, 3), np.float32)
    for c in range(3):
        fx, fy, ph = rng.uniform(0.005, 0.03, 2).tolist() + [rng.uniform(0, 6.28)]
        img[..., c] = 128 + 90 * np.sin(fx * x + fy * y + ph)
    if joints is not None:
        for k in range(joints.shape[0]):
            if vis[k] <= 0:
                continue
            cx, cy = int(round(joints[k, 0])), int(round(joints[k, 1]))
            x0, x1, y0, y1 = max(cx - radius, 0), min(cx + radius + 1, w), max(cy - radius, 0), min(cy + radius + 1, h)
            if x0 >= x1 or y0 >= y1:
                continue
            m = (x[y0:y1, x0:x1] - cx) ** 2 + (y[y0:y1, x0:x1] - cy) ** 2 <= radius ** 2
            col = np.array([(37 * k) % 256, (91 * k + 60) % 256, (153 * k + 120) % 256], np.float32)
            img[y0:y1, x0:x1][m] = col
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def make_scenes(seed, n, num_joints, size=(240, 400), aspect_ratio=1.0, p_vis=0.85):
    """n seeded scenes: uint8 images with height and width uniform in `size`, J joints inside a person box, visibility
    Bernoulli(p_vis), centre / scale of the joints' bounding box by _box2cs (float32 like COCO's for 17 joints, float64
    like MPII's otherwise).  -> dict with the keyword arguments of DeviceJointsDB."""
    rng = np.random.RandomState(seed)
    flip_pairs, upper, jw = skeleton(num_joints)
    dtype = np.float32 if num_joints == 17 else np.float64
    images, joints, vis = [], np.zeros((n, num_joints, 3)), np.zeros((n, num_joints, 3))
    center, scale = np.zeros((n, 2), dtype), np.zeros((n, 2), dtype)
    for i in range(n):
        h, w = (int(v) for v in rng.randint(size[0], size[1] + 1, 2))
        bw, bh = rng.uniform(0.35, 0.8) * w, rng.uniform(0.5, 0.9) * h
        bx, by = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
        joints[i, :, 0] = bx + rng.uniform(0, 1, num_joints) * bw
        joints[i, :, 1] = by + rng.uniform(0, 1, num_joints) * bh
        v = (rng.uniform(0, 1, num_joints) < p_vis).astype(np.float64)
        vis[i, :, 0] = vis[i, :, 1] = v
        joints[i, :, 0:2] *= v[:, None]                       # unannotated joints sit at the origin (coco.py:200-208)
        center[i], scale[i] = box2cs(bx, by, bw, bh, aspect_ratio, dtype)
        images.append(scene_image(rng, h, w, joints[i], v))
    return dict(images=images, joints=joints, joints_vis=vis, center=center, scale=scale, flip_pairs=flip_pairs,
                upper_body_ids=upper, aspect_ratio=aspect_ratio, joints_weight=jw)
