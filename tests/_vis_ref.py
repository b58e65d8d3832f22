"""Host restatement of the reference's lib/utils/vis.py:20-116 in numpy / torch-CPU, statement by statement, under the
definitions this project pins where the reference calls torchvision and OpenCV (include/fpd_amd.h, README "Unpinned"):

  make_grid    torchvision of the reference's era: norm_ip over the whole batch (add_(-min).div_(max - min + 1e-5)), the
               grid filled with pad_value 0, a single image returned bare
  cv2.resize   INTER_LINEAR at exactly 4:1 on uint8: (a + b + c + d + 2) >> 2 over the four centre pixels of each 4x4 block
  cv2.circle   radius 2, thickness 2: the pixels 1 <= dx^2 + dy^2 <= 9; radius 1, thickness 1: dx^2 + dy^2 == 1; clipped
  COLORMAP_JET the piecewise-linear table JET_BGR below

The canvases are the arrays the reference hands to cv2.imwrite.  Nothing here imports the package under test."""
import math

import numpy as np
import torch


def jet_bgr():
    out = np.zeros((256, 3), np.uint8)
    for v in range(256):
        t = v / 255.0
        r = min(max(1.5 - abs(4.0 * t - 3.0), 0.0), 1.0)
        g = min(max(1.5 - abs(4.0 * t - 2.0), 0.0), 1.0)
        b = min(max(1.5 - abs(4.0 * t - 1.0), 0.0), 1.0)
        out[v] = [math.floor(255.0 * b + 0.5), math.floor(255.0 * g + 0.5), math.floor(255.0 * r + 0.5)]
    return out


JET_BGR = jet_bgr()


def get_max_preds(batch_heatmaps):
    """lib/core/inference.py:18-46."""
    batch_size, num_joints, width = batch_heatmaps.shape[0], batch_heatmaps.shape[1], batch_heatmaps.shape[3]
    heatmaps_reshaped = batch_heatmaps.reshape((batch_size, num_joints, -1))
    idx = np.argmax(heatmaps_reshaped, 2)
    maxvals = np.amax(heatmaps_reshaped, 2)
    maxvals = maxvals.reshape((batch_size, num_joints, 1))
    idx = idx.reshape((batch_size, num_joints, 1))
    preds = np.tile(idx, (1, 1, 2)).astype(np.float32)
    preds[:, :, 0] = (preds[:, :, 0]) % width
    preds[:, :, 1] = np.floor((preds[:, :, 1]) / width)
    pred_mask = np.tile(np.greater(maxvals, 0.0), (1, 1, 2))
    pred_mask = pred_mask.astype(np.float32)
    preds *= pred_mask
    return preds, maxvals


def norm_ip(img, mn, mx):
    """torchvision.utils.make_grid's norm_ip (and vis.py:66): in place on a float32 tensor, Python-float scalars."""
    img.clamp_(min=mn, max=mx)
    img.add_(-mn)
    # div_ by a Python scalar: a true IEEE float32 division by float32(max - min + 1e-5)
    d = torch.tensor(mx - mn + 1e-5, dtype=torch.float64).to(torch.float32)
    img.copy_(torch.from_numpy(img.numpy() / d.numpy()))
    return img


def make_grid(tensor, nrow=8, padding=2, normalize=False):
    """torchvision.utils.make_grid(tensor, nrow, padding, normalize) with range None, scale_each False, pad_value 0."""
    if normalize:
        tensor = tensor.clone()
        norm_ip(tensor, float(tensor.min()), float(tensor.max()))
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((3, height * ymaps + padding, width * xmaps + padding), 0)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k = k + 1
    return grid


def circle(img, center, radius, color, thickness):
    """cv2.circle(img, center, radius, color, thickness) under the two pinned shapes; in place, clipped to img."""
    lo, hi = {(2, 2): (1, 9), (1, 1): (1, 1)}[(radius, thickness)]
    cx, cy = center
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            if lo <= dx * dx + dy * dy <= hi and 0 <= cy + dy < img.shape[0] and 0 <= cx + dx < img.shape[1]:
                img[cy + dy, cx + dx] = color


def resize4(image, size):
    """cv2.resize(image, (w, h)) for an image of exactly (4h, 4w): INTER_LINEAR's fixed-point result."""
    w, h = size
    assert image.shape[0] == 4 * h and image.shape[1] == 4 * w and image.dtype == np.uint8
    a = image.astype(np.int32)
    s = a[1::4, 1::4] + a[1::4, 2::4] + a[2::4, 1::4] + a[2::4, 2::4]
    return ((s + 2) >> 2).astype(np.uint8)


def apply_color_map(heatmap):
    return JET_BGR[heatmap]


def save_batch_image_with_joints(batch_image, batch_joints, batch_joints_vis, nrow=8, padding=2):
    """vis.py:20-51 up to the file write.  batch_joints / batch_joints_vis: numpy; the in-place edit of the joints
    (vis.py:46-47) is made on a copy."""
    grid = make_grid(batch_image, nrow, padding, True)
    ndarr = grid.mul(255).clamp(0, 255).byte().permute(1, 2, 0).cpu().numpy()
    ndarr = ndarr.copy()

    nmaps = batch_image.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height = int(batch_image.size(2) + padding)
    width = int(batch_image.size(3) + padding)
    batch_joints = np.array(batch_joints, dtype=np.float64)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            joints = batch_joints[k]
            joints_vis = batch_joints_vis[k]
            for joint, joint_vis in zip(joints, joints_vis):
                joint[0] = x * width + padding + joint[0]
                joint[1] = y * height + padding + joint[1]
                if np.ravel(joint_vis)[0]:
                    circle(ndarr, (int(joint[0]), int(joint[1])), 2, [255, 0, 0], 2)
            k = k + 1
    return ndarr


def save_batch_heatmaps(batch_image, batch_heatmaps, normalize=True):
    """vis.py:54-116 up to the file write; batch_heatmaps: float32 torch-CPU [N,J,h,w]."""
    if normalize:
        batch_image = batch_image.clone()
        min = float(batch_image.min())
        max = float(batch_image.max())
        norm_ip(batch_image, min, max)

    batch_size = batch_heatmaps.size(0)
    num_joints = batch_heatmaps.size(1)
    heatmap_height = batch_heatmaps.size(2)
    heatmap_width = batch_heatmaps.size(3)

    grid_image = np.zeros((batch_size * heatmap_height, (num_joints + 1) * heatmap_width, 3), dtype=np.uint8)

    preds, maxvals = get_max_preds(batch_heatmaps.detach().cpu().numpy())

    for i in range(batch_size):
        image = batch_image[i].mul(255).clamp(0, 255).byte().permute(1, 2, 0).cpu().numpy()
        heatmaps = batch_heatmaps[i].mul(255).clamp(0, 255).byte().cpu().numpy()

        resized_image = resize4(image, (int(heatmap_width), int(heatmap_height)))

        height_begin = heatmap_height * i
        height_end = heatmap_height * (i + 1)
        for j in range(num_joints):
            circle(resized_image, (int(preds[i][j][0]), int(preds[i][j][1])), 1, [0, 0, 255], 1)
            heatmap = heatmaps[j, :, :]
            colored_heatmap = apply_color_map(heatmap)
            masked_image = colored_heatmap * 0.7 + resized_image * 0.3
            circle(masked_image, (int(preds[i][j][0]), int(preds[i][j][1])), 1, [0, 0, 255], 1)

            width_begin = heatmap_width * (j + 1)
            width_end = heatmap_width * (j + 2)
            grid_image[height_begin:height_end, width_begin:width_end, :] = masked_image

        grid_image[height_begin:height_end, 0:heatmap_width, :] = resized_image

    return grid_image
