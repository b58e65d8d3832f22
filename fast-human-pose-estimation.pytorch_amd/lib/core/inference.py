"""`core.inference` with the reference's function names (/root/reference/lib/core/inference.py), evaluated on the device.

get_final_preds(config, batch_heatmaps, center, scale) -> (preds [N,J,2], maxvals [N,J,1]) numpy arrays like the
reference (its caller stores them into numpy result arrays, function.py:264-270); `batch_heatmaps` is a CUDA tensor
[N,J,h,w] (a numpy array is uploaded).  One kernel does the arg-max, the TEST.POST_PROCESS quarter-pixel shift and the
affine map back to image coordinates (csrc/infer.hip); the per-sample 2x3 matrices are host numpy
(utils.transforms.get_affine_transform, a dozen flops each).

With TEST.DARK (not in the reference) the quarter-pixel shift gives way to distribution-aware coordinate decoding
(Zhang et al., CVPR 2020): a Gaussian blur of TEST.BLUR_KERNEL taps and one Newton step of the log heat map at the
arg-max, again one kernel (csrc/dark.hip); TEST.POST_PROCESS then has no effect."""
import numpy as np
import torch

from ... import runtime as R
from ..utils.transforms import get_affine_transform
from .evaluate import get_max_preds  # noqa: F401  (same name as the reference's core.inference.get_max_preds)


def dark_ksize(dark):
    """The blur size of a `dark` argument as an int: 0 = off, else odd in [9, 31] (smaller sizes are fixed tables in OpenCV)."""
    if dark is None or dark is False:
        return 0
    k = int(dark)
    if isinstance(dark, bool) or k != dark:
        raise R.FpdError('DARK decoding: the blur size is an integer (TEST.BLUR_KERNEL), got %r' % (dark,))
    if k == 0:
        return 0
    if k % 2 == 0 or not R.DARK_MIN_KSIZE <= k <= R.DARK_MAX_KSIZE:
        raise R.FpdError('DARK decoding: TEST.BLUR_KERNEL = %d is not odd in [%d, %d]' % (k, R.DARK_MIN_KSIZE, R.DARK_MAX_KSIZE))
    return k


def dark_taps(ksize):
    """OpenCV's getGaussianKernel(ksize, 0) for ksize > 7 in float64: sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8."""
    k = dark_ksize(ksize)
    if k == 0:
        raise R.FpdError('DARK decoding: no taps for blur size 0')
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    t = np.exp(-0.5 / (sigma * sigma) * (np.arange(k, dtype=np.float64) - (k - 1) / 2) ** 2)
    return t / t.sum()


def dark_config(config):
    """The `dark` argument a config asks for: TEST.BLUR_KERNEL where TEST.DARK is on, else 0 (configs without the keys: off)."""
    t = config.TEST
    key = (lambda name, default: t.get(name, default)) if isinstance(t, dict) else (lambda name, default: getattr(t, name, default))
    if not key('DARK', False):
        return 0
    k = dark_ksize(key('BLUR_KERNEL', 11))
    if k == 0:
        raise R.FpdError('TEST.DARK needs TEST.BLUR_KERNEL odd in [%d, %d], got 0' % (R.DARK_MIN_KSIZE, R.DARK_MAX_KSIZE))
    return k


def dark_taps_device(ksize, device):
    return torch.from_numpy(dark_taps(ksize)).to(device)


def final_preds_device(batch_heatmaps, trans, post_process, dark=0):
    """(coords, preds, maxvals) CUDA tensors.  trans: [N,2,3] float64 CUDA tensor or None (heat-map coordinates only).
    dark: blur size of the DARK decoding, which then replaces the quarter-pixel shift (0: off)."""
    hm = batch_heatmaps
    if not hm.is_cuda:
        raise R.FpdError('get_final_preds works on CUDA (ROCm) tensors; there is no CPU path')
    dark = dark_ksize(dark)
    hm = hm.detach().float().contiguous()
    n, j, h, w = hm.shape
    dev = hm.device
    coords = torch.empty((n, j, 2), dtype=torch.float32, device=dev)
    maxvals = torch.empty((n, j, 1), dtype=torch.float32, device=dev)
    preds = torch.empty((n, j, 2), dtype=torch.float32, device=dev) if trans is not None else None
    if trans is not None:
        assert trans.dtype == torch.float64 and tuple(trans.shape) == (n, 2, 3) and trans.is_cuda
        trans = trans.contiguous()
    if dark:
        taps = dark_taps_device(dark, dev)
        a = R.DarkT()
        a.N, a.J, a.H, a.W, a.layout, a.ksize = n, j, h, w, R.DARK_NCHW, dark
        a.hm, a.taps, a.coords, a.maxvals = hm.data_ptr(), taps.data_ptr(), coords.data_ptr(), maxvals.data_ptr()
        if trans is not None:
            a.trans, a.preds = trans.data_ptr(), preds.data_ptr()
        R.check(R.lib().fpd_dark_refine(a, R.current_stream()), 'fpd_dark_refine')
        return coords, preds, maxvals
    a = R.FinalPredsT()
    a.N, a.J, a.H, a.W, a.post_process = n, j, h, w, int(bool(post_process))
    a.hm, a.coords, a.maxvals = hm.data_ptr(), coords.data_ptr(), maxvals.data_ptr()
    if trans is not None:
        a.trans, a.preds = trans.data_ptr(), preds.data_ptr()
    R.check(R.lib().fpd_final_preds(a, R.current_stream()), 'fpd_final_preds')
    return coords, preds, maxvals


def get_final_preds(config, batch_heatmaps, center, scale):
    """inference.py:49-79."""
    hm = batch_heatmaps if torch.is_tensor(batch_heatmaps) else torch.from_numpy(np.ascontiguousarray(batch_heatmaps)).cuda()
    n, _, h, w = hm.shape
    center, scale = np.asarray(center), np.asarray(scale)
    trans = np.stack([get_affine_transform(center[i], scale[i], 0, [w, h], inv=1) for i in range(n)])
    _, preds, maxvals = final_preds_device(hm, torch.from_numpy(trans).to(hm.device), config.TEST.POST_PROCESS, dark_config(config))
    return preds.cpu().numpy(), maxvals.cpu().numpy()
