"""`utils.vis` with the reference's function names (lib/utils/vis.py there), rendered on the device.

The reference downloads the batch and the heat maps, composes the canvases on the host (torchvision.utils.make_grid,
cv2.resize, cv2.applyColorMap, cv2.circle, numpy) and encodes the JPEG inside the loop.  Here the canvases are rendered
from the tensors where they lie (csrc/vis.hip: fpd_vis_minmax, fpd_vis_max_preds, fpd_vis_joints_grid, fpd_vis_heatmap_grid);
only the finished uint8 canvases cross PCIe, and with an AsyncImageWriter the encoding happens on a worker thread: a debug
iteration enqueues launches, one asynchronous copy per canvas into pinned memory and an event, and waits for nothing.

Exact (tests/_vis_ref.py restates vis.py:20-116 on the host): the grid geometry, the normalisation, the bytes, the 4:1 resize,
the float64 blend, the cumulative drawing order.  This project's own definitions, which nothing here can hold against OpenCV:
the two mark shapes (cv2.circle's rasteriser) and the colour table JET_BGR (COLORMAP_JET); see the README.

Heat maps are torch tensors of logical shape [N,J,h,w]: contiguous float32 (the loader's target), or a channels-last view
(`nhwc.permute(0, 3, 1, 2)`) of float32 / bfloat16 -- the merged validation map and a network's last map as they lie."""
import queue
import threading

import numpy as np
import torch

from ... import runtime as R


def _jet_bgr():
    """[256,3] uint8, BGR: c = clip(1.5 - |4t - k|, 0, 1) with k = 3, 2, 1 for r, g, b and t = v / 255; floor(255 c + 0.5)."""
    t = np.arange(256, dtype=np.float64) / 255.0
    chan = [np.clip(1.5 - np.abs(4.0 * t - k), 0.0, 1.0) for k in (1.0, 2.0, 3.0)]           # b, g, r
    return np.floor(255.0 * np.stack(chan, 1) + 0.5).astype(np.uint8)


JET_BGR = _jet_bgr()
_tables = {}


def _table(dev):
    t = _tables.get(dev)
    if t is None:
        t = _tables[dev] = torch.from_numpy(JET_BGR).to(dev)
    return t


def _device_image(batch_image, what):
    if not (torch.is_tensor(batch_image) and batch_image.is_cuda):
        raise R.FpdError('%s renders on the device: batch_image must be a CUDA (ROCm) tensor; there is no CPU path' % what)
    if batch_image.dim() != 4 or batch_image.shape[1] != 3:
        raise R.FpdError('%s: batch_image must be [N,3,H,W], got %s' % (what, tuple(batch_image.shape)))
    return batch_image.detach().float().contiguous()


def _map_form(hm, what):
    """(tensor to keep alive, dtype, layout) of a heat map [N,J,h,w] as the kernels read it."""
    if not (torch.is_tensor(hm) and hm.is_cuda):
        raise R.FpdError('%s renders on the device: the heat maps must be a CUDA (ROCm) tensor; there is no CPU path' % what)
    if hm.dim() != 4:
        raise R.FpdError('%s: heat maps must be [N,J,h,w], got %s' % (what, tuple(hm.shape)))
    hm = hm.detach()
    if hm.dtype == torch.float32 and hm.is_contiguous():
        return hm, R.F32, R.VIS_NCHW
    if hm.dtype in (torch.float32, torch.bfloat16) and hm.permute(0, 2, 3, 1).is_contiguous():
        return hm, (R.F32 if hm.dtype == torch.float32 else R.BF16), R.VIS_NHWC
    return hm.float().contiguous(), R.F32, R.VIS_NCHW


def image_minmax(batch_image):
    """Device float32 [2] = (min, max) of the batch: computed once per iteration, shared by every canvas."""
    x = _device_image(batch_image, 'image_minmax')
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    a = R.VisMinmaxT()
    a.n, a.x, a.out = x.numel(), x.data_ptr(), out.data_ptr()
    R.check(R.lib().fpd_vis_minmax(a, R.current_stream()), 'fpd_vis_minmax')
    return out


def max_preds(batch_heatmaps):
    """core.inference.get_max_preds on the device: (preds [N,J,2] float32 (x, y), maxvals [N,J,1]) device tensors."""
    hm, dtype, layout = _map_form(batch_heatmaps, 'max_preds')
    n, j, h, w = hm.shape
    preds = torch.empty((n, j, 2), dtype=torch.float32, device=hm.device)
    maxvals = torch.empty((n, j, 1), dtype=torch.float32, device=hm.device)
    a = R.VisMaxPredsT()
    a.N, a.J, a.h, a.w, a.dtype, a.layout = n, j, h, w, dtype, layout
    a.hm, a.preds, a.maxvals = hm.data_ptr(), preds.data_ptr(), maxvals.data_ptr()
    R.check(R.lib().fpd_vis_max_preds(a, R.current_stream()), 'fpd_vis_max_preds')
    return preds, maxvals


def grid_shape(n, h, w, nrow=8, padding=2):
    """(GH, GW) of make_grid for n images of h x w."""
    if n == 1:
        return h, w
    xmaps = min(nrow, n)
    ymaps = (n + xmaps - 1) // xmaps
    return (h + padding) * ymaps + padding, (w + padding) * xmaps + padding


def render_image_with_joints(batch_image, batch_joints, batch_joints_vis, nrow=8, padding=2, coord_scale=1.0, minmax=None):
    """The canvas of save_batch_image_with_joints as a device uint8 tensor [GH,GW,3] (enqueued, not waited for)."""
    what = 'save_batch_image_with_joints'
    x = _device_image(batch_image, what)
    n, _, h, w = x.shape
    dev = x.device
    joints = batch_joints if torch.is_tensor(batch_joints) else torch.as_tensor(np.asarray(batch_joints))
    joints = joints.detach().to(dev, non_blocking=True)
    if joints.dtype not in (torch.float32, torch.float64):
        joints = joints.double()
    joints = joints.contiguous()
    vis = batch_joints_vis if torch.is_tensor(batch_joints_vis) else torch.as_tensor(np.asarray(batch_joints_vis))
    vis = vis.detach().to(dev, non_blocking=True)
    if vis.dim() == 3:
        vis = vis[:, :, 0]                                         # the first column decides (vis.py:48)
    vis = vis.float().contiguous()
    if joints.dim() != 3 or joints.shape[0] != n or joints.shape[2] < 2 or tuple(vis.shape) != tuple(joints.shape[:2]):
        raise R.FpdError('%s: joints %s / joints_vis %s do not describe %d images' % (what, tuple(joints.shape), tuple(vis.shape), n))
    if minmax is None:
        minmax = image_minmax(x)
    gh, gw = grid_shape(n, h, w, nrow, padding)
    canvas = torch.empty((gh, gw, 3), dtype=torch.uint8, device=dev)
    a = R.VisJointsGridT()
    a.N, a.H, a.W, a.J, a.nrow, a.padding = n, h, w, joints.shape[1], int(nrow), int(padding)
    a.joints_f64, a.joints_stride, a.coord_scale = int(joints.dtype == torch.float64), joints.shape[2], float(coord_scale)
    a.canvas_bytes = canvas.numel()
    a.image, a.minmax, a.joints, a.vis, a.canvas = x.data_ptr(), minmax.data_ptr(), joints.data_ptr(), vis.data_ptr(), canvas.data_ptr()
    R.check(R.lib().fpd_vis_joints_grid(a, R.current_stream()), 'fpd_vis_joints_grid')
    return canvas


def render_heatmaps(batch_image, batch_heatmaps, normalize=True, minmax=None, preds=None):
    """The canvas of save_batch_heatmaps as a device uint8 tensor [N*h,(J+1)*w,3] (enqueued, not waited for)."""
    what = 'save_batch_heatmaps'
    x = _device_image(batch_image, what)
    hm, dtype, layout = _map_form(batch_heatmaps, what)
    n, j, h, w = hm.shape
    if x.shape[0] != n:
        raise R.FpdError('%s: %d images, %d heat maps' % (what, x.shape[0], n))
    if preds is None:
        preds = max_preds(hm)[0]
    if normalize and minmax is None:
        minmax = image_minmax(x)
    canvas = torch.empty((n * h, (j + 1) * w, 3), dtype=torch.uint8, device=x.device)
    table = _table(x.device)
    a = R.VisHeatmapGridT()
    a.N, a.J, a.h, a.w, a.H, a.W = n, j, h, w, x.shape[2], x.shape[3]
    a.dtype, a.layout, a.normalize, a.canvas_bytes = dtype, layout, int(bool(normalize)), canvas.numel()
    a.image, a.minmax, a.hm = x.data_ptr(), (minmax.data_ptr() if normalize else None), hm.data_ptr()
    a.preds, a.table, a.canvas = preds.data_ptr(), table.data_ptr(), canvas.data_ptr()
    R.check(R.lib().fpd_vis_heatmap_grid(a, R.current_stream()), 'fpd_vis_heatmap_grid')
    return canvas


def write_jpeg(path, canvas):
    """What the worker does with a finished canvas.  The channel reversal makes a viewer show what the file of the
    reference's cv2.imwrite (which takes the channels as B, G, R) would show."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(canvas[:, :, ::-1])).save(path, quality=95)


def save_batch_image_with_joints(batch_image, batch_joints, batch_joints_vis, file_name, nrow=8, padding=2):
    """vis.py:20-51; returns the canvas (numpy uint8 [GH,GW,3]).  batch_joints is not modified."""
    canvas = render_image_with_joints(batch_image, batch_joints, batch_joints_vis, nrow, padding).cpu().numpy()
    write_jpeg(file_name, canvas)
    return canvas


def save_batch_heatmaps(batch_image, batch_heatmaps, file_name, normalize=True):
    """vis.py:54-116; returns the canvas (numpy uint8 [N*h,(J+1)*w,3])."""
    canvas = render_heatmaps(batch_image, batch_heatmaps, normalize).cpu().numpy()
    write_jpeg(file_name, canvas)
    return canvas


class AsyncImageWriter(object):
    """One worker thread and a queue: put(path, canvas, event) returns at once; the worker waits for the job's event (the
    canvas's download), then encodes and writes.  close() joins the worker and re-raises what it raised."""

    def __init__(self):
        self._q = queue.Queue()
        self._error = None
        self._thread = threading.Thread(target=self._work, name='fpd-vis-writer', daemon=True)
        self._thread.start()

    def _work(self):
        while True:
            job = self._q.get()
            if job is None:
                return
            if self._error is not None:
                continue                                           # after a failure: drain, write nothing more
            path, canvas, event = job
            try:
                if event is not None:
                    event.synchronize()
                write_jpeg(path, canvas)
            except BaseException as e:                             # noqa: B902  (handed to close())
                self._error = e

    def put(self, path, canvas, event=None):
        """canvas: numpy uint8 [h,w,3] (for a download in flight: the pinned buffer's array, valid once `event` completes)."""
        if self._thread is None:
            raise R.FpdError('AsyncImageWriter.put after close()')
        self._q.put((path, canvas, event))

    def close(self):
        if self._thread is not None:
            self._q.put(None)
            self._thread.join()
            self._thread = None
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            self.close()
        else:
            try:
                self.close()
            except BaseException:                                  # noqa: B902  (the loop's own exception wins)
                pass
        return False


def _emit(path, canvas, writer):
    """A rendered device canvas -> the file: synchronously, or as a pinned download the writer's thread waits for."""
    if writer is None:
        write_jpeg(path, canvas.cpu().numpy())
        return
    host = torch.empty(canvas.shape, dtype=torch.uint8, pin_memory=True)       # a fresh block per canvas
    host.copy_(canvas, non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    writer.put(path, host.numpy(), event)


def save_debug_images(config, input, meta, target, joints_pred, output, prefix, writer=None):
    """vis.py:119-141: the flag logic and the file names.  joints_pred: predictions in input pixels ([N,J,2+], the
    reference's pred*4), or None = get_max_preds(output) * 4, formed on the device.  With a `writer` (AsyncImageWriter)
    the call only enqueues; without one it returns when the files are written."""
    d = config.DEBUG
    if not d.DEBUG:
        return
    for flag, keys in ((d.SAVE_BATCH_IMAGES_GT, ('joints', 'joints_vis')), (d.SAVE_BATCH_IMAGES_PRED, ('joints_vis',))):
        for key in (keys if flag else ()):
            if meta is None or key not in meta:
                raise R.FpdError("save_debug_images: DEBUG.SAVE_BATCH_IMAGES_GT / SAVE_BATCH_IMAGES_PRED need meta['%s'], which "
                                 'this loader does not deliver (the plain `synthetic` set has no joints; use synthetic_aug, '
                                 'mpii or coco, or switch the two flags off)' % key)
    if not (d.SAVE_BATCH_IMAGES_GT or d.SAVE_BATCH_IMAGES_PRED or d.SAVE_HEATMAPS_GT or d.SAVE_HEATMAPS_PRED):
        return
    minmax = image_minmax(input)
    out_preds = None
    if (d.SAVE_BATCH_IMAGES_PRED and joints_pred is None) or d.SAVE_HEATMAPS_PRED:
        out_preds = max_preds(output)[0]
    if d.SAVE_BATCH_IMAGES_GT:
        _emit('{}_gt.jpg'.format(prefix), render_image_with_joints(input, meta['joints'], meta['joints_vis'], minmax=minmax), writer)
    if d.SAVE_BATCH_IMAGES_PRED:
        if joints_pred is None:
            c = render_image_with_joints(input, out_preds, meta['joints_vis'], coord_scale=4.0, minmax=minmax)
        else:
            c = render_image_with_joints(input, joints_pred, meta['joints_vis'], minmax=minmax)
        _emit('{}_pred.jpg'.format(prefix), c, writer)
    if d.SAVE_HEATMAPS_GT:
        _emit('{}_hm_gt.jpg'.format(prefix), render_heatmaps(input, target, minmax=minmax), writer)
    if d.SAVE_HEATMAPS_PRED:
        _emit('{}_hm_pred.jpg'.format(prefix), render_heatmaps(input, output, minmax=minmax, preds=out_preds), writer)
