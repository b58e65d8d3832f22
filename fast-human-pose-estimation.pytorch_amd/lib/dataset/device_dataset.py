"""`JointsDataset.__getitem__` after the image is decoded (/root/reference/lib/dataset/JointsDataset.py:137-198), on the
device and per batch: half-body crop, scale / rotation jitter, horizontal flip with left/right exchange,
get_affine_transform, the crop (cv2.warpAffine + ToTensor + Normalize), the joint transform and generate_target.

  DeviceJointsDB        the dataset, resident on the device: decoded 8-bit images of any size packed into one buffer with
                        a table of {pointer, h, w, row_bytes}, the annotations, and the per-dataset tables.  Samples may
                        share an image (image_index), and the images may be streamed in from a loader (load)
  DeviceAugmentLoader   an iterable over batches.  Per batch the host draws the random numbers of the whole batch in one
                        vectorised call into a pinned staging buffer, copies it to the device and enqueues three kernels
                        (csrc/data.hip: augment_params, warp_affine_aug, render_targets_w; with MODEL.TARGET_TYPE
                        gaussian_unbiased the third is render_targets_unbiased).  There is no loop over samples
                        and nothing waits for the device.  With world_size > 1 it yields this rank's share of
                        the epoch: partition 'strided' (epoch_order, training and the default) or 'block' (block_range:
                        validation, every row exactly once across the ranks)

The draw table has one row per sample: the six numbers the reference pulls from np.random / random in its order of use
(include/fpd_amd.h fpd_augment_t): u_half, n_half, n_scale, n_rot, u_rot, u_flip.  u_* are uniform [0,1), n_* standard
normal (half_body_transform really compares a randn() with 0.5)."""
import ctypes as C

import numpy as np
import torch

from ... import runtime as R
from ... import synth
from ..utils.transforms import channel_sources
from .device_pipeline import gaussian_patch, render_targets_unbiased, unbiased_targets

DRAW_COLUMNS = ('u_half', 'n_half', 'n_scale', 'n_rot', 'u_rot', 'u_flip')
DEFAULT_CHUNK_BYTES = 256 << 20          # the pinned staging block of a streamed upload


class DeviceJointsDB:
    def __init__(self, images, joints, joints_vis, center, scale, flip_pairs, upper_body_ids, aspect_ratio,
                 joints_weight=None, device='cuda', pixel_std=200, image_index=None, load=None,
                 chunk_bytes=DEFAULT_CHUNK_BYTES, scores=None):
        """images: list of uint8 [h,w,3] arrays (decoded, channel order is the caller's); joints [N,J,3] and
        joints_vis [N,J,3] or [N,J] as in db_rec['joints_3d'] / ['joints_3d_vis']; center, scale [N,2] in the dtype the
        dataset computes them in (MPII float64, COCO float32: the dtype decides numpy's arithmetic on them, the values
        are stored as float64, which holds both exactly); joints_weight [J] or None.

        image_index [N] (None: sample i owns image i): the image of every sample, for datasets with several people per
        image -- each image is stored once and the table rows of its samples point at the same pixels.

        load (None: `images` holds the arrays): a callable i -> uint8 [h,w,3] array; `images` then holds the (h, w) of
        every image and the pixels are streamed to the device in image order through one pinned staging block of at most
        chunk_bytes, without a host copy of the dataset (an image may span blocks).

        scores [N] (None: every sample scores 1): the detector's score of every sample's box (COCO validation from detection
        boxes); validation batches carry it as meta['score'].

        Either way the pixels must fit into the device memory that is free now: FpdError otherwise, there is no
        host-resident mode."""
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise R.FpdError('DeviceJointsDB lives on a CUDA (ROCm) device; there is no CPU path')
        n_images = len(images)
        if image_index is None:
            image_index = np.arange(n_images)
        image_index = np.ascontiguousarray(image_index, np.int64).reshape(-1)
        if image_index.size and not (0 <= image_index.min() and image_index.max() < n_images):
            raise R.FpdError('DeviceJointsDB: image_index must lie in [0, %d)' % n_images)
        n = len(image_index)
        joints = np.asarray(joints, np.float64)
        vis = np.asarray(joints_vis)
        vis = np.ascontiguousarray(vis[..., 0] if vis.ndim == 3 else vis, np.float32)
        center, scale = np.asarray(center), np.asarray(scale)
        self.box_f32 = center.dtype == np.float32 and scale.dtype == np.float32
        j = joints.shape[1]
        if not (joints.shape == (n, j, 3) and vis.shape == (n, j) and center.shape == (n, 2) and scale.shape == (n, 2)):
            raise R.FpdError('DeviceJointsDB: annotation shapes do not match %d images x %d joints' % (n, j))
        self.n, self.num_joints = n, j
        self.flip_pairs = [list(p) for p in flip_pairs]
        self.upper_body_ids = tuple(upper_body_ids)
        self.aspect_ratio, self.pixel_std = float(aspect_ratio), float(pixel_std)
        # host copies: what validation hands to core.function.validate, and evaluate()
        self.h_joints, self.h_vis = joints, vis
        self.h_center, self.h_scale = np.ascontiguousarray(center, np.float64), np.ascontiguousarray(scale, np.float64)
        self.names = ['scene/%d' % i for i in range(n)]
        # a database that holds rows [row0, row0 + n) of a dataset of n_total rows (the datasets' to_device(rows=...))
        self.row0, self.n_total = 0, n
        self.h_scores = None if scores is None else np.ascontiguousarray(scores, np.float64).reshape(-1)
        if self.h_scores is not None and self.h_scores.size != n:
            raise R.FpdError('DeviceJointsDB: %d scores for %d samples' % (self.h_scores.size, n))
        # one packed image buffer + its table
        if load is None:
            for i, im in enumerate(images):
                if not (im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3):
                    raise R.FpdError('DeviceJointsDB: image %d must be a uint8 [h,w,3] array' % i)
            shapes = [(im.shape[0], im.shape[1]) for im in images]
        else:
            shapes = [(int(h), int(w)) for h, w in images]
        sizes = np.array([h * w * 3 for h, w in shapes], np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        need = int(offs[-1])
        free = torch.cuda.mem_get_info(self.device)[0]
        if need > free:
            raise R.FpdError('DeviceJointsDB: the %d images need %d bytes of device memory and %d bytes are free; the '
                             'database is device-resident, there is no host-resident mode' % (n_images, need, free))
        if load is None:
            packed = np.empty(need, np.uint8)
            for i, im in enumerate(images):
                packed[offs[i]:offs[i + 1]] = im.reshape(-1)
            self.pixels = torch.from_numpy(packed).to(self.device)
        else:
            self.pixels = self._stream(shapes, offs, load, int(chunk_bytes))
        self.image_index, self.image_offsets = image_index, offs
        table = (R.AugImgT * n)()
        base = self.pixels.data_ptr()
        for i, k in enumerate(image_index):
            h, w = shapes[k]
            table[i].img, table[i].h, table[i].w, table[i].row_bytes = base + int(offs[k]), h, w, w * 3
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        self.table = dev(np.frombuffer(bytes(table), np.uint8).copy())
        self.joints, self.vis, self.center, self.scale = dev(joints), dev(vis), dev(self.h_center), dev(self.h_scale)
        self.flip_src = dev(np.array(channel_sources(j, self.flip_pairs), np.int32))
        self.upper = dev(np.array([1 if k in self.upper_body_ids else 0 for k in range(j)], np.int32))
        self.joints_weight = None if joints_weight is None else dev(np.asarray(joints_weight, np.float32).reshape(j))

    def _stream(self, shapes, offs, load, chunk_bytes):
        """The packed pixel buffer, filled in image order through one pinned block: bytes [done, done + fill) of the
        buffer sit in stage[0:fill) until the block is full or the last image is in."""
        need = int(offs[-1])
        if chunk_bytes < 1:
            raise R.FpdError('DeviceJointsDB: chunk_bytes must be positive')
        pixels = torch.empty(need, dtype=torch.uint8, device=self.device)
        stage = torch.empty(max(min(chunk_bytes, need), 1), dtype=torch.uint8, pin_memory=True)
        host, cap = stage.numpy(), stage.numel()
        done = fill = 0
        for i, (h, w) in enumerate(shapes):
            im = load(i)
            if not (isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.shape == (h, w, 3)):
                raise R.FpdError('DeviceJointsDB: image %d must be a uint8 [%d,%d,3] array, load() gave %s %s'
                                 % (i, h, w, getattr(im, 'dtype', type(im)), getattr(im, 'shape', '')))
            flat, pos = np.ascontiguousarray(im).reshape(-1), 0
            assert done + fill == offs[i]
            while pos < flat.size:
                k = min(cap - fill, flat.size - pos)
                host[fill:fill + k] = flat[pos:pos + k]
                fill, pos = fill + k, pos + k
                if fill == cap:
                    pixels[done:done + fill].copy_(stage[:fill])       # blocking: the block is free again on return
                    done, fill = done + fill, 0
        if fill:
            pixels[done:done + fill].copy_(stage[:fill])
        assert done + fill == need
        return pixels

    def __len__(self):
        return self.n

    def args(self):
        d = R.AugDbT()
        d.N, d.J, d.box_f32 = self.n, self.num_joints, int(self.box_f32)
        d.images, d.joints, d.vis = self.table.data_ptr(), self.joints.data_ptr(), self.vis.data_ptr()
        d.center, d.scale = self.center.data_ptr(), self.scale.data_ptr()
        d.flip_src, d.upper = self.flip_src.data_ptr(), self.upper.data_ptr()
        d.aspect_ratio, d.pixel_std = self.aspect_ratio, self.pixel_std
        return d

    def evaluate(self, cfg, preds, output_dir, all_boxes, img_path, *args, **kwargs):
        """(name_value, perf_indicator) with the signature core.function.validate calls: PCK@0.5 of the predicted image
        coordinates against the annotated joints, threshold in units of a tenth of the person box height."""
        n = preds.shape[0]
        k = np.arange(n) % self.n
        d = np.linalg.norm(preds[:, :, 0:2] - self.h_joints[k][:, :, 0:2], axis=2) / (0.1 * self.h_scale[k][:, 1:2] * self.pixel_std)
        vis = self.h_vis[k] > 0
        pck = float(((d < 0.5) & vis).sum() / max(vis.sum(), 1))
        return {'PCK@0.5': pck}, pck


def epoch_order(n, seed, epoch, shuffle, rank=0, world_size=1):
    """(database rows of this rank in this epoch as int32, the generator its augmentation draws come from).

    One process: the permutation of (seed, epoch), and the draws continue on the generator that made it.  world_size > 1,
    every rank holding the whole database: all ranks draw that same permutation, pad it by wrap-around to a multiple of
    world_size and take rank::world_size (torch.utils.data.DistributedSampler's rule), and each draws its augmentation
    numbers from a generator of its own, seeded by (seed, epoch, rank)."""
    rank, world_size = int(rank), int(world_size)
    if not 0 <= rank < world_size:
        raise R.FpdError('epoch_order: rank %d is not in [0, %d)' % (rank, world_size))
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, epoch])))
    order = rng.permutation(n).astype(np.int32) if shuffle else np.arange(n, dtype=np.int32)
    if world_size == 1:
        return order, rng
    total = (n + world_size - 1) // world_size * world_size
    order = np.resize(order, total) if n else order
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, epoch, rank])))
    return np.ascontiguousarray(order[rank::world_size]), rng


def block_range(n, rank, world_size):
    """Rows [n*r//w, n*(r+1)//w) of n: contiguous blocks that tile [0, n) with no padding and no duplicate."""
    rank, world_size = int(rank), int(world_size)
    if not 0 <= rank < world_size:
        raise R.FpdError('block_range: rank %d is not in [0, %d)' % (rank, world_size))
    return n * rank // world_size, n * (rank + 1) // world_size


class DeviceAugmentLoader:
    def __init__(self, db, cfg, batch_size, is_train, shuffle=None, drop_last=None, seed=0,
                 mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), rank=0, world_size=1, partition='strided'):
        """partition: how world_size > 1 ranks share the rows.  'strided' = epoch_order's rank::world_size of the padded
        epoch permutation (training; every rank sees the same number of batches, rows may repeat).  'block' (validation
        only) = block_range of the dataset in database order: no padding, no duplicate, so the ranks' results concatenate
        to the whole set; the database may hold just that block (to_device(rows=...))."""
        self.db, self.batch_size, self.is_train = db, int(batch_size), bool(is_train)
        self.rank, self.world_size = int(rank), int(world_size)
        if not 0 <= self.rank < self.world_size:
            raise R.FpdError('DeviceAugmentLoader: rank %d is not in [0, %d)' % (self.rank, self.world_size))
        if partition not in ('strided', 'block'):
            raise R.FpdError("DeviceAugmentLoader: partition must be 'strided' or 'block', got %r" % (partition,))
        self.partition = partition
        self.shuffle = self.is_train if shuffle is None else bool(shuffle)
        if partition == 'block':
            if self.is_train:
                raise R.FpdError("DeviceAugmentLoader: partition='block' is for validation (is_train=False); training "
                                 'ranks need equal batch counts, which the strided rule pads for')
            if self.shuffle:
                raise R.FpdError("DeviceAugmentLoader: partition='block' yields database order; shuffle must be off")
            self.rows = block_range(getattr(db, 'n_total', len(db)), self.rank, self.world_size)
            row0 = getattr(db, 'row0', 0)
            if not (row0 <= self.rows[0] and self.rows[1] <= row0 + len(db)):
                raise R.FpdError('DeviceAugmentLoader: rank %d validates rows [%d, %d) and the database holds [%d, %d)'
                                 % (self.rank, self.rows[0], self.rows[1], row0, row0 + len(db)))
        self.drop_last = self.is_train if drop_last is None else bool(drop_last)
        self.seed, self.epoch = int(seed), 0
        self.image_size = tuple(int(v) for v in cfg.MODEL.IMAGE_SIZE)
        self.heatmap_size = tuple(int(v) for v in cfg.MODEL.HEATMAP_SIZE)
        ds = cfg.DATASET
        self.sf, self.rf, self.flip = float(ds.SCALE_FACTOR), float(ds.ROT_FACTOR), bool(ds.FLIP)
        self.prob_half_body, self.num_joints_half_body = float(ds.PROB_HALF_BODY), int(ds.NUM_JOINTS_HALF_BODY)
        self.sigma, self.unbiased = int(cfg.MODEL.SIGMA), unbiased_targets(cfg)
        self.g = torch.from_numpy(np.ascontiguousarray(gaussian_patch(self.sigma), np.float32)).to(db.device)
        # a database without a weight table behaves like the reference's joints_weight = 1 (JointsDataset.py:54)
        self.joints_weight = db.joints_weight if cfg.LOSS.USE_DIFFERENT_JOINTS_WEIGHT else None
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        n, b = (len(self.db) + self.world_size - 1) // self.world_size, self.batch_size      # samples of this rank
        if self.partition == 'block':
            n = self.rows[1] - self.rows[0]
        return n // b if self.drop_last else (n + b - 1) // b

    def __iter__(self):
        if self.partition == 'block':
            order, rng = np.arange(self.rows[0], self.rows[1], dtype=np.int32) - np.int32(getattr(self.db, 'row0', 0)), None
        else:
            order, rng = epoch_order(len(self.db), self.seed, self.epoch, self.shuffle, self.rank, self.world_size)
        self.epoch += 1
        for k in range(len(self)):
            yield self.batch(order[k * self.batch_size:(k + 1) * self.batch_size], rng)

    def stage(self, idx, rng):
        """The pinned [B,8]-double staging rows: int32 index in the first word, the six draws in columns 1..6."""
        b = len(idx)
        host = torch.empty((b, 8), dtype=torch.float64, pin_memory=True)       # a fresh block per batch: the caching host
        rows = host.numpy()                                                     # allocator recycles it after the copy ran
        rows.view(np.int32)[:, 0] = idx
        if self.is_train:
            u, nrm = rng.random((b, 3)), rng.standard_normal((b, 3))
            rows[:, (1, 5, 6)] = u
            rows[:, 2:5] = nrm
        return host

    def batch(self, idx, rng=None, draws=None):
        """One batch for the database rows `idx` (int32 array) -> (input, target, target_weight, meta); meta also carries the
        2x3 matrices (`trans`).  draws [B,6] overrides the generator (tests)."""
        db, dev = self.db, self.db.device
        b = len(idx)
        if draws is not None:
            host = torch.empty((b, 8), dtype=torch.float64, pin_memory=True)
            host.numpy().view(np.int32)[:, 0] = idx
            host.numpy()[:, 1:7] = draws
        else:
            host = self.stage(idx, rng)
        rows = host.to(dev, non_blocking=True)
        inp, target, weight, p = self.launch(rows, b)
        if self.is_train:
            meta = {'center': p['center'], 'scale': p['scale'], 'rotation': p['rotation'], 'flipped': p['flipped'],
                    'joints': p['joints'], 'joints_vis': p['vis'], 'index': rows.view(torch.int32)[:, 0]}
        else:
            contiguous = b > 0 and int(idx[-1]) - int(idx[0]) == b - 1
            meta = {'center': torch.from_numpy(db.h_center[idx]), 'scale': torch.from_numpy(db.h_scale[idx]),
                    'score': torch.ones(b, dtype=torch.float64) if db.h_scores is None else torch.from_numpy(db.h_scores[idx]),
                    'index': torch.from_numpy(np.asarray(idx) + np.int32(getattr(db, 'row0', 0))),      # dataset rows
                    'image': db.names[int(idx[0]):int(idx[0]) + b] if contiguous else [db.names[i] for i in idx],
                    'joints': p['joints'], 'joints_vis': p['vis']}
        meta['trans'] = p['trans']
        return inp, target, weight, meta

    def launch(self, rows, b):
        """The three launches for staged device rows [b,8] -> (input, target, target_weight, parameter tensors)."""
        db, dev = self.db, self.db.device
        j = db.num_joints
        w, h = self.image_size
        hw, hh = self.heatmap_size
        f64 = dict(dtype=torch.float64, device=dev)
        p = {'crop': torch.empty((b, C.sizeof(R.AugCropT)), dtype=torch.uint8, device=dev),
             'trans': torch.empty((b, 2, 3), **f64), 'joints': torch.empty((b, j, 3), **f64),
             'vis': torch.empty((b, j), dtype=torch.float32, device=dev), 'center': torch.empty((b, 2), **f64),
             'scale': torch.empty((b, 2), **f64), 'rotation': torch.empty((b,), **f64),
             'flipped': torch.empty((b,), dtype=torch.int32, device=dev)}
        st = R.current_stream()
        a = R.AugmentT()
        a.db = db.args()
        a.B, a.is_train, a.flip, a.num_joints_half_body = b, int(self.is_train), int(self.flip), self.num_joints_half_body
        a.idx_stride, a.draw_stride, a.out_w, a.out_h = 16, 8, w, h
        a.sf, a.rf, a.prob_half_body = self.sf, self.rf, self.prob_half_body
        a.idx, a.draws = rows.data_ptr(), rows.data_ptr() + 8
        a.crop, a.trans, a.joints, a.vis = p['crop'].data_ptr(), p['trans'].data_ptr(), p['joints'].data_ptr(), p['vis'].data_ptr()
        a.center, a.scale, a.rotation, a.flipped = (p['center'].data_ptr(), p['scale'].data_ptr(), p['rotation'].data_ptr(),
                                                    p['flipped'].data_ptr())
        R.check(R.lib().fpd_augment_params(a, st), 'fpd_augment_params')
        inp = torch.empty((b, 3, h, w), dtype=torch.float32, device=dev)
        c = R.WarpAugT()
        c.B, c.H, c.W, c.N = b, h, w, db.n
        c.images, c.crop, c.out = db.table.data_ptr(), p['crop'].data_ptr(), inp.data_ptr()
        for k in range(3):
            c.mean[k], c.std[k] = self.mean[k], self.std[k]
        R.check(R.lib().fpd_warp_affine_aug(c, st), 'fpd_warp_affine_aug')
        if self.unbiased:
            target, weight = render_targets_unbiased(p['joints'], p['vis'], (hw, hh), (w, h), self.sigma, self.joints_weight)
            return inp, target, weight, p
        target = torch.empty((b, j, hh, hw), dtype=torch.float32, device=dev)
        weight = torch.empty((b, j, 1), dtype=torch.float32, device=dev)
        t = R.TargetsWT()
        t.t.B, t.t.J, t.t.H, t.t.W, t.t.patch = b, j, hh, hw, self.g.shape[0]
        t.t.stride_x, t.t.stride_y = w / hw, h / hh
        t.t.joints, t.t.vis, t.t.g = p['joints'].data_ptr(), p['vis'].data_ptr(), self.g.data_ptr()
        t.t.target, t.t.weight = target.data_ptr(), weight.data_ptr()
        if self.joints_weight is not None:
            t.joints_weight = self.joints_weight.data_ptr()
        R.check(R.lib().fpd_render_targets_w(t, st), 'fpd_render_targets_w')
        return inp, target, weight, p


def synthetic_aug(cfg, device, rank=0, train=True, world_size=1):
    """DATASET.DATASET 'synthetic_aug' of the tools: seeded scenes (synth.make_scenes) about 1.25x the network input in
    size, resident on the device, behind augmenting loaders; every rank validates its block of the validation scenes.
    -> (train_loader or None, valid_loader, valid_db)."""
    w, h = (int(v) for v in cfg.MODEL.IMAGE_SIZE)
    side = max(w, h)

    def db(seed, n):
        return DeviceJointsDB(device=device, **synth.make_scenes(seed, n, cfg.MODEL.NUM_JOINTS, size=(side, side + side // 2),
                                                                 aspect_ratio=w * 1.0 / h))
    loader = None
    if train:
        loader = DeviceAugmentLoader(db(rank * 1000003 + 17, cfg.DATASET.NUM_SCENES), cfg, cfg.TRAIN.BATCH_SIZE_PER_GPU, True,
                                     shuffle=cfg.TRAIN.SHUFFLE, drop_last=True, seed=rank)
    valid_db = db(1009, cfg.DATASET.NUM_VALID_SAMPLES)
    return loader, DeviceAugmentLoader(valid_db, cfg, cfg.TEST.BATCH_SIZE_PER_GPU, False, rank=rank, world_size=world_size,
                                       partition='block'), valid_db
