"""The MPII Human Pose dataset (/root/reference/lib/dataset/mpii.py): the annotation records of `_get_db`, the decoded
images resident on the device behind the augmenting loaders (device_dataset.py), and PCKh.

    root/annot/<image_set>.json        list of {image, center [x,y], scale, joints [16][2], joints_vis [16]}, 1-based
    root/annot/gt_<TEST_SET>.mat       dataset_joints, jnt_missing, pos_gt_src, headboxes_src (evaluate)
    root/images/<image>                anything PIL decodes, or a .npy holding a uint8 [h,w,3] array in B,G,R order

What differs from the reference's class: there is no `__getitem__` -- `to_device()` decodes every distinct image once
(several people share one) and hands the records to a DeviceJointsDB, whose loaders do the per-sample work in three
launches per batch; `aspect_ratio` is set (the reference leaves it unset, so PROB_HALF_BODY > 0 crashes there); the
pickle cache of the record list under DATASET.CACHE_ROOT is not reproduced (the records are rebuilt from the JSON on
every start); DATASET.DATA_FORMAT 'zip' and DATASET.SELECT_DATA raise.  Images are decoded by PIL's libjpeg, the
reference's by OpenCV's: the same file may decode to pixels that differ by a few grey levels."""
import json
import logging
import os
from collections import OrderedDict, deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ... import runtime as R

logger = logging.getLogger(__name__)

SC_BIAS = 0.6
PCKH_ROWS = (('Head', ('head',)), ('Shoulder', ('lsho', 'rsho')), ('Elbow', ('lelb', 'relb')), ('Wrist', ('lwri', 'rwri')),
             ('Hip', ('lhip', 'rhip')), ('Knee', ('lkne', 'rkne')), ('Ankle', ('lank', 'rank')))


def image_shape(path):
    """(h, w) of an image file without decoding it."""
    try:
        if path.endswith('.npy'):
            shape = np.load(path, mmap_mode='r').shape
            if len(shape) != 3 or shape[2] != 3:
                raise ValueError('shape %s is not [h,w,3]' % (shape,))
            return int(shape[0]), int(shape[1])
        from PIL import Image
        with Image.open(path) as im:
            w, h = im.size
        return int(h), int(w)
    except Exception as e:
        raise R.FpdError('MPIIDataset: cannot read image %s (%s: %s)' % (path, type(e).__name__, e))


def read_image(path, color_rgb=False):
    """The uint8 [h,w,3] array `cv2.imread(path, IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION)` stands for (B,G,R; the EXIF
    orientation is not applied), in R,G,B order with DATASET.COLOR_RGB (JointsDataset.py:126-131)."""
    try:
        if path.endswith('.npy'):
            bgr = np.load(path)
            if not (bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3):
                raise ValueError('%s %s is not a uint8 [h,w,3] array' % (bgr.dtype, bgr.shape))
            return np.ascontiguousarray(bgr[:, :, ::-1] if color_rgb else bgr)
        from PIL import Image
        with Image.open(path) as im:
            rgb = np.asarray(im.convert('RGB'), np.uint8)
        return np.ascontiguousarray(rgb if color_rgb else rgb[:, :, ::-1])
    except Exception as e:
        raise R.FpdError('MPIIDataset: cannot read image %s (%s: %s)' % (path, type(e).__name__, e))


class _Prefetch:
    """load(i) for i = 0, 1, 2, ...: image i decoded by a pool thread, at most `depth` images ahead of the consumer."""

    def __init__(self, pool, paths, color_rgb, depth):
        self.pool, self.paths, self.color_rgb, self.depth = pool, paths, color_rgb, depth
        self.pending, self.next = deque(), 0

    def __call__(self, i):
        while self.next < len(self.paths) and self.next < i + self.depth:
            self.pending.append(self.pool.submit(read_image, self.paths[self.next], self.color_rgb))
            self.next += 1
        return self.pending.popleft().result()


class MPIIDataset:
    def __init__(self, cfg, root, image_set, is_train, transform=None):
        if cfg.DATASET.DATA_FORMAT == 'zip':
            raise R.FpdError("MPIIDataset: DATASET.DATA_FORMAT 'zip' (images.zip@) is not supported; unpack the archive "
                             "into %s" % os.path.join(root, 'images'))
        if cfg.DATASET.SELECT_DATA:
            raise R.FpdError('MPIIDataset: DATASET.SELECT_DATA is not supported')
        self.cfg, self.root, self.image_set, self.is_train = cfg, root, image_set, bool(is_train)
        self.pixel_std = 200
        self.num_joints = 16
        self.flip_pairs = [[0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13]]
        self.parent_ids = [1, 2, 6, 6, 3, 4, 6, 6, 7, 8, 11, 12, 7, 7, 13, 14]
        self.upper_body_ids = (7, 8, 9, 10, 11, 12, 13, 14, 15)
        self.lower_body_ids = (0, 1, 2, 3, 4, 5, 6)
        w, h = cfg.MODEL.IMAGE_SIZE
        self.aspect_ratio = w * 1.0 / h
        self.color_rgb = bool(cfg.DATASET.COLOR_RGB)
        self.workers = max(1, min(16, int(cfg.WORKERS)))
        self.db = self._get_db()
        logger.info('=> load {} samples'.format(len(self.db)))

    def __len__(self):
        return len(self.db)

    def _get_db(self):
        """mpii.py:56-107: the person box grows by 1.25 and its centre moves down by 15 px per unit of scale unless the
        centre is the -1 placeholder; centre and joints go from MATLAB's 1-based pixels to 0-based; float64 throughout;
        the `test` set has no joints."""
        path = os.path.join(self.root, 'annot', self.image_set + '.json')
        try:
            with open(path) as f:
                anno = json.load(f)
        except (OSError, ValueError) as e:
            raise R.FpdError('MPIIDataset: cannot read the annotations %s (%s)' % (path, e))
        db = []
        for a in anno:
            c = np.array(a['center'], dtype=np.float64)
            s = np.array([a['scale'], a['scale']], dtype=np.float64)
            if c[0] != -1:
                c[1] = c[1] + 15 * s[1]
                s = s * 1.25
            c = c - 1
            joints_3d = np.zeros((self.num_joints, 3), dtype=np.float64)
            joints_3d_vis = np.zeros((self.num_joints, 3), dtype=np.float64)
            if self.image_set != 'test':
                joints = np.array(a['joints'])
                vis = np.array(a['joints_vis'])
                if len(joints) != self.num_joints:
                    raise R.FpdError('MPIIDataset: %s has a record with %d joints, not %d' % (path, len(joints), self.num_joints))
                joints_3d[:, 0:2] = joints[:, 0:2] - 1
                joints_3d_vis[:, 0] = vis
                joints_3d_vis[:, 1] = vis
            db.append({'image': os.path.join(self.root, 'images', a['image']), 'center': c, 'scale': s,
                       'joints_3d': joints_3d, 'joints_3d_vis': joints_3d_vis, 'filename': '', 'imgnum': 0})
        return db

    def to_device(self, device='cuda', chunk_bytes=None, rows=None):
        """-> DeviceJointsDB: every distinct image decoded once by min(16, WORKERS) threads a few images ahead of the
        upload, streamed into one device buffer; `names` are the image paths (validate's image_path)."""
        from .device_dataset import DEFAULT_CHUNK_BYTES, DeviceJointsDB
        lo, hi = (0, len(self.db)) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= lo <= hi <= len(self.db):
            raise R.FpdError('MPIIDataset.to_device: rows (%d, %d) outside the %d records' % (lo, hi, len(self.db)))
        recs = self.db[lo:hi]        # rows=(lo, hi): only the pictures these records refer to are decoded and uploaded
        paths, slot = [], {}
        for rec in recs:
            if rec['image'] not in slot:
                slot[rec['image']] = len(paths)
                paths.append(rec['image'])
        index = np.array([slot[rec['image']] for rec in recs], np.int64)
        stack = lambda k, shape: np.stack([rec[k] for rec in recs]) if recs else np.zeros(shape)  # noqa: E731
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            shapes = list(pool.map(image_shape, paths))
            db = DeviceJointsDB(shapes, stack('joints_3d', (0, self.num_joints, 3)), stack('joints_3d_vis', (0, self.num_joints, 3)),
                                stack('center', (0, 2)), stack('scale', (0, 2)), self.flip_pairs, self.upper_body_ids,
                                self.aspect_ratio, device=device, pixel_std=self.pixel_std, image_index=index,
                                load=_Prefetch(pool, paths, self.color_rgb, 2 * self.workers),
                                chunk_bytes=DEFAULT_CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
        db.names = [rec['image'] for rec in recs]
        db.row0, db.n_total = lo, len(self.db)
        logger.info('=> %s: %d samples over %d images, %.1f MB on %s', self.image_set, len(db), len(paths),
                    db.pixels.numel() / 1e6, db.device)
        return db

    def evaluate(self, cfg, preds, output_dir, *args, **kwargs):
        """mpii.py:109-194 -> (OrderedDict Head .. Ankle, Mean, Mean@0.1 in percent, Mean).  PCKh: a joint counts when its
        distance to the annotation is at most 0.5 x (0.6 x the head box diagonal); the means weight each joint by its
        number of annotated instances and leave pelvis and thorax (6, 7) out.  On the host, once per epoch."""
        from scipy.io import loadmat, savemat
        preds = preds[:, :, 0:2] + 1.0                                       # back to 1-based
        if output_dir:
            savemat(os.path.join(output_dir, 'pred.mat'), mdict={'preds': preds})
        if 'test' in cfg.DATASET.TEST_SET:
            return {'Null': 0.0}, 0.0
        gt_file = os.path.join(cfg.DATASET.ROOT, 'annot', 'gt_{}.mat'.format(cfg.DATASET.TEST_SET))
        try:
            gt = loadmat(gt_file)
        except (OSError, ValueError) as e:
            raise R.FpdError('MPIIDataset.evaluate: cannot read %s (%s)' % (gt_file, e))
        names = [str(np.ravel(v)[0]) for v in np.ravel(gt['dataset_joints'])]
        visible = 1 - gt['jnt_missing']                                      # [16,N]
        err = np.linalg.norm(np.transpose(preds, [1, 2, 0]) - gt['pos_gt_src'], axis=1)          # [16,N]
        head = np.linalg.norm(gt['headboxes_src'][1, :, :] - gt['headboxes_src'][0, :, :], axis=0) * SC_BIAS
        scaled = err / (head * np.ones((len(err), 1))) * visible
        count = np.sum(visible, axis=1)

        def pckh(threshold):
            return 100. * np.sum((scaled <= threshold) * visible, axis=1) / count
        at_half, at_tenth = pckh(0.5), pckh(np.arange(0, 0.5 + 0.01, 0.01)[11])
        keep = np.ones(len(count), bool)
        keep[6:8] = False
        kept = np.where(keep, count, 0)
        ratio = kept / np.sum(kept).astype(np.float64)
        value = OrderedDict()
        for row, joints in PCKH_ROWS:
            v = [at_half[names.index(j)] for j in joints]
            value[row] = v[0] if len(v) == 1 else 0.5 * (v[0] + v[1])
        value['Mean'] = np.sum(np.where(keep, at_half * ratio, 0))
        value['Mean@0.1'] = np.sum(np.where(keep, at_tenth * ratio, 0))
        return value, value['Mean']


def mpii(cfg, device, rank=0, world_size=1, train=True):
    """DATASET.DATASET 'mpii' of the tools: DATASET.ROOT / TRAIN_SET behind an augmenting loader that takes this rank's share
    of every epoch (every rank holds the whole training set), DATASET.ROOT / TEST_SET behind a validation loader over this
    rank's block of the set (block_range; only that block's pictures are decoded and uploaded; every rank validates, rank 0
    evaluates: core.function.validate(gather=)).  -> (train_loader or None, valid_loader, valid_set)."""
    from .device_dataset import DeviceAugmentLoader, block_range
    loader = None
    if train:
        train_set = MPIIDataset(cfg, cfg.DATASET.ROOT, cfg.DATASET.TRAIN_SET, True)
        loader = DeviceAugmentLoader(train_set.to_device(device), cfg, cfg.TRAIN.BATCH_SIZE_PER_GPU, True, shuffle=cfg.TRAIN.SHUFFLE,
                                     drop_last=True, seed=0, rank=rank, world_size=world_size)
    valid_set = MPIIDataset(cfg, cfg.DATASET.ROOT, cfg.DATASET.TEST_SET, False)
    rows = block_range(len(valid_set), rank, world_size)
    valid_loader = DeviceAugmentLoader(valid_set.to_device(device, rows=rows), cfg, cfg.TEST.BATCH_SIZE_PER_GPU, False,
                                       rank=rank, world_size=world_size, partition='block')
    return loader, valid_loader, valid_set
