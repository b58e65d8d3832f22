"""The COCO keypoint dataset (/root/reference/lib/dataset/coco.py): the records of `_get_db` from ground-truth or detection
boxes, the decoded images resident on the device behind the augmenting loaders (device_dataset.py), and `evaluate`:
rescoring + OKS NMS of every picture in one launch (csrc/oks_nms.hip through lib/nms/nms.py), the results file, and
the keypoint AP / AR table (coco_eval.py: matched and accumulated on the device, csrc/coco_eval.hip).

    root/annotations/person_keypoints_<set>.json      (image_info_<set>.json for a test set)
    root/images/<set>/<%012d>.jpg                     ('COCO_<set>_' in front of the number for the 2014 sets; every test
                                                       set reads the folder test2017)
    TEST.COCO_BBOX_FILE                               list of {image_id, category_id, bbox [x,y,w,h], score}

What differs from the reference's class: pycocotools is not available, so the annotation file is read by AnnotationIndex
below (file order throughout -- what pycocotools' dictionaries give on Python 3.7+, an assumption no test can pin here) and
the AP table comes from coco_eval.py; there is no `__getitem__` (see mpii.py); the pickle cache of the record list is not
written; DATASET.DATA_FORMAT 'zip' and DATASET.SELECT_DATA raise; images are decoded by PIL's libjpeg, not OpenCV's."""
import json
import logging
import os
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ... import runtime as R
from . import coco_eval
from .mpii import _Prefetch, image_shape

logger = logging.getLogger(__name__)


class AnnotationIndex:
    """What COCODataset asks of `pycocotools.coco.COCO` (coco.py:70-172), over the standard library's json, in file order."""

    def __init__(self, path):
        try:
            with open(path) as f:
                data = json.load(f)
        except (OSError, ValueError) as e:
            raise R.FpdError('COCODataset: cannot read the annotations %s (%s)' % (path, e))
        self.images = OrderedDict((im['id'], im) for im in data.get('images', []))
        self.categories = list(data.get('categories', []))
        self.annotations = list(data.get('annotations', []))
        self._of_image = {}
        for a in self.annotations:
            self._of_image.setdefault(a['image_id'], []).append(a)

    def image_ids(self):
        return list(self.images)

    def image(self, image_id):
        return self.images[image_id]

    def image_annotations(self, image_id, iscrowd=None):
        """The annotations of an image; iscrowd False: those with `iscrowd` 0 (getAnnIds(imgIds=, iscrowd=False))."""
        anns = self._of_image.get(image_id, [])
        return list(anns) if iscrowd is None else [a for a in anns if a['iscrowd'] == iscrowd]

    def category_ids(self):
        return [c['id'] for c in self.categories]

    def category_names(self):
        return [c['name'] for c in self.categories]


class COCODataset:
    def __init__(self, cfg, root, image_set, is_train, transform=None):
        if cfg.DATASET.DATA_FORMAT == 'zip':
            raise R.FpdError("COCODataset: DATASET.DATA_FORMAT 'zip' (<set>.zip@) is not supported; unpack the archive "
                             "into %s" % os.path.join(root, 'images', image_set))
        if cfg.DATASET.SELECT_DATA:
            raise R.FpdError('COCODataset: DATASET.SELECT_DATA is not supported')
        self.cfg, self.root, self.image_set, self.is_train = cfg, root, image_set, bool(is_train)
        self.data_format = cfg.DATASET.DATA_FORMAT
        self.nms_thre, self.image_thre, self.soft_nms = cfg.TEST.NMS_THRE, cfg.TEST.IMAGE_THRE, cfg.TEST.SOFT_NMS
        self.oks_thre, self.in_vis_thre = cfg.TEST.OKS_THRE, cfg.TEST.IN_VIS_THRE
        self.bbox_file, self.use_gt_bbox = cfg.TEST.COCO_BBOX_FILE, cfg.TEST.USE_GT_BBOX
        self.image_width, self.image_height = cfg.MODEL.IMAGE_SIZE[0], cfg.MODEL.IMAGE_SIZE[1]
        self.aspect_ratio = self.image_width * 1.0 / self.image_height
        self.pixel_std = 200
        self.color_rgb = bool(cfg.DATASET.COLOR_RGB)
        self.workers = max(1, min(16, int(cfg.WORKERS)))
        prefix = 'person_keypoints' if 'test' not in image_set else 'image_info'
        self.coco = AnnotationIndex(os.path.join(root, 'annotations', prefix + '_' + image_set + '.json'))
        cats = self.coco.category_names()
        self.classes = ['__background__'] + cats
        logger.info('=> classes: {}'.format(self.classes))
        self.num_classes = len(self.classes)
        self._class_to_ind = dict(zip(self.classes, range(self.num_classes)))
        self._class_to_coco_ind = dict(zip(cats, self.coco.category_ids()))
        self._coco_ind_to_class_ind = dict((self._class_to_coco_ind[c], self._class_to_ind[c]) for c in self.classes[1:])
        self.image_set_index = self.coco.image_ids()
        self.num_images = len(self.image_set_index)
        logger.info('=> num_images: {}'.format(self.num_images))
        self.num_joints = 17
        self.flip_pairs = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
        self.parent_ids = None
        self.upper_body_ids = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
        self.lower_body_ids = (11, 12, 13, 14, 15, 16)
        self.joints_weight = np.array([1., 1., 1., 1., 1., 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5],
                                      dtype=np.float32).reshape((self.num_joints, 1))
        self._packed_gt = None
        self.db = self._get_db()
        logger.info('=> load {} samples'.format(len(self.db)))

    def __len__(self):
        return len(self.db)

    def _get_db(self):
        """coco.py:140-147: annotated boxes for training and TEST.USE_GT_BBOX, else the detector's."""
        if self.is_train or self.use_gt_bbox:
            db = []
            for index in self.image_set_index:
                db.extend(self._image_records(index))
            return db
        return self._detection_records()

    def _image_records(self, index):
        """coco.py:156-221: the non-crowd people of one image whose box, clipped to the image, is not empty and who have an
        annotated keypoint; visibility 2 becomes 1."""
        im = self.coco.image(index)
        width, height = im['width'], im['height']
        rec = []
        for obj in self.coco.image_annotations(index, iscrowd=False):
            x, y, w, h = obj['bbox']
            x1 = np.max((0, x))
            y1 = np.max((0, y))
            x2 = np.min((width - 1, x1 + np.max((0, w - 1))))
            y2 = np.min((height - 1, y1 + np.max((0, h - 1))))
            if not (obj['area'] > 0 and x2 >= x1 and y2 >= y1):
                continue
            if self._coco_ind_to_class_ind[obj['category_id']] != 1:
                continue
            if max(obj['keypoints']) == 0:
                continue
            k = np.asarray(obj['keypoints'][:self.num_joints * 3], dtype=np.float64).reshape(self.num_joints, 3)
            joints_3d = np.zeros((self.num_joints, 3), dtype=np.float64)
            joints_3d_vis = np.zeros((self.num_joints, 3), dtype=np.float64)
            joints_3d[:, 0:2] = k[:, 0:2]
            joints_3d_vis[:, 0] = joints_3d_vis[:, 1] = np.minimum(k[:, 2], 1)
            center, scale = self._box2cs([x1, y1, x2 - x1, y2 - y1])
            rec.append({'image': self.image_path_from_index(index), 'center': center, 'scale': scale, 'joints_3d': joints_3d,
                        'joints_3d_vis': joints_3d_vis, 'filename': '', 'imgnum': 0})
        return rec

    def _box2cs(self, box):
        x, y, w, h = box[:4]
        return self._xywh2cs(x, y, w, h)

    def _xywh2cs(self, x, y, w, h):
        """coco.py:227-242: the box centre, and the box grown to the network's aspect ratio and by 1.25, in units of
        200 px; both float32."""
        center = np.zeros((2), dtype=np.float32)
        center[0] = x + w * 0.5
        center[1] = y + h * 0.5
        if w > self.aspect_ratio * h:
            h = w * 1.0 / self.aspect_ratio
        elif w < self.aspect_ratio * h:
            w = h * self.aspect_ratio
        scale = np.array([w * 1.0 / self.pixel_std, h * 1.0 / self.pixel_std], dtype=np.float32)
        if center[0] != -1:
            scale = scale * 1.25
        return center, scale

    def image_path_from_index(self, index):
        """coco.py:244-257, e.g. images/train2017/000000119993.jpg."""
        file_name = '%012d.jpg' % index
        if '2014' in self.image_set:
            file_name = 'COCO_%s_' % self.image_set + file_name
        prefix = 'test2017' if 'test' in self.image_set else self.image_set
        return os.path.join(self.root, 'images', prefix, file_name)

    def _detection_records(self):
        """coco.py:259-300: every person box of TEST.COCO_BBOX_FILE with score >= TEST.IMAGE_THRE; no joints, all visible."""
        try:
            with open(self.bbox_file, 'r') as f:
                all_boxes = json.load(f)
        except (OSError, ValueError) as e:
            raise R.FpdError('COCODataset: cannot read TEST.COCO_BBOX_FILE %r (%s)' % (self.bbox_file, e))
        if not all_boxes:
            raise R.FpdError('COCODataset: TEST.COCO_BBOX_FILE %r holds no boxes' % self.bbox_file)
        logger.info('=> Total boxes: {}'.format(len(all_boxes)))
        db = []
        for det in all_boxes:
            if det['category_id'] != 1:
                continue
            score = det['score']
            if score < self.image_thre:
                continue
            center, scale = self._box2cs(det['bbox'])
            db.append({'image': self.image_path_from_index(det['image_id']), 'center': center, 'scale': scale, 'score': score,
                       'joints_3d': np.zeros((self.num_joints, 3), dtype=np.float64),
                       'joints_3d_vis': np.ones((self.num_joints, 3), dtype=np.float64)})
        logger.info('=> Total boxes after fliter low score@{}: {}'.format(self.image_thre, len(db)))
        return db

    def to_device(self, device='cuda', chunk_bytes=None, rows=None):
        """-> DeviceJointsDB as MPIIDataset.to_device builds it: every distinct picture decoded once and shared by its people,
        streamed into one device buffer; `names` are the picture paths (evaluate reads the picture id out of them); the box
        scores of a detection-box set travel as the database's `scores`."""
        from .device_dataset import DEFAULT_CHUNK_BYTES, DeviceJointsDB
        lo, hi = (0, len(self.db)) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= lo <= hi <= len(self.db):
            raise R.FpdError('COCODataset.to_device: rows (%d, %d) outside the %d records' % (lo, hi, len(self.db)))
        recs = self.db[lo:hi]        # rows=(lo, hi): only the pictures these records refer to are decoded and uploaded
        paths, slot = [], {}
        for rec in recs:
            if rec['image'] not in slot:
                slot[rec['image']] = len(paths)
                paths.append(rec['image'])
        index = np.array([slot[rec['image']] for rec in recs], np.int64)
        j = self.num_joints
        stack = lambda k, shape, dt: np.stack([rec[k] for rec in recs]) if recs else np.zeros(shape, dt)  # noqa: E731
        scores = np.array([rec['score'] for rec in recs], np.float64) if recs and 'score' in recs[0] else None
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            shapes = list(pool.map(image_shape, paths))
            db = DeviceJointsDB(shapes, stack('joints_3d', (0, j, 3), np.float64), stack('joints_3d_vis', (0, j, 3), np.float64),
                                stack('center', (0, 2), np.float32), stack('scale', (0, 2), np.float32), self.flip_pairs,
                                self.upper_body_ids, self.aspect_ratio, joints_weight=self.joints_weight, device=device,
                                pixel_std=self.pixel_std, image_index=index,
                                load=_Prefetch(pool, paths, self.color_rgb, 2 * self.workers),
                                chunk_bytes=DEFAULT_CHUNK_BYTES if chunk_bytes is None else chunk_bytes, scores=scores)
        db.names = [rec['image'] for rec in recs]
        db.row0, db.n_total = lo, len(self.db)
        logger.info('=> %s: %d samples over %d images, %.1f MB on %s', self.image_set, len(db), len(paths),
                    db.pixels.numel() / 1e6, db.device)
        return db

    def nms(self, preds, all_boxes, img_path, device='cuda', timer=None):
        """Rescoring + OKS NMS of coco.py:318-369 -> (picture ids in order of first appearance, per picture the kept people
        as rows of `preds` in pick order, the rescored value of every row).  The people are sorted by picture on the host
        (one stable argsort), uploaded once, and one launch serves every picture."""
        from ..nms.nms import oks_nms_device
        ids = np.array([int(p[-16:-4]) for p in img_path], np.int64)
        n = len(ids)
        first = {}
        for i in ids.tolist():
            first.setdefault(i, len(first))
        group = np.array([first[i] for i in ids.tolist()], np.int64)
        order = np.argsort(group, kind='stable')
        offsets = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=len(first)))]).astype(np.int64)
        preds = np.asarray(preds)
        score, keep, n_keep = oks_nms_device(preds[:n][order], np.asarray(all_boxes)[:n, 4][order], np.asarray(all_boxes)[:n, 5][order],
                                             offsets, self.oks_thre, soft=bool(self.soft_nms), in_vis_thre=self.in_vis_thre,
                                             device=device, timer=timer)
        rescored = np.empty(n, np.float64)
        rescored[order] = score
        kept = [order[offsets[k] + keep[offsets[k]:offsets[k] + n_keep[k]]] for k in range(len(first))]
        return list(first), kept, rescored

    def packed_ground_truth(self):
        """The annotations as coco_eval.pack_ground_truth's arrays: made on first use, they do not change between validations."""
        if self._packed_gt is None:
            cats = self.coco.category_ids()
            if len(cats) != 1:
                raise R.FpdError('COCODataset: the device AP table evaluates exactly one category, the annotations have %d '
                                 '(evaluate(..., host_eval=True) takes any number)' % len(cats))
            self._packed_gt = coco_eval.pack_ground_truth(self.coco.annotations, self.coco.image_ids(), cats[0])
        return self._packed_gt

    def evaluate(self, cfg, preds, output_dir, all_boxes, img_path, *args, **kwargs):
        """coco.py:302-379 -> (OrderedDict of the ten statistics, AP); ({'Null': 0}, 0) for a test set.  Writes
        <output_dir>/results/keypoints_<set>_results_<RANK>.json: picture order, then pick order.  The AP table comes from the
        device (coco_eval.evaluate_arrays_device over the kept people as arrays); host_eval=True: from the numpy functions."""
        res_folder = os.path.join(output_dir, 'results')
        os.makedirs(res_folder, exist_ok=True)
        res_file = os.path.join(res_folder, 'keypoints_{}_results_{}.json'.format(self.image_set, cfg.RANK))
        pictures, kept, rescored = self.nms(preds, all_boxes, img_path)
        cat_id = self._class_to_coco_ind[self.classes[1]]
        flat = np.asarray(preds, np.float64).reshape(len(preds), -1)
        boxes = np.asarray(all_boxes, np.float64)
        results = [{'image_id': int(pic), 'category_id': cat_id, 'keypoints': flat[r].tolist(), 'score': float(rescored[r]),
                    'center': boxes[r, 0:2].tolist(), 'scale': boxes[r, 2:4].tolist()}
                   for pic, rows in zip(pictures, kept) for r in rows]
        logger.info('=> writing results json to %s' % res_file)
        with open(res_file, 'w') as f:
            json.dump(results, f, sort_keys=True, indent=4)
        if 'test' in self.image_set:
            return {'Null': 0}, 0
        if kwargs.get('host_eval', False):
            stats = coco_eval.evaluate_keypoints(self.coco.annotations, results, self.coco.image_ids(), self.coco.category_ids())
        else:
            rows = np.concatenate(kept).astype(np.int64) if kept else np.zeros(0, np.int64)
            stats = coco_eval.evaluate_arrays_device(self.packed_ground_truth(), np.repeat(np.asarray(pictures, np.int64), [len(k) for k in kept]),
                                                     flat[rows], rescored[rows], device=kwargs.get('device', 'cuda'))
        name_value = OrderedDict(zip(coco_eval.STAT_NAMES, [float(v) for v in stats]))
        return name_value, name_value['AP']


def coco(cfg, device, rank=0, world_size=1, train=True):
    """DATASET.DATASET 'coco' of the tools, as `mpii`: DATASET.ROOT / TRAIN_SET behind an augmenting loader that takes this
    rank's share of every epoch, DATASET.ROOT / TEST_SET (ground-truth or detection boxes per TEST.USE_GT_BBOX) behind a
    validation loader over this rank's block of the set (every rank validates, rank 0 evaluates).
    -> (train_loader or None, valid_loader, valid_set)."""
    from .device_dataset import DeviceAugmentLoader, block_range
    loader = None
    if train:
        train_set = COCODataset(cfg, cfg.DATASET.ROOT, cfg.DATASET.TRAIN_SET, True)
        loader = DeviceAugmentLoader(train_set.to_device(device), cfg, cfg.TRAIN.BATCH_SIZE_PER_GPU, True, shuffle=cfg.TRAIN.SHUFFLE,
                                     drop_last=True, seed=0, rank=rank, world_size=world_size)
    valid_set = COCODataset(cfg, cfg.DATASET.ROOT, cfg.DATASET.TEST_SET, False)
    rows = block_range(len(valid_set), rank, world_size)
    valid_loader = DeviceAugmentLoader(valid_set.to_device(device, rows=rows), cfg, cfg.TEST.BATCH_SIZE_PER_GPU, False,
                                       rank=rank, world_size=world_size, partition='block')
    return loader, valid_loader, valid_set
