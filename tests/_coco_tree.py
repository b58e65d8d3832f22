"""A temporary COCO directory written from the inputs stored in tests/golden/coco_ref.npz (made by
tests/golden/make_golden_coco.py, which runs the reference's own COCODataset on the tree this module writes):

    annotations/person_keypoints_train2017.json, person_keypoints_val2017.json     5 pictures; the annotations of the fixture:
                                                 people with and without keypoints, a crowd, a zero-area box, a box that
                                                 reaches outside its picture
    annotations/image_info_test-dev2017.json     the pictures and categories only
    detections.json                              person boxes with scores, one box of another category, one below IMAGE_THRE
    images/<set>/<%012d>.jpg                     seeded smooth colour fields, five different odd sizes (JPEG via PIL)"""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'coco_ref.npz')
IMAGE_SHAPES = ((97, 141), (163, 105), (119, 157), (135, 101), (107, 151))          # (h, w)
IMAGE_IDS = (785, 139, 872, 1000, 632)                                              # file order, not sorted
SETS = ('train2017', 'val2017')
TEST_SET = 'test-dev2017'
NMS_SIZES = (1, 2, 3, 17, 65, 130, 257)
KEYPOINT_NAMES = ('nose', 'left_eye', 'right_eye', 'left_ear', 'right_ear', 'left_shoulder', 'right_shoulder', 'left_elbow',
                  'right_elbow', 'left_wrist', 'right_wrist', 'left_hip', 'right_hip', 'left_knee', 'right_knee', 'left_ankle',
                  'right_ankle')


def load_golden():
    return dict(np.load(GOLDEN))


def image(k):
    """Picture k: a smooth seeded colour field (JPEG keeps it close), R,G,B."""
    h, w = IMAGE_SHAPES[k]
    rng = np.random.default_rng(2000 + k)
    y, x = np.mgrid[0:h, 0:w]
    planes = [127 + 120 * np.sin(x / rng.uniform(9, 25) + rng.uniform(0, 6)) * np.cos(y / rng.uniform(9, 25) + rng.uniform(0, 6))
              for _ in range(3)]
    return np.stack(planes, -1).astype(np.uint8)


def annotation_file(g, with_annotations=True):
    """The dict of a person_keypoints file from the in_* arrays (image_info: pictures and categories only)."""
    images = [{'id': int(i), 'width': int(IMAGE_SHAPES[k][1]), 'height': int(IMAGE_SHAPES[k][0]), 'file_name': '%012d.jpg' % i}
              for k, i in enumerate(IMAGE_IDS)]
    out = {'images': images, 'categories': [{'id': 1, 'name': 'person', 'supercategory': 'person',
                                             'keypoints': list(KEYPOINT_NAMES), 'skeleton': []}]}
    if with_annotations:
        out['annotations'] = [
            {'id': 100 + n, 'image_id': int(IMAGE_IDS[int(g['in_ann_image'][n])]), 'category_id': 1,
             'bbox': [float(v) for v in g['in_ann_bbox'][n]], 'area': float(g['in_ann_area'][n]),
             'iscrowd': int(g['in_ann_iscrowd'][n]), 'keypoints': [int(v) for v in g['in_ann_keypoints'][n]],
             'num_keypoints': int((g['in_ann_keypoints'][n][2::3] > 0).sum())} for n in range(len(g['in_ann_image']))]
    return out


def detections(g):
    return [{'image_id': int(IMAGE_IDS[int(g['in_det_image'][n])]), 'category_id': int(g['in_det_category'][n]),
             'bbox': [float(v) for v in g['in_det_bbox'][n]], 'score': float(g['in_det_score'][n])}
            for n in range(len(g['in_det_image']))]


def write_tree(root, g, images=True):
    """g: the in_* arrays (the loaded fixture, or the generator's).  -> root"""
    root = str(root)
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    for s in SETS:
        with open(os.path.join(root, 'annotations', 'person_keypoints_%s.json' % s), 'w') as f:
            json.dump(annotation_file(g), f)
    with open(os.path.join(root, 'annotations', 'image_info_%s.json' % TEST_SET), 'w') as f:
        json.dump(annotation_file(g, False), f)
    with open(os.path.join(root, 'detections.json'), 'w') as f:
        json.dump(detections(g), f)
    if images:
        from PIL import Image
        for folder in SETS + ('test2017',):
            os.makedirs(os.path.join(root, 'images', folder), exist_ok=True)
            for k, i in enumerate(IMAGE_IDS):
                Image.fromarray(image(k)).save(os.path.join(root, 'images', folder, '%012d.jpg' % i), quality=92)
    return root


def make_cfg(root, test=None, **dataset):
    """The library's default config, pointed at the tree: 17 joints, 48x64 input, PROB_HALF_BODY on, detections at hand."""
    from fpd_amd.lib.config import _defaults
    cfg = _defaults()
    cfg.MODEL.IMAGE_SIZE, cfg.MODEL.HEATMAP_SIZE, cfg.MODEL.NUM_JOINTS = [48, 64], [12, 16], 17
    cfg.DATASET.DATASET, cfg.DATASET.ROOT, cfg.DATASET.PROB_HALF_BODY = 'coco', str(root), 0.3
    cfg.DATASET.TRAIN_SET, cfg.DATASET.TEST_SET = 'train2017', 'val2017'
    cfg.TEST.COCO_BBOX_FILE, cfg.TEST.IMAGE_THRE, cfg.TEST.OKS_THRE, cfg.TEST.IN_VIS_THRE = os.path.join(str(root), 'detections.json'), 0.1, 0.9, 0.2
    cfg.TEST.USE_GT_BBOX = True
    cfg.DATASET.merge_from_dict(dataset)
    cfg.TEST.merge_from_dict(test or {})
    return cfg


DB_KEYS = ('center', 'scale', 'joints_3d', 'joints_3d_vis')


def db_arrays(db, root):
    """The records of a db as the arrays the fixture stores them in."""
    out = {k: np.stack([rec[k] for rec in db]) for k in DB_KEYS}
    out['image'] = np.array([os.path.relpath(rec['image'], root) for rec in db])
    if db and 'score' in db[0]:
        out['score'] = np.array([rec['score'] for rec in db], np.float64)
    else:
        out['filename'] = np.array([rec['filename'] for rec in db])
        out['imgnum'] = np.array([rec['imgnum'] for rec in db])
    return out


RESULT_KEYS = ('image_id', 'category_id', 'keypoints', 'score', 'center', 'scale')


def results_arrays(results):
    """A results list (as read back from the results file) as arrays."""
    return {'image_id': np.array([r['image_id'] for r in results], np.int64),
            'category_id': np.array([r['category_id'] for r in results], np.int64),
            'keypoints': np.array([r['keypoints'] for r in results], np.float64).reshape(len(results), -1),
            'score': np.array([r['score'] for r in results], np.float64),
            'center': np.array([r['center'] for r in results], np.float64).reshape(len(results), 2),
            'scale': np.array([r['scale'] for r in results], np.float64).reshape(len(results), 2)}
