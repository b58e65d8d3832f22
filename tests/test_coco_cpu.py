"""The COCO dataset class on the host (lib/dataset/coco.py, lib/dataset/coco_eval.py, lib/config.py; no GPU): the `db`
records against the reference's own (tests/golden/coco_ref.npz), the configuration keys, the numpy restatement of
rescoring + OKS NMS (tests/_coco_ref.py) against the reference's `oks_nms` / `soft_oks_nms` / `oks_iou`, the argument checks of
fpd_oks_nms, and the keypoint AP / AR table on cases small enough to derive by hand (every expected value is derived in a
comment next to it).

The hand-derived cases use people with ONE annotated joint, the left eye (sigma 0.025, so (2 sigma)^2 = 0.0025): the OKS of
a detection with such a gt is exp(-d^2 / 0.0025 / area / 2) for the distance d between the two left eyes."""
import argparse
import os

import numpy as np
import pytest

from tests import _coco_ref as C
from tests import _coco_tree as T

G = T.load_golden()


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return T.write_tree(tmp_path_factory.mktemp('coco'), G, images=False)


# ---- the records ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case,image_set,is_train,use_gt', [('train', 'train2017', True, False), ('val_gt', 'val2017', False, True),
                                                            ('val_det', 'val2017', False, False)])
def test_db_records_equal_the_reference_bit_for_bit(tree, case, image_set, is_train, use_gt):
    from fpd_amd.lib.dataset import COCODataset
    ds = COCODataset(T.make_cfg(tree, test={'USE_GT_BBOX': use_gt}), tree, image_set, is_train)
    got = T.db_arrays(ds.db, tree)
    want = {k[len('db/%s/' % case):]: v for k, v in G.items() if k.startswith('db/%s/' % case)}
    assert sorted(got) == sorted(want) and len(ds) == len(want['image']) == {'train': 9, 'val_gt': 9, 'val_det': 12}[case]
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert got['center'].dtype == got['scale'].dtype == np.float32 and got['joints_3d'].dtype == np.float64
    for rec in ds.db:
        assert sorted(rec) == (['center', 'image', 'joints_3d', 'joints_3d_vis', 'scale', 'score'] if case == 'val_det' else
                               ['center', 'filename', 'image', 'imgnum', 'joints_3d', 'joints_3d_vis', 'scale'])
    if case == 'val_det':
        assert (got['joints_3d_vis'] == 1).all() and (got['joints_3d'] == 0).all() and got['score'].min() >= 0.1
    else:
        assert set(np.unique(got['joints_3d_vis'])) == {0.0, 1.0}          # visibility 2 became 1


def test_tables_and_image_paths(tree):
    from fpd_amd.lib.dataset import COCODataset
    ds = COCODataset(T.make_cfg(tree), tree, 'val2017', False)
    assert ds.num_joints == 17 and ds.flip_pairs == [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
    assert ds.upper_body_ids == tuple(range(11)) and ds.lower_body_ids == tuple(range(11, 17)) and ds.parent_ids is None
    assert ds.joints_weight.dtype == np.float32 and ds.joints_weight.shape == (17, 1)
    assert ds.joints_weight.reshape(-1).tolist() == [1, 1, 1, 1, 1, 1, 1, np.float32(1.2), np.float32(1.2), 1.5, 1.5, 1, 1,
                                                      np.float32(1.2), np.float32(1.2), 1.5, 1.5]
    assert ds.classes == ['__background__', 'person'] and ds.image_set_index == list(T.IMAGE_IDS)      # file order
    assert ds.image_path_from_index(139) == os.path.join(tree, 'images', 'val2017', '000000000139.jpg')
    ds.image_set = 'val2014'
    assert ds.image_path_from_index(139) == os.path.join(tree, 'images', 'val2014', 'COCO_val2014_000000000139.jpg')
    test = COCODataset(T.make_cfg(tree), tree, T.TEST_SET, False)                  # image_info_<set>.json, no annotations
    assert len(test.db) == 0 and test.image_path_from_index(7) == os.path.join(tree, 'images', 'test2017', '000000000007.jpg')
    # the annotation index: file order, non-crowd filter
    idx = ds.coco
    assert idx.image_ids() == list(T.IMAGE_IDS) and idx.category_ids() == [1] and idx.category_names() == ['person']
    crowd_image = T.IMAGE_IDS[int(G['in_ann_image'][3])]
    assert [a['id'] for a in idx.image_annotations(crowd_image)] == [102, 103, 104]
    assert [a['id'] for a in idx.image_annotations(crowd_image, iscrowd=False)] == [102, 104]


def test_zip_and_select_data_raise(tree):
    from fpd_amd.lib.dataset import COCODataset
    from fpd_amd.runtime import FpdError
    with pytest.raises(FpdError, match='zip'):
        COCODataset(T.make_cfg(tree, DATA_FORMAT='zip'), tree, 'val2017', False)
    with pytest.raises(FpdError, match='SELECT_DATA'):
        COCODataset(T.make_cfg(tree, SELECT_DATA=True), tree, 'train2017', True)
    with pytest.raises(FpdError, match='COCO_BBOX_FILE'):
        COCODataset(T.make_cfg(tree, test={'USE_GT_BBOX': False, 'COCO_BBOX_FILE': os.path.join(tree, 'nope.json')}), tree, 'val2017', False)


COCO_YAML = """
DATASET:
  COLOR_RGB: true
  DATASET: 'coco'
  DATA_FORMAT: jpg
  FLIP: true
  NUM_JOINTS_HALF_BODY: 8
  PROB_HALF_BODY: 0.3
  ROOT: 'data/coco'
  ROT_FACTOR: 45
  SCALE_FACTOR: 0.35
  TEST_SET: 'val2017'
  TRAIN_SET: 'train2017'
MODEL:
  NUM_JOINTS: 17
  IMAGE_SIZE:
  - 192
  - 256
  HEATMAP_SIZE:
  - 48
  - 64
TEST:
  BATCH_SIZE_PER_GPU: 32
  COCO_BBOX_FILE: 'data/coco/person_detection_results/COCO_val2017_detections_AP_H_56_person.json'
  BBOX_THRE: 1.0
  IMAGE_THRE: 0.0
  IN_VIS_THRE: 0.2
  MODEL_FILE: ''
  NMS_THRE: 1.0
  OKS_THRE: 0.9
  USE_GT_BBOX: true
  FLIP_TEST: true
  POST_PROCESS: true
"""


def test_config_defaults_and_a_coco_yaml(tmp_path):
    from fpd_amd.lib.config import _defaults, update_config
    cfg = _defaults()
    want = {'USE_GT_BBOX': False, 'IMAGE_THRE': 0.1, 'NMS_THRE': 0.6, 'SOFT_NMS': False, 'OKS_THRE': 0.5, 'IN_VIS_THRE': 0.0,
            'COCO_BBOX_FILE': '', 'BBOX_THRE': 1.0}
    for k, v in want.items():
        assert cfg.TEST[k] == v and type(cfg.TEST[k]) is type(v), k
    assert cfg.RANK == 0
    path = tmp_path / 'coco.yaml'
    path.write_text(COCO_YAML)
    update_config(cfg, argparse.Namespace(cfg=str(path), opts=['TEST.SOFT_NMS', 'True']))
    assert cfg.DATASET.DATASET == 'coco' and cfg.TEST.USE_GT_BBOX is True and cfg.TEST.SOFT_NMS is True
    assert (cfg.TEST.OKS_THRE, cfg.TEST.IN_VIS_THRE, cfg.TEST.IMAGE_THRE, cfg.TEST.NMS_THRE) == (0.9, 0.2, 0.0, 1.0)
    assert cfg.TEST.COCO_BBOX_FILE.endswith('AP_H_56_person.json') and cfg.TEST.SHIFT_HEATMAP is False


# ---- rescoring + NMS: the restatement against the reference's functions -------------------------------------------------

@pytest.mark.parametrize('p', T.NMS_SIZES)
def test_restatement_reproduces_the_reference_nms(p):
    kpts, area, box = G['nms/%d/kpts' % p], G['nms/%d/area' % p], G['nms/%d/box_score' % p]
    thresh, vis = float(G['nms/thresh']), float(G['nms/in_vis_thre'])
    score = C.rescore(kpts, box, vis)
    assert score.dtype == np.float64 and np.array_equal(score, G['nms/%d/score' % p])              # bit for bit
    assert len(set(score.tolist())) == p                                                            # tie-free
    assert C.hard_nms(kpts, area, score, thresh) == G['nms/%d/hard' % p].tolist()
    assert C.soft_nms(kpts, area, score, thresh) == G['nms/%d/soft' % p].tolist()
    top = int(np.argmax(score))
    want = G['nms/%d/oks_top' % p]
    assert want[top] == 1.0 and np.abs(C.oks(kpts, area, top) - want).max() <= 1e-12 * want.max()
    if p >= 17:
        kept = len(G['nms/%d/hard' % p])
        assert kept * 5 >= p and (p - kept) * 5 >= p
    s2, keep, n_keep = C.nms_pictures(kpts, area, box, [0, p], vis, thresh, False)
    assert np.array_equal(s2, score) and keep[:n_keep[0]].tolist() == G['nms/%d/hard' % p].tolist() and (keep[n_keep[0]:] == -1).all()


def test_oks_nms_entry_point_checks_its_arguments_without_a_device():
    from fpd_amd import runtime as R
    lib = R.lib()
    err = lambda: lib.fpd_last_error().decode()  # noqa: E731
    assert hasattr(lib, 'fpd_oks_nms') and lib.fpd_abi_sizeof(b'fpd_oks_nms_t') == R.C.sizeof(R.OksNmsT)
    a = R.OksNmsT()
    assert lib.fpd_oks_nms(a, None) != 0 and 'null' in err()
    a.offsets = a.n_keep = a.sigmas = 64                       # never dereferenced by the checks below
    a.J = 65
    assert lib.fpd_oks_nms(a, None) != 0 and 'J=65' in err()
    a.J, a.soft = 17, 2
    assert lib.fpd_oks_nms(a, None) != 0 and '0 or 1' in err()
    a.soft, a.P_total, a.n_img = 0, 4, 1
    assert lib.fpd_oks_nms(a, None) != 0 and 'per-person' in err()
    a.P_total, a.n_img, a.oks_thre = 0, 0, float('nan')
    assert lib.fpd_oks_nms(a, None) != 0 and 'threshold' in err()
    a.oks_thre = 0.9
    assert lib.fpd_oks_nms(a, None) == 0                        # no picture: nothing is launched


def test_wrappers_refuse_in_vis_thre():
    from fpd_amd.lib.nms import nms
    from fpd_amd.runtime import FpdError
    person = {'keypoints': np.zeros((17, 3), np.float32), 'area': 1.0, 'score': 1.0}
    for call in (lambda: nms.oks_nms([person], 0.9, None, 0.2), lambda: nms.soft_oks_nms([person], 0.9, in_vis_thre=0.2),
                 lambda: nms.oks_iou(np.zeros(51), np.zeros((1, 51)), 1.0, np.ones(1), in_vis_thre=0.0)):
        with pytest.raises(FpdError, match='in_vis_thre'):
            call()
    assert nms.oks_nms([], 0.9) == [] and len(nms.soft_oks_nms([], 0.9)) == 0


# ---- keypoint AP / AR on hand-derived cases -------------------------------------------------------------------------------

EYE = 1                                         # left eye: sigma 0.025


def eye_gt(image_id, x, y, area=2500.0, iscrowd=0, annotated=True):
    """A person whose only annotated joint is the left eye at (x, y); annotated False: no joint at all (num_keypoints 0)
    and a 10 x 10 box at (x, y)."""
    k = np.zeros((17, 3))
    if annotated:
        k[EYE] = (x, y, 2)
    return {'image_id': image_id, 'category_id': 1, 'keypoints': k.reshape(-1).tolist(), 'num_keypoints': int(annotated),
            'area': area, 'bbox': [x, y, 10.0, 10.0], 'iscrowd': iscrowd}


def eye_dt(image_id, x, y, score, extent=(40.0, 50.0)):
    """A detection whose left eye is at (x, y); its other joints span a box of `extent` with the eye at one corner, so
    its own area is extent[0] * extent[1] (2000: medium)."""
    k = np.zeros((17, 3))
    k[:, 0], k[:, 1] = x, y
    k[0, 0:2] = (x + extent[0], y + extent[1])
    k[:, 2] = 0.9
    return {'image_id': image_id, 'category_id': 1, 'keypoints': k.reshape(-1).tolist(), 'score': score}


def stats(gts, dts):
    from fpd_amd.lib.dataset import coco_eval
    return coco_eval.evaluate_keypoints(gts, dts, sorted({g['image_id'] for g in gts}), [1])


def test_eval_parameters():
    from fpd_amd.lib.dataset import coco_eval as E
    assert np.array_equal(E.OKS_THRS, np.linspace(.5, .95, 10)) and np.array_equal(E.REC_THRS, np.linspace(0, 1, 101))
    assert E.MAX_DETS == 20 and E.AREA_RANGES == ((0, 1e10), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))
    assert np.array_equal(E.SIGMAS, C.SIGMAS) and E.SIGMAS[EYE] * 2 == 0.05
    assert E.STAT_NAMES == ('AP', 'Ap .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)')
    assert E.detection_area(eye_dt(1, 5, 7, 0.5)['keypoints']) == 2000.0


def test_eval_detections_equal_to_the_ground_truth_score_one():
    """Three medium people (full 17-joint poses, area 2500) over two pictures, each detected exactly, distinct scores.
    Every OKS is exp(0) = 1 >= every threshold, so at each threshold tp = [1, 2, 3], fp = [0, 0, 0], npig = 3:
    precision = tp / (tp + 2^-52) = [1 - 2^-52.., 1, 1] and the pass from the right lifts the first entry to 1;
    recall = [1/3, 2/3, 1] reaches every recall threshold, so all 101 samples are 1 and the recall entry is 1.
    All, .5, .75 and medium: 1.  No gt is large: npig = 0 there, AP(L) = AR(L) = -1."""
    rng = np.random.default_rng(3)
    gts, dts = [], []
    for n, (img, score) in enumerate(((7, 0.9), (7, 0.6), (9, 0.75))):
        k = np.zeros((17, 3))
        k[:, 0:2] = rng.uniform(0, 60, (17, 2)) + 200 * n
        k[:, 2] = 2
        gts.append({'image_id': img, 'category_id': 1, 'keypoints': k.reshape(-1).tolist(), 'num_keypoints': 17, 'area': 2500.0,
                    'bbox': [200.0 * n, 200.0 * n, 60.0, 60.0], 'iscrowd': 0})
        dts.append({'image_id': img, 'category_id': 1, 'keypoints': k.reshape(-1).tolist(), 'score': score})
    s = stats(gts, dts)
    assert s.tolist() == [1.0, 1.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0, -1.0]


def test_eval_a_far_detection_in_front_halves_the_precision():
    """One picture, two medium gts A and B; a detection far from both (OKS: d^2 = 500^2 gives e = 2e4, exp(-e) = 0) with the
    higher score and one exactly on A with the lower.  In score order: [miss, hit].  At every threshold tp = [0, 1],
    fp = [1, 1], npig = 2: recall = [0, 0.5], precision = [0, 1 / (2 + 2^-52)] = [0, 0.5], lifted from the right to
    [0.5, 0.5].  The recall thresholds 0 .. 0.50 (51 of the 101) are reached, the rest sample 0: AP = 51 * 0.5 / 101; the
    recall entry is 0.5.  The far detection's own area is 2000 (medium) and both gts are medium: the medium figures are
    the same; nothing is large."""
    gts = [eye_gt(1, 100, 100), eye_gt(1, 300, 100)]
    dts = [eye_dt(1, 600, 100, 0.9), eye_dt(1, 100, 100, 0.4)]
    ap = 51 * 0.5 / 101
    assert stats(gts, dts).tolist() == pytest.approx([ap, ap, ap, ap, -1, 0.5, 0.5, 0.5, 0.5, -1], abs=1e-12)


def test_eval_an_unmatched_detection_outside_the_area_range_is_ignored():
    """The same picture, but the far detection spans 100 x 100 = 10000 (large).  Over all areas nothing changes
    (AP = 51 * 0.5 / 101).  In the medium range it is unmatched and its own area is outside: ignored, neither tp nor fp:
    tp = [0, 1], fp = [0, 0], precision = [0 / 2^-52, 1 / (1 + 2^-52)] = [0, 1 - 2^-52], lifted to 1 - 2^-52 in front:
    AP(M) = 51 / 101 (within 1e-12), AR(M) = 0.5.  In the large range both gts are ignored: -1."""
    gts = [eye_gt(1, 100, 100), eye_gt(1, 300, 100)]
    dts = [eye_dt(1, 600, 100, 0.9, extent=(100.0, 100.0)), eye_dt(1, 100, 100, 0.4)]
    ap = 51 * 0.5 / 101
    assert stats(gts, dts).tolist() == pytest.approx([ap, ap, ap, 51 / 101, -1, 0.5, 0.5, 0.5, 0.5, -1], abs=1e-12)


def test_eval_crowd_and_unannotated_people_count_neither_way():
    """Two ordinary gts, each detected exactly (scores 0.9, 0.85); a crowd gt with two detections exactly on it (0.8, 0.7):
    a crowd may be matched again and again, both detections inherit its ignore flag; a gt with num_keypoints 0 whose box
    [400, 100, 10, 10] doubled about itself is [390, 420] x [90, 120], and a detection with every joint inside it
    (0.6): dx = dy = 0 for all 17 joints, OKS = 1, matched to an ignored gt, ignored.  What counts: tp = [1, 2], fp = 0,
    npig = 2 -> precision [1 - 2^-52.., 1] lifted to 1, recall 1: every populated figure is exactly 1.  Were the crowd or the
    unannotated person counted as gts, recall would drop below 1; were their detections false positives, precision would."""
    gts = [eye_gt(1, 100, 100), eye_gt(1, 200, 100), eye_gt(1, 300, 100, iscrowd=1), eye_gt(1, 400, 100, annotated=False)]
    dts = [eye_dt(1, 100, 100, 0.9), eye_dt(1, 200, 100, 0.85), eye_dt(1, 300, 100, 0.8), eye_dt(1, 300, 100, 0.7),
           eye_dt(1, 395, 95, 0.6, extent=(20.0, 20.0))]
    assert stats(gts, dts).tolist() == [1.0, 1.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0, -1.0]


def test_eval_a_taken_gt_is_not_matched_twice():
    """gts A, B; detections: exactly A (0.9), exactly A again (0.8), exactly B (0.7).  The second finds A taken and B at OKS 0:
    a false positive.  tp = [1, 1, 2], fp = [0, 1, 1], npig = 2: recall = [.5, .5, 1], precision = [1-, 1/2, 2/3] lifted
    to [1-, 2/3, 2/3].  Recall thresholds 0 .. 0.50 (51) sample the first entry (1 within 2^-52), 0.51 .. 1 (50) the
    third: AP = (51 + 50 * 2/3) / 101; recall entry 1."""
    gts = [eye_gt(1, 100, 100), eye_gt(1, 300, 100)]
    dts = [eye_dt(1, 100, 100, 0.9), eye_dt(1, 100, 100, 0.8), eye_dt(1, 300, 100, 0.7)]
    ap = (51 + 50 * 2 / 3) / 101
    assert stats(gts, dts).tolist() == pytest.approx([ap, ap, ap, ap, -1, 1, 1, 1, 1, -1], abs=1e-12)


def test_eval_the_scan_stops_at_the_ignored_gts_once_a_counting_match_is_in_hand():
    """An ordinary gt N with its eye at (100, 100) and a crowd C with its eye at (101, 102), both of area 2500; one detection
    exactly on C.  Against N: d^2 = 1 + 4 = 5, e = 5 / 0.0025 / 2500 / 2 = 0.4, OKS = exp(-0.4) = 0.6703; against C: 1.
    Thresholds 0.5 .. 0.65 (4 of 10): N qualifies, and the scan stops before the crowd although its OKS is higher: a true
    positive: precision 1 - 2^-52 at all 101 recall thresholds, recall 1.  Thresholds 0.7 .. 0.95 (6): N does not qualify,
    the crowd takes the detection, which is then ignored: tp = fp = [0], precision 0 / 2^-52 = 0, recall 0.
    AP = AR = 4 / 10; at .5: 1; at .75: 0."""
    gts = [eye_gt(1, 100, 100), eye_gt(1, 101, 102, iscrowd=1)]
    dts = [eye_dt(1, 101, 102, 0.9)]
    assert np.exp(-0.4) == pytest.approx(0.6703, abs=1e-4)
    assert stats(gts, dts).tolist() == pytest.approx([0.4, 1, 0, 0.4, -1, 0.4, 1, 0, 0.4, -1], abs=1e-12)


def test_eval_a_detection_takes_the_gt_it_fits_best_not_the_first_that_qualifies():
    """gts N1 (eye at (100, 100), area 9000) and N2 (eye at (101, 102), area 1600), both medium; detections D1 exactly on N2
    (0.9) and D2 exactly on N1 (0.8).  D1 against N1: e = 5 / 0.0025 / 9000 / 2 = 0.111, OKS 0.895 -- N1 qualifies first up to
    threshold 0.85, but N2 (OKS 1) is the better fit and is taken.  D2 then finds N1 free: OKS 1.  Both are true
    positives at every threshold: everything populated is exactly 1.  (Taking the first gt that qualifies would leave D2
    with N2 at OKS exp(-5 / 0.0025 / 1600 / 2) = 0.535: a miss from threshold 0.55 on.)"""
    gts = [eye_gt(1, 100, 100, area=9000.0), eye_gt(1, 101, 102, area=1600.0)]
    dts = [eye_dt(1, 101, 102, 0.9), eye_dt(1, 100, 100, 0.8)]
    assert stats(gts, dts).tolist() == [1.0, 1.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0, -1.0]


def test_eval_the_21st_detection_of_a_picture_is_cut():
    """21 gts 100 px apart in one picture, each detected exactly, scores 0.95, 0.94, ...: the picture's detections are cut
    to the 20 best, the 21st person is missed.  tp = 1 .. 20, fp = 0, npig = 21: precision 1 (lifted), recall k / 21 up to
    20/21 = 0.952: the recall thresholds 0 .. 0.95 (96 of 101) are reached.  AP = 96 / 101, AR = 20 / 21."""
    gts = [eye_gt(1, 100 * k, 50) for k in range(21)]
    dts = [eye_dt(1, 100 * k, 50, 0.95 - 0.01 * k) for k in range(21)]
    ap, ar = 96 / 101, 20 / 21
    assert stats(gts, dts).tolist() == pytest.approx([ap, ap, ap, ap, -1, ar, ar, ar, ar, -1], abs=1e-12)


def test_eval_large_people_and_a_picture_without_detections():
    """Picture 1: a large gt (area 10000) detected exactly; picture 2: a medium gt and no detection.  All areas: tp = [1],
    npig = 2, recall [0.5], precision [1 - 2^-52]: 51 recall thresholds reached: AP = 51 / 101, AR = 0.5.  Large: npig = 1,
    tp = [1]: AP(L) = AR(L) = 1.  Medium: the detection matched an ignored (large) gt and is ignored: tp = fp = [0]:
    AP(M) = AR(M) = 0."""
    gts = [eye_gt(1, 100, 100, area=10000.0), eye_gt(2, 100, 100)]
    dts = [eye_dt(1, 100, 100, 0.9)]
    ap = 51 / 101
    assert stats(gts, dts).tolist() == pytest.approx([ap, ap, ap, 0, 1, 0.5, 0.5, 0.5, 0, 1], abs=1e-12)
