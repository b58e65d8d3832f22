"""The device AP table's host side (lib/dataset/coco_eval.py pack_ground_truth / group_detections, the argument checks of
fpd_coco_match and fpd_coco_accumulate) and the conditions the generated pictures of tests/_coco_eval_cases.py must meet for
tests/test_coco_eval_gpu.py to mean something; no GPU."""
import numpy as np
import pytest

from tests import _coco_eval_cases as K


@pytest.fixture(scope='module')
def pictures():
    return K.host_case_set()


def by_id(pictures, name):
    return pictures[sorted(K.case_set()[2]).index(K.PIC[name])]


def test_margins_keep_the_last_bits_of_an_oks_from_deciding_a_match(pictures):
    """Every picture of the set: no OKS (exactly 1 aside) within 1e-9 of a threshold, no two different OKS values of one
    detection within 1e-9 of each other -- seven orders of magnitude above what the device's exp and summation order can
    move a value (a few 1e-14, tests/test_coco_eval_gpu.py)."""
    thr_gap, row_gap = K.margins(pictures)
    print('smallest |oks - t| %.3e, smallest gap in a row %.3e' % (thr_gap, row_gap))
    assert thr_gap >= 1e-9 and row_gap >= 1e-9


def test_the_set_holds_every_situation(pictures):
    from fpd_amd.lib.dataset import coco_eval as E
    assert len(pictures) == 40
    g, d, oks, res = by_id(pictures, 'gts_only')
    assert len(g) == 4 and not d and res[0] is not None and res[0][0].shape == (10, 0)
    g, d, oks, res = by_id(pictures, 'dts_only')
    assert not g and len(d) == 5 and not res[0][0].any()
    g, d, oks, res = by_id(pictures, 'empty')
    assert not g and not d and res == [None, None, None]
    assert len(by_id(pictures, 'twenty')[1]) == 20 and len(by_id(pictures, 'one_dt')[1]) == 1
    # the cut: 25 results of the picture in the file, the 20 best kept
    in_file = [x for x in K.case_set()[1] if x['image_id'] == K.PIC['twenty_five']]
    g, d, oks, res = by_id(pictures, 'twenty_five')
    assert len(in_file) == 25 and len(d) == 20 and min(x['score'] for x in d) >= sorted(x['score'] for x in in_file)[5]
    # a crowd matched by several detections: more matched-and-ignored detections than ignored gts
    g, d, oks, res = by_id(pictures, 'crowd')
    assert sum(x['iscrowd'] for x in g) == 1 and sum(x['_ignore'] for x in g) == 1
    assert int((res[0][0][0] & res[0][1][0]).sum()) >= 3
    assert len({x['score'] for x in d}) < len(d)                                    # and equal scores within a picture
    # a gt without an annotated joint: the box-distance branch, with values of 1 and below 1
    g, d, oks, res = by_id(pictures, 'blank')
    assert g[0]['num_keypoints'] == 0 and (oks == 1).any() and ((oks < 1) & (oks > 0.01)).any()
    # two byte-identical gts: equal columns, a tie at a value that passes the lowest threshold
    g, d, oks, res = by_id(pictures, 'twins')
    assert len(g) == 2 and {k: v for k, v in g[0].items()} == {k: v for k, v in g[1].items()}
    assert np.array_equal(oks[:, 0], oks[:, 1]) and oks.max() >= 0.5
    # areas exactly on both edges of the medium range count in it, and in 'large' for 96^2
    g, d, oks, res = by_id(pictures, 'edges')
    assert [x['area'] for x in g] == [1024.0, 9216.0] and not res[1][2].any() and res[2][2].tolist() == [False, True]      # (match_picture returns the flags counting-first)
    # the scan stops: at threshold 0.5 the detection takes the counting gt (OKS 0.67) although the crowd fits better (1)
    g, d, oks, res = by_id(pictures, 'scan_stops')
    assert oks[0, 0] < oks[0, 1] == 1.0 and res[0][0][0, 0] and not res[0][1][0, 0] and res[0][1][9, 0]
    # best fit, not first fit: the first gt qualifies at 0.5 (0.895) and the second is taken (1), so the second detection finds the first free
    g, d, oks, res = by_id(pictures, 'best_fit')
    assert 0.5 <= oks[0, 0] < oks[0, 1] and res[0][0][7].all() and not res[0][1].any()
    # more gts than the kernel's register bit mask holds
    g, d, oks, res = by_id(pictures, 'big')
    assert len(g) == K.BIG_G == 200 > K.FAST_G == 64 and len(d) == 20 and res[0][0].any() and not res[0][0].all()
    # across the set: every flag combination, all three area ranges populated, people in every range, score ties across pictures
    m, ig, counted, scores, area = K.flag_tables(pictures)
    for r in range(3):
        assert counted[r].sum() > 0
        for want in ((1, 0), (1, 1), (0, 0), (0, 1))[:4 if r else 3]:        # (nothing is outside the range 'all')
            assert ((m[r] == want[0]) & (ig[r] == want[1])).any(), (r, want)
    assert (area < 1024).any() and ((area > 1024) & (area < 9216)).any() and (area > 9216).any()
    assert len(set(scores.tolist())) < len(scores)
    assert any(0 < len(p[0]) <= K.FAST_G and len(p[0]) * len(p[1]) > 0 for p in pictures)
    assert E.MAX_DETS == 20


def test_packing_and_grouping_agree_with_the_dict_based_grouping(pictures):
    """pack_ground_truth and group_detections against evaluate_keypoints' own grouping (restated in host_pictures): the same
    people per picture in the same order -- pictures without gts, without detections, 25 detections cut to the 20 best, equal
    scores in file order."""
    from fpd_amd.lib.dataset import coco_eval as E
    gts, dts, image_ids = K.case_set()
    shuffled = list(reversed(image_ids)) + image_ids[:3]                           # any order, repeats: the ids are sorted and made unique
    packed = E.pack_ground_truth(gts + [dict(gts[0], category_id=2), dict(gts[0], image_id=999)], shuffled, 1)
    assert packed['image_ids'].tolist() == image_ids and packed['gt_offsets'].dtype == np.int32
    assert packed['gt_kpts'].dtype == np.float64 and packed['gt_flags'].dtype == np.uint8
    rows, dt_offsets = E.group_detections(packed['image_ids'], [d['image_id'] for d in dts] + [999], [d['score'] for d in dts] + [0.99])
    assert dt_offsets.dtype == np.int32 and dt_offsets[-1] == len(rows) and packed['gt_offsets'][-1] == len(gts)
    for i, (g, d, _, _) in enumerate(pictures):
        a, b = packed['gt_offsets'][i:i + 2]
        assert b - a == len(g)
        for n, x in enumerate(g):
            assert packed['gt_kpts'][a + n].reshape(-1).tolist() == x['keypoints'] and packed['gt_area'][a + n] == x['area']
            assert packed['gt_bbox'][a + n].tolist() == x['bbox']
            assert packed['gt_flags'][a + n] == int(x['_ignore']) | int(bool(x['iscrowd'])) << 1
        a, b = dt_offsets[i:i + 2]
        assert [int(r) + 1 for r in rows[a:b]] == [x['id'] for x in d]               # the host numbers the results from 1 in file order
    assert (np.diff(dt_offsets) == 20).sum() == 3 and (np.diff(dt_offsets) == 0).any() and (np.diff(packed['gt_offsets']) == 0).any()
    # equal scores keep file order; the 21st is cut by score, not by position
    ids = [5] * 23 + [4]
    scores = [0.5] * 21 + [0.9, 0.1, 0.5]
    rows, off = E.group_detections([4, 5], ids, scores)
    assert rows.tolist() == [23, 21] + list(range(19)) and off.tolist() == [0, 1, 21]
    empty = E.pack_ground_truth([], [3, 1], 1)
    assert empty['gt_offsets'].tolist() == [0, 0, 0] and empty['gt_kpts'].shape == (0, 0, 3)
    rows, off = E.group_detections([], [7], [0.5])
    assert rows.size == 0 and off.tolist() == [0]


def test_entry_points_check_their_arguments_without_a_device():
    from fpd_amd import runtime as R
    from fpd_amd.lib.dataset import coco_eval as E
    lib = R.lib()
    err = lambda: lib.fpd_last_error().decode()  # noqa: E731
    assert lib.fpd_abi_version() == 2
    # the struct sizes: a host built against another layout fails at load (runtime.lib), and here
    assert lib.fpd_abi_sizeof(b'fpd_coco_match_t') == R.C.sizeof(R.CocoMatchT) == 288
    assert lib.fpd_abi_sizeof(b'fpd_coco_accum_t') == R.C.sizeof(R.CocoAccumT) == 88
    a = R.CocoMatchT()
    assert lib.fpd_coco_match(a, None) != 0 and 'null' in err()
    a.gt_offsets = a.dt_offsets = a.oks_offsets = a.status = a.sigmas = a.gt_counted = 64      # never dereferenced by the checks below
    a.J = 65
    assert lib.fpd_coco_match(a, None) != 0 and 'J=65' in err()
    a.J, a.n_img = 17, -1
    assert lib.fpd_coco_match(a, None) != 0 and 'negative' in err()
    a.n_img, a.G_total = 1, 3
    assert lib.fpd_coco_match(a, None) != 0 and 'per-gt' in err()
    a.G_total, a.D_total = 0, 2
    assert lib.fpd_coco_match(a, None) != 0 and 'per-detection' in err()
    a.D_total, a.oks_total = 0, 5
    assert lib.fpd_coco_match(a, None) != 0 and 'oks' in err()
    a.oks_total = 0
    assert lib.fpd_coco_match(a, None) != 0 and 'area range' in err()               # the ranges and thresholds are arguments
    for r, (lo, hi) in enumerate(E.AREA_RANGES):
        a.area_lo[r], a.area_hi[r] = lo, hi
    a.oks_thrs[3] = float('nan')
    assert lib.fpd_coco_match(a, None) != 0 and 'threshold 3' in err()
    a.oks_thrs[3], a.n_img = 0.65, 0
    assert lib.fpd_coco_match(a, None) == 0                                           # no picture: nothing is launched
    b = R.CocoAccumT()
    assert lib.fpd_coco_accumulate(b, None) != 0 and 'null' in err()
    b.npig = b.rec_thrs = b.precision = b.recall = b.status = 64
    assert lib.fpd_coco_accumulate(b, None) != 0 and 'n_rec=0' in err()
    b.n_rec, b.D_total = 101, -4
    assert lib.fpd_coco_accumulate(b, None) != 0 and 'negative' in err()
    b.D_total = 7
    assert lib.fpd_coco_accumulate(b, None) != 0 and 'per-detection' in err()
    # offsets that do not rise, sizes that disagree, more than one category: refused on the host before any device is touched
    packed = E.pack_ground_truth(K.case_set()[0], K.case_set()[2], 1)
    none = (np.zeros(0, np.int64), np.zeros((0, 51)), np.zeros(0))
    for bad in ([0, 6, 2, len(packed['gt_area'])], [1] + packed['gt_offsets'][1:].tolist(), packed['gt_offsets'][:-1].tolist() + [7]):
        with pytest.raises(R.FpdError, match='offsets must rise'):
            E.evaluate_arrays_device(dict(packed, gt_offsets=np.asarray(bad, np.int32)), *none)
    with pytest.raises(R.FpdError, match='sigmas'):
        E.evaluate_arrays_device(packed, *none, sigmas=E.SIGMAS[:5])
    with pytest.raises(R.FpdError, match='detections of shape'):
        E.evaluate_arrays_device(packed, np.zeros(2, np.int64), np.zeros((2, 50)), np.zeros(2))
    with pytest.raises(R.FpdError, match='one category'):
        E.evaluate_keypoints_device([], [], [1], [1, 2])
    # no picture at all: the host's answer without a launch
    assert E.evaluate_arrays_device(E.pack_ground_truth([], [], 1), *none).tolist() == [-1.0] * 10
