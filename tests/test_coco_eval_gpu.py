"""COCO keypoint AP on the MI355X (csrc/coco_eval.hip through fpd_coco_match / fpd_coco_accumulate; lib/dataset/coco_eval.py)
against the host functions of the same module, which are the expected values everywhere: every match flag, ignore flag and gt
count of every picture, area range and threshold; the OKS matrices; the precision / recall tables bit for bit; the ten
statistics bit for bit; COCODataset.evaluate with and without host_eval.

The generated pictures (tests/_coco_eval_cases.py) hold every situation of the matching, among them a picture of 200 gts: the
kernel keeps the taken flags of up to 64 gts (COCO_FAST_G) in a register bit mask and those of larger pictures in the caller's
scratch.  tests/test_coco_eval_cpu.py checks, without a GPU, that the situations are there and that no comparison of the set
hangs on the last bits of an OKS."""
import os

import numpy as np
import pytest
import torch

from tests import _coco_eval_cases as K
from tests import _coco_tree as T

pytestmark = pytest.mark.gpu

# |device oks - picture_oks|: every term exp(-e) is <= 1 and within 1 ulp on either side, and the (at most) 17 terms are summed in
# another order than numpy's pairwise sum: < 17 * 2^-52 + 16 * 17 * 2^-53, a few 1e-14, before the division by the joint count
OKS_TOL = 1e-13


@pytest.fixture(scope='module')
def host():
    pictures = K.host_case_set()
    return pictures, K.flag_tables(pictures)


_RUNS = {}


def device_run(grid):
    """fpd_coco_match over the generated set -> numpy arrays; made once per grid, shared, never modified."""
    if grid not in _RUNS:
        from fpd_amd.lib.dataset import coco_eval as E
        gts, dts, image_ids = K.case_set()
        t, packed, rows, dt_offsets = K.device_inputs(gts, dts, image_ids)
        out = E.match_device(t, grid=grid)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items() if k != 'scratch'}
        got.update(oks_offsets=t['oks_offsets'].cpu().numpy(), dt_offsets=dt_offsets, gt_offsets=packed['gt_offsets'])
        _RUNS[grid] = got
    return _RUNS[grid]


@pytest.mark.parametrize('grid', [0, 3])
def test_match_equals_match_picture_on_every_picture(host, grid):
    """grid 0: a workgroup per picture; grid 3: each workgroup owns 13 or 14 pictures, among them pictures of either path."""
    pictures, (matched, ignored, counted, scores, area) = host
    got = device_run(grid)
    assert (got['status'] == 0).all()
    assert got['dt_area'].dtype == np.float64 and np.array_equal(got['dt_area'], area)                  # bit for bit
    assert np.array_equal(got['gt_counted'], counted)
    worst = 0.0
    for i, (g, d, oks, res) in enumerate(pictures):
        a, b = got['dt_offsets'][i:i + 2]
        assert b - a == len(d) and got['gt_offsets'][i + 1] - got['gt_offsets'][i] == len(g)
        o = got['oks'][got['oks_offsets'][i]:got['oks_offsets'][i + 1]].reshape(len(d), len(g))
        if o.size:
            worst = max(worst, float(np.abs(o - oks).max()))
        for r in range(3):
            assert np.array_equal(got['matched'][r, :, a:b], matched[r, :, a:b]), (i, r)
            assert np.array_equal(got['dt_ignored'][r, :, a:b], ignored[r, :, a:b]), (i, r)
    print('largest |device oks - picture_oks| %.3e over %d pictures' % (worst, len(pictures)))
    assert worst <= OKS_TOL
    if grid:
        first = device_run(0)
        for k in ('matched', 'dt_ignored', 'gt_counted', 'dt_area', 'oks', 'status'):
            assert np.array_equal(got[k], first[k]), k


def _accumulate_case(d_total, seed):
    """Flags made on the host for `d_total` detections over pictures of 0..6 detections -> (per area range the per-picture
    tuples coco_eval.accumulate takes, the flag tables, scores, npig).  Range 0: threshold 0 matches everything and npig equals
    the detections, so its recall reaches 1; the other thresholds match about a third, so theirs never reaches the upper recall
    points.  Range 1: some ignored detections, npig three times the detections.  Range 2: every gt ignored, npig = 0.  Scores
    have two decimals: ties within and across pictures."""
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < d_total:
        sizes.append(min(int(rng.integers(0, 7)), d_total - sum(sizes)))
    sizes += [0, 0]
    matched = (rng.uniform(size=(3, 10, d_total)) < 0.35).astype(np.uint8)
    ignored = (rng.uniform(size=(3, 10, d_total)) < 0.2).astype(np.uint8)
    matched[0, 0], ignored[0] = 1, 0
    scores = np.round(rng.uniform(0.05, 1.0, d_total), 2)
    per_area, npig = [], []
    for r in range(3):
        res, at = [], 0
        for i, s in enumerate(sizes):
            gi = [np.zeros(s if d_total else 2, bool), np.zeros(3 * s + (i == 0), bool), np.ones(2, bool)][r]      # the picture's gts, ignored or not
            res.append((matched[r, :, at:at + s].astype(bool), ignored[r, :, at:at + s].astype(bool), gi, scores[at:at + s]))
            at += s
        per_area.append(res)
        npig.append(int(sum(np.count_nonzero(~x[2]) for x in res)))
    return per_area, matched, ignored, scores, npig


@pytest.mark.parametrize('d_total', [0, 1, 255, 256, 257, 5000])
def test_accumulate_equals_the_host_bit_for_bit(d_total):
    from fpd_amd.lib.dataset import coco_eval as E
    per_area, matched, ignored, scores, npig = _accumulate_case(d_total, 7 + d_total)
    assert npig[2] == 0 and npig[1] > 0 and npig[0] == (d_total if d_total else 2 * len(per_area[0]))
    assert d_total < 2 or len(set(scores.tolist())) < d_total
    dev = torch.device('cuda')
    order = torch.sort(torch.from_numpy(scores).to(dev), stable=True, descending=True).indices.to(torch.int32)
    precision, recall, status = E.accumulate_device(torch.from_numpy(matched).to(dev), torch.from_numpy(ignored).to(dev), order,
                                                    torch.tensor(npig, dtype=torch.int32, device=dev), torch.from_numpy(E.REC_THRS).to(dev))
    precision, recall, status = precision.cpu().numpy(), recall.cpu().numpy(), status.cpu().numpy()
    assert (status == 0).all() and precision.shape == (10, 101, 3) and recall.shape == (10, 3)
    for r in range(3):
        want_p, want_r = E.accumulate(per_area[r])
        assert np.array_equal(precision[:, :, r], want_p) and np.array_equal(recall[:, r], want_r), r
    assert (precision[:, :, 2] == -1).all() and (recall[:, 2] == -1).all()
    if d_total:
        assert recall[0, 0] == 1.0 and (precision[0, :, 0] > 0).all()                 # every recall point reached ...
        assert (precision[:, -1, 1] == 0).all() and (d_total < 255 or (precision[1:, -1, 0] == 0).all())      # ... and the upper ones never
    else:
        assert (precision[:, :, :2] == 0).all() and (recall[:, :2] == 0).all()        # gts that count, no detection


def test_statistics_equal_the_host_bit_for_bit_on_the_generated_set():
    from fpd_amd.lib.dataset import coco_eval as E
    gts, dts, image_ids = K.case_set()
    want = E.evaluate_keypoints(gts, dts, image_ids, [1])
    got = E.evaluate_keypoints_device(gts, dts, image_ids, [1])
    assert got.dtype == np.float64 and got.tolist() == want.tolist(), (got, want)
    assert (want[[0, 3, 4, 5]] > 0).all() and (want < 1).all()                        # a table with something in every column
    # the arrays entry with its tables, through a capped grid
    packed = E.pack_ground_truth(gts, image_ids, 1)
    stats, precision, recall = E.evaluate_arrays_device(packed, [d['image_id'] for d in dts], [d['keypoints'] for d in dts],
                                                        [d['score'] for d in dts], grid=5, return_tables=True)
    assert stats.tolist() == want.tolist() and precision.shape == (10, 101, 1, 3) and recall.shape == (10, 1, 3)
    pictures = K.host_case_set()
    for r in range(3):
        want_p, want_r = E.accumulate([p[3][r] for p in pictures])
        assert np.array_equal(precision[:, :, 0, r], want_p) and np.array_equal(recall[:, 0, r], want_r)


@pytest.mark.parametrize('scene', sorted(K.hand_scenes()))
def test_statistics_equal_the_host_on_the_hand_derived_scenes(scene):
    from fpd_amd.lib.dataset import coco_eval as E
    gts, dts = K.hand_scenes()[scene]
    image_ids = sorted({g['image_id'] for g in gts})
    want = E.evaluate_keypoints(gts, dts, image_ids, [1])
    assert E.evaluate_keypoints_device(gts, dts, image_ids, [1]).tolist() == want.tolist()


@pytest.mark.parametrize('mode', ['hard', 'soft'])
def test_dataset_evaluate_is_the_same_with_and_without_host_eval(tmp_path, mode):
    from fpd_amd.lib.dataset import COCODataset
    G = T.load_golden()
    tree = T.write_tree(tmp_path / 'coco', G, images=False)
    cfg = T.make_cfg(tree, test={'USE_GT_BBOX': False, 'SOFT_NMS': mode == 'soft'})
    ds = COCODataset(cfg, tree, 'val2017', False)
    paths = [os.path.join(tree, p) for p in G['in_paths']]
    on_host = ds.evaluate(cfg, G['in_preds'].copy(), str(tmp_path / 'host'), G['in_boxes'].copy(), paths, host_eval=True)
    on_device = ds.evaluate(cfg, G['in_preds'].copy(), str(tmp_path / 'device'), G['in_boxes'].copy(), paths)
    assert on_device == on_host and list(on_device[0].values()) == list(on_host[0].values())
    assert ds.packed_ground_truth() is ds.packed_ground_truth()                      # packed once
    with open(os.path.join(str(tmp_path / 'host'), 'results', 'keypoints_val2017_results_0.json')) as a, \
            open(os.path.join(str(tmp_path / 'device'), 'results', 'keypoints_val2017_results_0.json')) as b:
        assert a.read() == b.read()


def test_a_bad_offset_table_is_refused_and_nothing_of_the_picture_is_written():
    """The gts of picture 1 declared past the end of the gt arrays, which leaves picture 2 a start past the end and a negative
    count: status -1 for both, the sentinels in their rows untouched; the pictures around them are served as ever."""
    from fpd_amd.lib.dataset import coco_eval as E
    gts, dts, image_ids = K.case_set()
    keep = [K.PIC['twenty'], K.PIC['crowd'], K.PIC['edges'], K.PIC['twins']]
    gts, dts = [g for g in gts if g['image_id'] in keep], [d for d in dts if d['image_id'] in keep]
    t, packed, rows, dt_offsets = K.device_inputs(gts, dts, keep)
    good = {k: v.cpu().numpy() for k, v in E.match_device(t).items()}
    g_off, d_off = packed['gt_offsets'].copy(), dt_offsets.copy()
    assert (np.diff(g_off) > 0).all() and (np.diff(d_off) > 0).all()
    g_total = int(g_off[-1])
    bad_g = g_off.copy()
    bad_g[2] = g_total + 5                                                            # picture 1 ends past G_total (picture 2 then has a negative count)
    dev = t['sigmas'].device
    fill = lambda k, v: torch.full(good[k].shape, v, dtype=getattr(torch, good[k].dtype.name), device=dev)  # noqa: E731
    out = {'matched': fill('matched', 7), 'dt_ignored': fill('dt_ignored', 7), 'gt_counted': fill('gt_counted', -7),
           'dt_area': fill('dt_area', -7.0), 'status': fill('status', 9), 'oks': fill('oks', -7.0)}
    got = E.match_device(dict(t, gt_offsets=torch.from_numpy(bad_g).to(dev)), out=out)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    oks_off = t['oks_offsets'].cpu().numpy()
    assert got['status'].tolist() == [0, -1, -1, 0]
    for i in range(4):
        d, o = slice(d_off[i], d_off[i + 1]), slice(oks_off[i], oks_off[i + 1])
        if got['status'][i] == 0:
            for k in ('matched', 'dt_ignored'):
                assert np.array_equal(got[k][:, :, d], good[k][:, :, d])
            assert np.array_equal(got['dt_area'][d], good['dt_area'][d]) and np.array_equal(got['oks'][o], good['oks'][o])
            assert np.array_equal(got['gt_counted'][:, i], good['gt_counted'][:, i])
        else:
            assert (got['matched'][:, :, d] == 7).all() and (got['dt_ignored'][:, :, d] == 7).all() and (got['dt_area'][d] == -7.0).all()
            assert (got['oks'][o] == -7.0).all() and (got['gt_counted'][:, i] == -7).all()
