"""Rescoring + OKS NMS on the MI355X (csrc/oks_nms.hip through the C ABI fpd_oks_nms; lib/nms/nms.py) against the
reference's own `oks_nms` / `soft_oks_nms` / `oks_iou` as recorded in tests/golden/coco_ref.npz: P = 1, 2, 3, 17, 65, 130, 257
clustered people (65 and 257 are the smallest sizes that cross a wavefront and a 256-thread block), and against the numpy
restatement (tests/_coco_ref.py, itself held to the fixture by tests/test_coco_cpu.py) on seeded multi-picture inputs.

Tolerances: the keep lists and `score` are exact (the fixture's decisions have margins >= 1e-6; the rescoring is float32
arithmetic in a fixed order and one float64 product); the OKS with the top person is compared within 1e-12 relative: 17
terms, each a correctly rounded float64 quotient chain followed by an exp good to a few ulp (2.2e-16), with a hundredfold
margin."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _coco_ref as C
from tests import _coco_tree as T

pytestmark = pytest.mark.gpu

G = T.load_golden()
THRESH, VIS = float(G['nms/thresh']), float(G['nms/in_vis_thre'])


def case(p):
    return G['nms/%d/kpts' % p], G['nms/%d/area' % p], G['nms/%d/box_score' % p]


def device_nms(kpts, area, box, offsets, soft, **kw):
    from fpd_amd.lib.nms.nms import oks_nms_device
    return oks_nms_device(kpts, area, box, offsets, THRESH, soft=soft, in_vis_thre=VIS, want_oks=True, **kw)


@pytest.mark.parametrize('soft', [False, True], ids=['hard', 'soft'])
@pytest.mark.parametrize('p', T.NMS_SIZES)
def test_every_golden_case(p, soft):
    kpts, area, box = case(p)
    score, keep, n_keep, oks = device_nms(kpts, area, box, [0, p], soft)
    want = G['nms/%d/%s' % (p, 'soft' if soft else 'hard')]
    assert score.dtype == np.float64 and np.array_equal(score, G['nms/%d/score' % p])              # bit for bit
    assert n_keep.tolist() == [len(want)] and keep[:len(want)].tolist() == want.tolist() and (keep[len(want):] == -1).all()
    want_oks = G['nms/%d/oks_top' % p]
    rel = np.abs(oks - want_oks) / want_oks
    print('P %d %s: kept %d, max relative OKS error %.3g' % (p, 'soft' if soft else 'hard', len(want), rel.max()))
    assert (want_oks > 0).all() and rel.max() <= 1e-12
    assert len(want) == (min(p, 20) if soft else len(G['nms/%d/hard' % p]))


@pytest.mark.parametrize('soft', [False, True], ids=['hard', 'soft'])
@pytest.mark.parametrize('grid', [0, 3], ids=['grid_default', 'grid3'])
def test_all_cases_as_the_pictures_of_one_launch(grid, soft):
    """257, empty, 1, 130, 2, 65, empty, 3, 17 people: a picture must not read its neighbour's; with 3 workgroups for 9
    pictures each workgroup owns three in turn."""
    sizes = [257, 0, 1, 130, 2, 65, 0, 3, 17]
    parts = [case(p) for p in sizes if p]
    kpts, area, box = (np.concatenate([c[k] for c in parts]) for k in range(3))
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    score, keep, n_keep, oks = device_nms(kpts, area, box, offsets, soft, grid=grid)
    for i, p in enumerate(sizes):
        a = int(offsets[i])
        if p == 0:
            assert n_keep[i] == 0
            continue
        want = G['nms/%d/%s' % (p, 'soft' if soft else 'hard')]
        assert np.array_equal(score[a:a + p], G['nms/%d/score' % p]), p
        assert n_keep[i] == len(want) and keep[a:a + len(want)].tolist() == want.tolist() and (keep[a + len(want):a + p] == -1).all(), p
        want_oks = G['nms/%d/oks_top' % p]
        assert (np.abs(oks[a:a + p] - want_oks) <= 1e-12 * want_oks).all(), p


@pytest.mark.parametrize('soft', [False, True], ids=['hard', 'soft'])
def test_seeded_pictures_against_the_restatement(soft):
    """60 pictures of 0 .. 40 clustered people.  The decisions of these inputs have the margins the fixture asks for
    (asserted here, on the host), so the last bits of an exp cannot flip one."""
    rng = np.random.default_rng(11)
    sizes = rng.integers(0, 41, 60)
    sizes[:3] = (0, 1, 40)
    parts = [C.clustered_people(rng, int(p)) for p in sizes if p]
    kpts, area, box = (np.concatenate([c[k] for c in parts]) for k in range(3))
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    want_score, want_keep, want_n = C.nms_pictures(kpts, area, box, offsets, VIS, THRESH, soft)
    for i in range(len(sizes)):
        a, b = int(offsets[i]), int(offsets[i + 1])
        if b - a > 1:
            og, sg, wg = C.margins(kpts[a:b], area[a:b], want_score[a:b], THRESH)
            assert og >= 1e-6 and sg > 0 and wg >= 1e-9, (i, og, sg, wg)
    score, keep, n_keep, _ = device_nms(kpts, area, box, offsets, soft, grid=7)
    assert np.array_equal(score, want_score) and np.array_equal(n_keep, want_n) and np.array_equal(keep, want_keep)
    assert 0.2 < want_n.sum() / sizes.sum() < (1.01 if soft else 0.6)


def test_everyone_suppressed_by_the_first_pick_and_nobody_suppressed():
    rng = np.random.default_rng(5)
    p = 300                                                             # more than one sweep of a 256-thread block
    pose = rng.uniform(50, 400, (1, 17, 2))
    kpts = np.zeros((p, 17, 3), np.float32)
    kpts[:, :, 0:2] = pose + rng.uniform(-0.05, 0.05, (p, 17, 2))       # OKS of any two > 0.999
    kpts[:, :, 2] = rng.uniform(0.3, 1.0, (p, 17))
    area, box = rng.uniform(4e4, 1.2e5, p), rng.uniform(0.1, 1.0, p)
    score, keep, n_keep, oks = device_nms(kpts, area, box, [0, p], False)
    assert np.array_equal(score, C.rescore(kpts, box, VIS)) and len(set(score.tolist())) == p
    assert oks.min() > 0.999 and n_keep.tolist() == [1] and keep[0] == int(np.argmax(score)) and (keep[1:] == -1).all()
    # the same people 1000 px apart: every OKS but the pick's own is 0, everyone is kept, best first
    kpts[:, :, 0] += (np.arange(p) * 1000.0)[:, None]
    score2, keep2, n_keep2, oks2 = device_nms(kpts, area, box, [0, p], False)
    assert np.array_equal(score2, score) and n_keep2.tolist() == [p]
    assert keep2.tolist() == np.argsort(-score, kind='stable').tolist()
    assert np.sort(oks2)[-2] < 1e-6 and oks2[keep2[0]] == 1.0
    # soft: the 20 best in order (nothing decays: exp(-0^2 / thresh) = 1)
    _, keep3, n_keep3, _ = device_nms(kpts, area, box, [0, p], True)
    assert n_keep3.tolist() == [20] and keep3[:20].tolist() == keep2[:20].tolist() and (keep3[20:] == -1).all()


def test_equal_scores_go_to_the_lower_index():
    """The kernel's own rule (numpy leaves the order of ties open): four distant people with the same maxvals and box score."""
    kpts = np.zeros((4, 17, 3), np.float32)
    kpts[:, :, 0] = (np.arange(4) * 1000.0)[:, None] + np.arange(17)[None, :]
    kpts[:, :, 2] = 0.5
    box = np.array([0.5, 0.9, 0.9, 0.5])
    for soft in (False, True):
        _, keep, n_keep, _ = device_nms(kpts, np.full(4, 5e4), box, [0, 4], soft)
        assert n_keep.tolist() == [4] and keep.tolist() == [1, 2, 0, 3]


def test_rescoring_counts_only_the_joints_above_the_threshold():
    kpts = np.zeros((3, 17, 3), np.float32)
    kpts[:, :, 0] = (np.arange(3) * 1000.0)[:, None]
    kpts[0, :, 2] = 0.1                                                  # nothing above 0.2: score 0
    kpts[1, :3, 2] = (0.2, 0.7, 0.4)                                     # 0.2 is not above 0.2: mean of 0.7 and 0.4
    kpts[2, :, 2] = np.float32(0.2) + np.float32(1e-7)
    score, keep, n_keep, _ = device_nms(kpts, np.full(3, 5e4), np.array([0.9, 0.5, 0.25]), [0, 3], False)
    want1 = np.float64((np.float32(0.7) + np.float32(0.4)) / np.float32(2)) * 0.5
    assert score[0] == 0.0 and score[1] == want1 and 0.25 * 0.2 < score[2] < 0.25 * 0.2001
    assert np.array_equal(score, C.rescore(kpts, np.array([0.9, 0.5, 0.25]), VIS)) and keep.tolist() == [1, 2, 0]


def test_a_bad_offset_table_is_refused_per_picture_and_nothing_of_it_is_touched():
    """Straight through the C ABI (the Python wrapper checks the offsets before it uploads): picture 0 claims rows 0 .. 6 of 4
    people, picture 1 a negative range; picture 2 is fine."""
    from fpd_amd import runtime as R
    kpts, area, box = (torch.from_numpy(np.ascontiguousarray(v[:4])).cuda() for v in case(17))
    kpts = kpts.float()
    offsets = torch.tensor([0, 6, 2, 4], dtype=torch.int32).cuda()
    sig = torch.from_numpy(C.SIGMAS).cuda()
    score = torch.full((4,), -7.0, dtype=torch.float64).cuda()
    work = torch.full((4,), -7.0, dtype=torch.float64).cuda()
    keep = torch.full((4,), -7, dtype=torch.int32).cuda()
    n_keep = torch.full((3,), -7, dtype=torch.int32).cuda()
    a = R.OksNmsT()
    a.P_total, a.n_img, a.J, a.rescore, a.in_vis_thre, a.oks_thre = 4, 3, 17, 1, VIS, THRESH
    a.kpts, a.area, a.box_score, a.offsets, a.sigmas = kpts.data_ptr(), area.data_ptr(), box.data_ptr(), offsets.data_ptr(), sig.data_ptr()
    a.score, a.work, a.keep, a.n_keep = score.data_ptr(), work.data_ptr(), keep.data_ptr(), n_keep.data_ptr()
    R.check(R.lib().fpd_oks_nms(ctypes.byref(a), R.current_stream()), 'fpd_oks_nms')
    torch.cuda.synchronize()
    assert n_keep.tolist()[:2] == [-1, -1] and n_keep.tolist()[2] >= 1
    assert score[:2].tolist() == [-7.0, -7.0] and keep[:2].tolist() == [-7, -7] and (score[2:] != -7.0).all()
    from fpd_amd.lib.nms.nms import oks_nms_device
    with pytest.raises(R.FpdError, match='offsets'):
        oks_nms_device(case(17)[0][:4], case(17)[1][:4], case(17)[2][:4], [0, 6, 2, 4], THRESH)


def test_the_wrappers_keep_the_reference_signatures_and_return_types():
    from fpd_amd.lib.nms import nms
    from fpd_amd.runtime import FpdError
    p = 65
    kpts, area, _ = case(p)
    score = G['nms/%d/score' % p]
    db = [{'keypoints': kpts[i], 'area': area[i], 'score': score[i]} for i in range(p)]
    hard = nms.oks_nms(db, THRESH)
    assert type(hard) is list and all(type(k) is int for k in hard) and hard == G['nms/%d/hard' % p].tolist()
    soft = nms.soft_oks_nms(db, THRESH)
    assert isinstance(soft, np.ndarray) and soft.dtype == np.intp and soft.tolist() == G['nms/%d/soft' % p].tolist()
    top = int(np.argmax(score))
    flat = kpts.reshape(p, -1)
    iou = nms.oks_iou(flat[top], flat, area[top], area)
    want = G['nms/%d/oks_top' % p]
    assert isinstance(iou, np.ndarray) and iou.dtype == np.float64 and iou.shape == (p,)
    assert (np.abs(iou - want) <= 1e-12 * want).all()
    assert nms.oks_iou(flat[top], flat[:0], area[top], area[:0]).shape == (0,)
    for call in (lambda: nms.oks_nms(db, THRESH, None, 0.2), lambda: nms.soft_oks_nms(db, THRESH, None, 0.2),
                 lambda: nms.oks_iou(flat[top], flat, area[top], area, None, 0.2)):
        with pytest.raises(FpdError, match='in_vis_thre'):
            call()
