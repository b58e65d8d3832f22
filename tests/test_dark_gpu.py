"""DARK sub-pixel decoding on the device: fpd_dark_refine against the float64 numpy restatement (tests/_dark_ref.py) on both
layouts, its two output forms against each other and against fpd_val_post's rows, and core.function.validate with
TEST.DARK against the per-batch body.

With FPD_DARK_RECORD=<file> every heat-map-coordinate case appends its measured error and its float32 error scale to that
file (the record kept as profiles/dark_gpu.txt)."""
import os

import numpy as np
import pytest
import torch

from tests import _cases_infer as CI
from tests import _dark_ref as D

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
_REF = {}


def reference(name):
    """(maps, k, float64 restatement, E32) of a case, computed once on the CPU and only read afterwards."""
    if name not in _REF:
        if name == 'designed':
            maps, k = D.designed_case()[0], 11
        else:
            maps, _, k = D.random_case(name)
        r64, r32 = D.decode(maps, k), D.decode(maps, k, np.float32)
        e32 = float(np.abs(r64[0].astype(np.float64) - r32[0].astype(np.float64)).max())
        for a in r64[:3]:
            a.setflags(write=False)
        _REF[name] = (maps, k, r64, e32)
    return _REF[name]


def run_dark(maps, k, layout, trans=None):
    """fpd_dark_refine on [N,J,H,W] float32 maps handed over in `layout` -> coords, maxvals, refined, preds (numpy)."""
    from fpd_amd import runtime as R
    from fpd_amd.lib.core.inference import dark_taps_device
    n, j, h, w = maps.shape
    hm = torch.from_numpy(np.ascontiguousarray(maps if layout == 'nchw' else maps.transpose(0, 2, 3, 1))).cuda()
    taps = dark_taps_device(k, hm.device)
    coords = torch.full((n, j, 2), SENTINEL, dtype=torch.float32, device='cuda')
    maxvals = torch.full((n, j), SENTINEL, dtype=torch.float32, device='cuda')
    refined = torch.full((n, j), -1, dtype=torch.int32, device='cuda')
    a = R.DarkT()
    a.N, a.J, a.H, a.W, a.ksize = n, j, h, w, k
    a.layout = R.DARK_NCHW if layout == 'nchw' else R.DARK_NHWC
    a.hm, a.taps, a.coords, a.maxvals, a.refined = hm.data_ptr(), taps.data_ptr(), coords.data_ptr(), maxvals.data_ptr(), refined.data_ptr()
    preds = None
    if trans is not None:
        t = torch.from_numpy(np.ascontiguousarray(trans, np.float64)).cuda()
        preds = torch.full((n, j, 2), SENTINEL, dtype=torch.float32, device='cuda')
        a.trans, a.preds = t.data_ptr(), preds.data_ptr()
    R.check(R.lib().fpd_dark_refine(a, R.current_stream()), 'fpd_dark_refine')
    return coords.cpu().numpy(), maxvals.cpu().numpy(), refined.cpu().numpy(), (preds.cpu().numpy() if preds is not None else None)


def check_heatmap_coords(name, layout):
    from fpd_amd.lib.core.inference import final_preds_device
    maps, k, (c64, v64, r64, _), e32 = reference(name)
    coords, maxvals, refined, _ = run_dark(maps, k, layout)
    arg, _, argv = final_preds_device(torch.from_numpy(maps).cuda(), None, 0)
    arg, argv = arg.cpu().numpy(), argv.cpu().numpy()[..., 0]
    err = np.abs(coords.astype(np.float64) - c64.astype(np.float64))
    bound = 4 * e32 + 2.0 ** -17
    moved = int((coords != arg).any(-1).sum())
    line = '%-8s %-4s %dx%dx%dx%d k=%d  refined %d of %d (moved %d)  kernel error %.3e  E32 %.3e  bound 4*E32+2^-17 %.3e' % (
        (name, layout) + maps.shape + (k, int(refined.sum()), refined.size, moved, err.max(), e32, bound))
    print(line)
    if os.environ.get('FPD_DARK_RECORD'):
        with open(os.environ['FPD_DARK_RECORD'], 'a') as f:
            f.write(line + '\n')
    assert maxvals.tobytes() == argv.tobytes() == v64.tobytes()
    assert np.array_equal(refined, r64), (name, layout, refined, r64)
    keep = refined == 0
    assert coords[keep].tobytes() == arg[keep].tobytes() == c64[keep].tobytes()
    assert err.max() <= bound, (name, layout, err.max(), e32, bound)
    return coords, arg, refined


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('name', ['S1', 'S2', 'S3', 'S4'])
def test_heatmap_coordinates_match_the_float64_restatement(name, layout):
    coords, arg, refined = check_heatmap_coords(name, layout)
    assert refined.all() and (coords != arg).any(-1).all()      # the input condition of the random cases: every map is refined


def test_heatmap_coordinates_at_the_lds_limit():
    """128x128: two fp32 images of the map are 128 KB of LDS, beyond the 64 KB a kernel gets without asking."""
    for layout in ('nchw', 'nhwc'):
        _, _, refined = check_heatmap_coords('S5', layout)
        assert refined.all()


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
def test_designed_cases_take_the_guards_the_clamp_and_the_first_maximum(layout):
    maps, names = D.designed_case()
    coords, arg, refined = check_heatmap_coords('designed', layout)
    assert np.array_equal(refined[0], D.designed_expectation(names))
    q = names.index('spike')
    assert refined[0, q] == 1 and coords[0, q].tolist() == [5.0, 7.0]          # a step of exactly zero
    q = names.index('two maxima')
    assert arg[0, q].tolist() == [4.0, 5.0] and refined[0, q] == 1              # the first of the two wins
    q = names.index('not positive')
    assert coords[0, q].tolist() == [0.0, 0.0]


@pytest.mark.parametrize('f32', [0, 1])
@pytest.mark.parametrize('name', ['S1', 'S3'])
def test_get_final_preds_with_dark_maps_the_kernels_coordinates_to_the_image(name, f32):
    """Form (a): image coordinates against the kernel's own float32 heat-map coordinates under the float64 matrix on the host."""
    from fpd_amd import runtime as R
    from fpd_amd.lib.config import _defaults
    from fpd_amd.lib.core import inference as I
    from fpd_amd.lib.utils.transforms import get_affine_transform
    maps, k, (c64, v64, _, _), _ = reference(name)
    n, j, h, w = maps.shape
    c, s = CI.centers_scales(31 + f32, n, np.float32 if f32 else np.float64)
    cfg = _defaults()
    cfg.TEST.DARK, cfg.TEST.BLUR_KERNEL, cfg.TEST.POST_PROCESS = True, k, True
    preds, maxvals = I.get_final_preds(cfg, torch.from_numpy(maps).cuda(), c, s)
    coords = run_dark(maps, k, 'nchw')[0]
    assert not np.array_equal(coords, D.argmax_coords(maps)[0])
    trans = np.stack([get_affine_transform(c[i], s[i], 0, [w, h], inv=1) for i in range(n)])
    want = np.einsum('nrc,njc->njr', trans, np.concatenate([coords.astype(np.float64), np.ones((n, j, 1))], -1))
    assert preds.dtype == np.float32 and preds.shape == (n, j, 2) and maxvals.shape == (n, j, 1)
    np.testing.assert_allclose(preds, want, rtol=0, atol=2e-4)
    assert maxvals[..., 0].tobytes() == v64.tobytes()
    # the same launch through the struct, and TEST.POST_PROCESS has no say once DARK is on
    assert run_dark(maps, k, 'nchw', trans)[3].tobytes() == preds.tobytes()
    cfg.TEST.POST_PROCESS = False
    assert I.get_final_preds(cfg, torch.from_numpy(maps).cuda(), c, s)[0].tobytes() == preds.tobytes()
    # off: the quarter-pixel shift, as before
    cfg.TEST.DARK = False
    off = I.get_final_preds(cfg, torch.from_numpy(maps).cuda(), c, s)[0]
    assert off.tobytes() != preds.tobytes()
    with pytest.raises(R.FpdError):
        I.final_preds_device(torch.from_numpy(maps).cuda(), None, False, dark=10)


@pytest.mark.parametrize('flip', [0, 1])
@pytest.mark.parametrize('f32', [0, 1])
def test_form_b_on_the_merged_map_equals_form_a_and_writes_x_and_y_only(f32, flip):
    from fpd_amd import runtime as R
    from fpd_amd.lib.core.inference import dark_taps_device, final_preds_device
    from fpd_amd.lib.utils.transforms import channel_sources, get_affine_transform
    maps, k, _, _ = reference('S2')
    n, j, h, w = maps.shape
    pairs = [[0, 1], [2, 4]]
    row0, rows = 3, n + 5
    a_t = torch.from_numpy(np.ascontiguousarray(maps.transpose(0, 2, 3, 1))).cuda()
    b_t = torch.from_numpy(np.ascontiguousarray(D.random_case('S2', seed=77)[0].transpose(0, 2, 3, 1))).cuda() if flip else None
    c, s = CI.centers_scales(41 + f32, n, np.float32 if f32 else np.float64)
    score = np.linspace(0.2, 0.9, n)
    merged = torch.empty((n, h, w, j), dtype=torch.float32, device='cuda')
    preds = torch.full((rows, j, 3), SENTINEL, dtype=torch.float32, device='cuda')
    boxes = torch.full((rows, 6), SENTINEL, dtype=torch.float64, device='cuda')
    meta = torch.from_numpy(np.concatenate([np.asarray(c, np.float64).reshape(-1), np.asarray(s, np.float64).reshape(-1), score])).cuda()
    p = R.ValPostT()
    p.N, p.J, p.H, p.W, p.dtype = n, j, h, w, R.F32
    p.shift, p.post_process, p.box_f32, p.row0, p.rows = flip, 0, f32, row0, rows
    p.a, p.b = a_t.data_ptr(), (b_t.data_ptr() if flip else None)
    p.center, p.scale, p.score = meta.data_ptr(), meta.data_ptr() + 16 * n, meta.data_ptr() + 32 * n
    p.merged, p.all_preds, p.all_boxes = merged.data_ptr(), preds.data_ptr(), boxes.data_ptr()
    for q, v in enumerate(channel_sources(j, pairs)):
        p.src[q] = v
    R.check(R.lib().fpd_val_post(p, R.current_stream()), 'fpd_val_post')
    before_p, before_b = preds.cpu().numpy(), boxes.cpu().numpy()
    taps = dark_taps_device(k, 'cuda')
    d = R.DarkT()
    d.N, d.J, d.H, d.W, d.layout, d.ksize, d.box_f32, d.row0, d.rows = n, j, h, w, R.DARK_NHWC, k, f32, row0, rows
    d.hm, d.taps, d.center, d.scale, d.all_preds = merged.data_ptr(), taps.data_ptr(), p.center, p.scale, preds.data_ptr()
    R.check(R.lib().fpd_dark_refine(d, R.current_stream()), 'fpd_dark_refine')
    after_p, after_b = preds.cpu().numpy(), boxes.cpu().numpy()
    # form (a) on the NCHW copy of the same map, the matrices from the host
    trans = np.stack([get_affine_transform(c[i], s[i], 0, [w, h], inv=1) for i in range(n)])
    nchw = merged.permute(0, 3, 1, 2).contiguous()
    _, want, want_v = final_preds_device(nchw, torch.from_numpy(trans).cuda(), True, dark=k)
    sl = slice(row0, row0 + n)
    assert after_p[sl, :, 0:2].tobytes() == want.cpu().numpy().tobytes()
    assert after_p[sl, :, 2].tobytes() == before_p[sl, :, 2].tobytes() == want_v.cpu().numpy()[..., 0].tobytes()
    assert after_b.tobytes() == before_b.tobytes()
    keep = np.ones(rows, bool)
    keep[sl] = False
    assert (after_p[keep] == SENTINEL).all() and (after_b[keep] == SENTINEL).all() and not (after_b[sl] == SENTINEL).any()
    assert (after_p[sl, :, 0:2] != before_p[sl, :, 0:2]).any()                # the decode moved something


# ---- validate ----
def make_cfg(n_valid, batch, flip, dark):
    from fpd_amd.lib.config import _defaults
    cfg = _defaults()
    cfg.DATASET.DATASET, cfg.DATASET.NUM_VALID_SAMPLES, cfg.TEST.BATCH_SIZE_PER_GPU, cfg.PRINT_FREQ = 'synthetic_aug', n_valid, batch, 1
    cfg.TEST.FLIP_TEST = cfg.TEST.SHIFT_HEATMAP = cfg.TEST.POST_PROCESS = bool(flip)
    cfg.MODEL.EXTRA.NUM_FEATURES, cfg.MODEL.EXTRA.NUM_STACKS = 32, 2
    cfg.MODEL.IMAGE_SIZE, cfg.MODEL.HEATMAP_SIZE = [128, 128], [32, 32]
    cfg.TEST.DARK = bool(dark)
    return cfg


_MODEL = []


def tiny_model():
    if not _MODEL:
        from fpd_amd.lib import models
        torch.manual_seed(3)
        m = models.hourglass.get_pose_net(make_cfg(4, 4, False, False), is_train=False)
        if hasattr(m, 'reset_parameters'):
            m.reset_parameters()
        _MODEL.append(m.cuda().eval())
    return _MODEL[0]


@pytest.mark.parametrize('flip', [False, True])
def test_validate_with_dark_equals_the_per_batch_body_and_is_silent_when_off(flip, tmp_path, monkeypatch):
    """10 samples in batches of 4, tiny fp32 hourglass: three batches, the last one smaller."""
    from fpd_amd import runtime as R
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    from fpd_amd.lib.dataset.device_dataset import synthetic_aug
    lib, calls = R.lib(), []
    real = lib.fpd_dark_refine

    def counted(a, st):
        calls.append(int(a.layout))
        return real(a, st)
    monkeypatch.setattr(lib, 'fpd_dark_refine', counted)
    model, crit = tiny_model(), JointsMSELoss(True).cuda()
    res = {}
    for dark in (False, True):
        cfg = make_cfg(10, 4, flip, dark)
        _, loader, db = synthetic_aug(cfg, 'cuda', train=False)
        del calls[:]
        F._validate_per_batch(cfg, loader, db, model, crit, str(tmp_path), str(tmp_path))
        want, n_want = F._validate_per_batch.last, list(calls)
        del calls[:]
        F.validate(cfg, loader, db, model, crit, str(tmp_path), str(tmp_path))
        got, n_got = F.validate.last, list(calls)
        assert n_want == ([R.DARK_NCHW] * 3 if dark else []) and n_got == ([R.DARK_NHWC] * 3 if dark else []), (dark, n_want, n_got)
        assert got['all_preds'].dtype == np.float32 and got['all_preds'].shape == (10, 16, 3) and np.isfinite(got['all_preds']).all()
        assert got['all_preds'].tobytes() == want['all_preds'].tobytes()
        assert got['all_boxes'].tobytes() == want['all_boxes'].tobytes()
        res[dark] = got
    assert res[True]['all_preds'][:, :, 2].tobytes() == res[False]['all_preds'][:, :, 2].tobytes()
    assert res[True]['all_boxes'].tobytes() == res[False]['all_boxes'].tobytes()
    assert (res[True]['all_preds'][:, :, 0:2] != res[False]['all_preds'][:, :, 0:2]).any()
