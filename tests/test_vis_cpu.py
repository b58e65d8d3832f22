"""utils.vis, the parts that need no GPU: the host restatement (tests/_vis_ref.py) against hand-derived cases, a HOST build of
the kernels' per-pixel arithmetic (csrc/vis_math.h) against the restatement bit for bit, the same text under the host
sanitizers as a stand-alone program, the ABI surface and refusals of the four fpd_vis_* entry points, save_debug_images' flag
logic with the renderer stubbed, and AsyncImageWriter on numpy canvases."""
import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _vis_ref as ref
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'fast-human-pose-estimation.pytorch_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'native', 'vis_host.cpp')


def _cxx():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler for the host build of csrc/vis_math.h')
    return cxx


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('vis') / 'libvis_host.so')
    subprocess.check_call([_cxx(), '-O2', '-ffp-contract=off', '-Wno-unknown-pragmas', '-shared', '-fPIC', '-I' + CSRC, SRC, '-o', so])
    lib = C.CDLL(so)
    lib.vis_mark_pos_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double]
    lib.vis_trunc_host.argtypes = [C.c_double]
    lib.vis_norm_bytes_host.argtypes = [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_int, C.c_void_p]
    lib.vis_heat_bytes_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    return lib


# ---- the restatement against hand-derived cases ----

@pytest.mark.parametrize('n,nrow,shape,cells', [
    (3, 2, (38, 30), [(2, 2), (2, 16), (20, 2)]),                   # 2 x 2 cells of 16 x 12 (+2): (18*2+2, 14*2+2); cell 3 unused
    (9, 8, (38, 114), [(2, 2 + 14 * k) for k in range(8)] + [(20, 2)]),
    (1, 8, (16, 12), [(0, 0)]),                                     # a single image comes back bare
])
def test_restated_make_grid_geometry(n, nrow, shape, cells):
    x = torch.stack([torch.full((3, 16, 12), float(k + 1)) for k in range(n)])
    g = ref.make_grid(x, nrow, 2, False)
    assert tuple(g.shape) == (3,) + shape
    want = torch.zeros((3,) + shape)
    for k, (y0, x0) in enumerate(cells):
        want[:, y0:y0 + 16, x0:x0 + 12] = k + 1
    assert torch.equal(g, want)
    from fpd_amd.lib.utils import vis
    assert vis.grid_shape(n, 16, 12, nrow, 2) == shape


def test_restated_resize_is_the_rounded_mean_of_the_four_centre_pixels():
    block = np.zeros((4, 4, 3), np.uint8)
    block[:, :, 0] = np.arange(16).reshape(4, 4) * 10              # centre: 50, 60, 90, 100 -> (300 + 2) >> 2 = 75
    block[1, 1, 1], block[1, 2, 1], block[2, 1, 1], block[2, 2, 1] = 255, 255, 255, 254      # 1019 + 2 >> 2 = 255
    block[1, 1, 2], block[0, 0, 2], block[3, 3, 2] = 1, 200, 200                           # (1 + 2) >> 2 = 0: the rim is not read
    out = ref.resize4(block, (1, 1))
    assert out.shape == (1, 1, 3) and out[0, 0].tolist() == [75, 255, 0]
    two = np.concatenate([block, block[:, :, ::-1]], 1)
    assert ref.resize4(two, (2, 1))[0].tolist() == [[75, 255, 0], [0, 255, 75]]


def test_colour_table_entries():
    """255 c = 382.5 - |4v - 255k| wherever c is not clipped: every unclipped entry sits on a rounding tie of
    floor(255 c + 0.5), which exact arithmetic resolves to 383 - |4v - 255k| and the float64 evaluation the table is defined
    by to that or one less.  The clipped entries, the two ends and the breakpoints are derived by hand; the restatement (Python
    scalars) and the package (numpy) evaluate the same float64 operations and must agree everywhere."""
    from fpd_amd.lib.utils import vis
    assert vis.JET_BGR.dtype == np.uint8 and vis.JET_BGR.shape == (256, 3) and np.array_equal(ref.JET_BGR, vis.JET_BGR)
    t = ref.JET_BGR.astype(np.int64)
    for v in range(256):
        for pos, k in ((0, 1), (1, 2), (2, 3)):                     # b, g, r
            c = Fraction(3, 2) - abs(Fraction(4 * v, 255) - k)
            if c >= 1 or c <= 0:
                assert t[v, pos] == (255 if c >= 1 else 0), (v, pos)
            else:
                assert 383 - abs(4 * v - 255 * k) - t[v, pos] in (0, 1), (v, pos)
    assert t[0].tolist() == [128, 0, 0] and t[255].tolist() == [0, 0, 128]
    # the breakpoints 4t = 0.5, 1.5, 2.5, 3.5 fall between v = 31|32, 95|96, 159|160, 223|224: a channel saturates or
    # leaves zero there (the values next to 0 are the ties 0.5 and 1.5)
    assert t[31, 0] in (251, 252) and t[32, 0] == 255 and t[31, 1] == 0 and t[32, 1] in (0, 1)
    assert t[95, 0] == 255 and t[96, 0] in (253, 254) and t[95, 1] in (252, 253) and t[96, 1] == 255 and t[95, 2] == 0 and t[96, 2] in (1, 2)
    assert t[159, 2] in (253, 254) and t[160, 2] == 255 and t[159, 1] == 255 and t[160, 1] in (252, 253) and t[159, 0] in (1, 2) and t[160, 0] == 0
    assert t[223, 2] == 255 and t[224, 2] in (251, 252) and t[223, 1] in (0, 1) and t[224, 1] == 0


def test_both_mark_shapes_pixel_by_pixel():
    img = np.zeros((9, 9), np.uint8)
    ref.circle(img, (4, 4), 2, 1, 2)
    assert img.tolist() == [[0] * 9,
                            [0, 0, 0, 0, 1, 0, 0, 0, 0],
                            [0, 0, 1, 1, 1, 1, 1, 0, 0],
                            [0, 0, 1, 1, 1, 1, 1, 0, 0],
                            [0, 1, 1, 1, 0, 1, 1, 1, 0],
                            [0, 0, 1, 1, 1, 1, 1, 0, 0],
                            [0, 0, 1, 1, 1, 1, 1, 0, 0],
                            [0, 0, 0, 0, 1, 0, 0, 0, 0],
                            [0] * 9]
    img = np.zeros((5, 5), np.uint8)
    ref.circle(img, (2, 2), 1, 1, 1)
    assert img.tolist() == [[0] * 5, [0, 0, 1, 0, 0], [0, 1, 0, 1, 0], [0, 0, 1, 0, 0], [0] * 5]
    img = np.zeros((3, 4), np.uint8)                                 # clipped by the corner, and a centre outside the image
    ref.circle(img, (0, 0), 1, 1, 1)
    ref.circle(img, (4, 2), 1, 1, 1)
    assert img.tolist() == [[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1]]


def test_restated_get_max_preds_ties_and_negative_maps():
    hm = np.full((1, 3, 4, 6), -1.0, np.float32)
    hm[0, 0, 1, 5] = hm[0, 0, 3, 0] = hm[0, 0, 1, 2] = 2.0           # ties: the first in row-major order wins -> (2, 1)
    hm[0, 1, 3, 5] = 0.5
    p, m = ref.get_max_preds(hm)                                     # map 2 is all negative: zeroed coordinates, the max kept
    assert p.dtype == np.float32 and p[0].tolist() == [[2, 1], [5, 3], [0, 0]] and m[0, :, 0].tolist() == [2.0, 0.5, -1.0]
    hm[0, 2, 2, 3] = 0.0                                             # a maximum of exactly 0 is zeroed too
    assert ref.get_max_preds(hm)[0][0, 2].tolist() == [0, 0]


# ---- the host build of csrc/vis_math.h against the restatement ----

def test_host_blend_is_numpys_for_every_pair_and_the_check_discriminates(host_lib):
    out = np.zeros((256, 256), np.uint8)
    host_lib.vis_blend_all_host(out.ctypes.data_as(C.c_void_p))
    c, r = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    want = np.zeros((256, 256), np.uint8)
    want[:, :] = c * 0.7 + r * 0.3                                   # as vis.py:102,109: float64, assigned into uint8
    assert np.array_equal(out, want)
    f32 = (c.astype(np.float32) * np.float32(0.7) + r.astype(np.float32) * np.float32(0.3)).astype(np.uint8)
    tenths = ((7 * c.astype(np.int32) + 3 * r.astype(np.int32)) // 10).astype(np.uint8)
    assert int((f32 != want).sum()) == 1415 and int((tenths != want).sum()) == 1271


def _norm_bytes_ref(x, normalize=True):
    t = torch.from_numpy(x.copy())
    if normalize:
        ref.norm_ip(t, float(t.min()), float(t.max()))
    return t.mul(255).clamp(0, 255).byte().numpy()


def _norm_bytes_host(host_lib, x, normalize=True):
    out = np.zeros(x.shape, np.uint8)
    host_lib.vis_norm_bytes_host(x.ctypes.data_as(C.c_void_p), x.size, float(x.min()), float(x.max()), int(normalize),
                                 out.ctypes.data_as(C.c_void_p))
    return out


def test_host_normalise_and_byte_is_the_torch_chain_bit_for_bit(host_lib):
    rng = np.random.RandomState(7)
    cases = [rng.standard_normal(40000).astype(np.float32) * s + o for s, o in ((1, 0), (0.3, 2), (50, -7), (1e-6, 0))]
    cases.append(np.full(100, 0.25, np.float32))                     # constant image: max == min, d = float32(1e-5)
    cases.append(np.zeros(100, np.float32))
    k = np.arange(256, dtype=np.float32)                             # values at the byte boundaries k / 255 and their neighbours
    edge = np.concatenate([k / np.float32(255), np.nextafter(k / np.float32(255), np.float32(-1)),
                           np.nextafter(k / np.float32(255), np.float32(2)), np.float32([0.0, 1.0 + 1e-5])])
    cases.append(edge.astype(np.float32))
    cases.append((edge * 3 - 1).astype(np.float32))
    for x in cases:
        assert np.array_equal(_norm_bytes_host(host_lib, x), _norm_bytes_ref(x)), (x.min(), x.max())
    for x in (cases[0], edge.astype(np.float32), np.float32([-0.0, -3.0, 0.5, 2.0, 0.999999, 1.0])):
        assert np.array_equal(_norm_bytes_host(host_lib, x, False), _norm_bytes_ref(x, False))
        out = np.zeros(x.shape, np.uint8)
        host_lib.vis_heat_bytes_host(x.ctypes.data_as(C.c_void_p), x.size, out.ctypes.data_as(C.c_void_p))
        assert np.array_equal(out, torch.from_numpy(x).mul(255).clamp(0, 255).byte().numpy())


def test_host_coordinate_truncation_marks_and_resize(host_lib):
    rng = np.random.RandomState(3)
    joints = np.concatenate([rng.uniform(-40, 40, 500), [-0.5, -1.0, -1.5, -0.999, 0.999, 0.0, -17.000001, 13.5, 1e6, -1e6]])
    for cell, extent, padding in ((0, 12, 2), (3, 12, 2), (1, 16, 0), (7, 256, 2)):
        for j in joints:
            want = int(cell * (extent + padding) + padding + np.float64(j))           # vis.py:46-49
            assert host_lib.vis_mark_pos_host(cell, extent, padding, float(j)) == want, (cell, extent, padding, j)
    for v, want in ((-0.9, 0), (-1.0, -1), (2.999, 2), (-2.5, -2), (float('nan'), -(1 << 30)), (1e300, 1 << 30), (-1e300, -(1 << 30))):
        assert host_lib.vis_trunc_host(v) == want
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            assert host_lib.vis_in_ring_host(dx, dy) == int(1 <= dx * dx + dy * dy <= 9)
            assert host_lib.vis_in_cross_host(dx, dy) == int(dx * dx + dy * dy == 1)
    assert host_lib.vis_in_cross_host(1 << 30, 1) == 0 and host_lib.vis_in_ring_host(-(1 << 30), 0) == 0
    for a, b, c, d in rng.randint(0, 256, (300, 4)).tolist() + [[255] * 4, [0, 0, 0, 1], [0, 0, 1, 1]]:
        img = np.zeros((4, 4, 1), np.uint8)
        img[1, 1, 0], img[1, 2, 0], img[2, 1, 0], img[2, 2, 0] = a, b, c, d
        assert host_lib.vis_resize4_host(a, b, c, d) == int(ref.resize4(img, (1, 1))[0, 0, 0])


def test_the_header_walks_its_cases_clean_under_the_host_sanitizers(tmp_path):
    """The same text with a small main, built with -fsanitize=address,undefined and run as a program of its own."""
    exe = str(tmp_path / 'vis_san')
    subprocess.check_call([_cxx(), '-O1', '-g', '-ffp-contract=off', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DVIS_MAIN', '-I' + CSRC, SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b'cases ok' in r.stdout, r.stdout.decode()


# ---- the ABI without a device ----

def test_abi_has_the_vis_entry_points_and_they_refuse_bad_arguments_without_a_device():
    from fpd_amd import runtime as R
    lib = R.lib()
    err = lambda: lib.fpd_last_error().decode()  # noqa: E731
    assert lib.fpd_abi_version() == 2
    assert lib.fpd_abi_sizeof(b'fpd_vis_minmax_t') == C.sizeof(R.VisMinmaxT) == 24
    assert lib.fpd_abi_sizeof(b'fpd_vis_max_preds_t') == C.sizeof(R.VisMaxPredsT) == 48
    assert lib.fpd_abi_sizeof(b'fpd_vis_joints_grid_t') == C.sizeof(R.VisJointsGridT) == 88
    assert lib.fpd_abi_sizeof(b'fpd_vis_heatmap_grid_t') == C.sizeof(R.VisHeatmapGridT) == 96
    # every case below is refused before a launch: the pointers are never dereferenced

    def mm():
        a = R.VisMinmaxT()
        a.n, a.x, a.out = 10, 0x1000, 0x2000
        return a
    for f in ('x', 'out'):
        a = mm()
        setattr(a, f, None)
        assert lib.fpd_vis_minmax(a, None) < 0 and 'null' in err(), f
    a = mm()
    a.n = 0
    assert lib.fpd_vis_minmax(a, None) < 0 and 'positive' in err()
    assert lib.fpd_vis_minmax(None, None) < 0

    def mp():
        a = R.VisMaxPredsT()
        a.N, a.J, a.h, a.w, a.dtype, a.layout = 2, 3, 4, 6, R.F32, R.VIS_NCHW
        a.hm, a.preds, a.maxvals = 0x1000, 0x2000, 0x3000
        return a
    for f in ('hm', 'preds', 'maxvals'):
        a = mp()
        setattr(a, f, None)
        assert lib.fpd_vis_max_preds(a, None) < 0 and 'null' in err(), f
    a = mp()
    a.dtype = R.BF16                                                # NCHW maps are float32
    assert lib.fpd_vis_max_preds(a, None) < 0 and 'dtype' in err()
    a = mp()
    a.layout = 2
    assert lib.fpd_vis_max_preds(a, None) < 0 and 'layout' in err()

    def jg():
        a = R.VisJointsGridT()
        a.N, a.H, a.W, a.J, a.nrow, a.padding, a.joints_f64, a.joints_stride, a.coord_scale = 3, 16, 12, 4, 2, 2, 1, 3, 1.0
        a.canvas_bytes = 38 * 30 * 3
        a.image, a.minmax, a.joints, a.vis, a.canvas = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
        return a
    for f in ('image', 'minmax', 'joints', 'vis', 'canvas'):
        a = jg()
        setattr(a, f, None)
        assert lib.fpd_vis_joints_grid(a, None) < 0 and 'null' in err(), f
    a = jg()
    a.nrow = 0
    assert lib.fpd_vis_joints_grid(a, None) < 0 and 'nrow' in err()
    a = jg()
    a.padding = -1
    assert lib.fpd_vis_joints_grid(a, None) < 0 and 'padding' in err()
    a = jg()
    a.canvas_bytes -= 1
    assert lib.fpd_vis_joints_grid(a, None) < 0 and 'canvas_bytes' in err()
    a = jg()
    a.N, a.canvas_bytes = 1, 18 * 14 * 3                            # a single image is the bare 16 x 12 canvas
    assert lib.fpd_vis_joints_grid(a, None) < 0 and 'canvas_bytes' in err()
    for f in ('image', 'minmax', 'joints', 'vis'):
        a = jg()
        a.canvas = getattr(a, f)
        assert lib.fpd_vis_joints_grid(a, None) < 0 and 'alias' in err(), f

    def hg():
        a = R.VisHeatmapGridT()
        a.N, a.J, a.h, a.w, a.H, a.W, a.dtype, a.layout, a.normalize = 2, 3, 4, 6, 16, 24, R.F32, R.VIS_NCHW, 1
        a.canvas_bytes = 2 * 4 * 4 * 6 * 3
        a.image, a.minmax, a.hm, a.preds, a.table, a.canvas = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
        return a
    for f in ('image', 'minmax', 'hm', 'preds', 'table', 'canvas'):
        a = hg()
        setattr(a, f, None)
        assert lib.fpd_vis_heatmap_grid(a, None) < 0 and 'null' in err(), f
    for f, v in (('H', 17), ('W', 20), ('h', 5)):
        a = hg()
        setattr(a, f, v)
        assert lib.fpd_vis_heatmap_grid(a, None) < 0 and 'not 4x' in err(), f
    a = hg()
    a.J = R.MAX_JOINTS + 1
    assert lib.fpd_vis_heatmap_grid(a, None) < 0 and 'J <=' in err()
    a = hg()
    a.canvas_bytes += 3
    assert lib.fpd_vis_heatmap_grid(a, None) < 0 and 'canvas_bytes' in err()
    for f in ('image', 'minmax', 'hm', 'preds', 'table'):
        a = hg()
        a.canvas = getattr(a, f)
        assert lib.fpd_vis_heatmap_grid(a, None) < 0 and 'alias' in err(), f


# ---- save_debug_images with the renderer stubbed ----

class _Node(dict):
    __getattr__ = dict.__getitem__


def _config(debug=True, gt=False, pred=False, hm_gt=False, hm_pred=False):
    return _Node(DEBUG=_Node(DEBUG=debug, SAVE_BATCH_IMAGES_GT=gt, SAVE_BATCH_IMAGES_PRED=pred, SAVE_HEATMAPS_GT=hm_gt,
                             SAVE_HEATMAPS_PRED=hm_pred))


@pytest.fixture
def stubbed(monkeypatch):
    """utils.vis with the four device calls replaced: the canvases are host tensors whose size names the call."""
    from fpd_amd.lib.utils import vis
    calls = []

    def joints(image, batch_joints, vis_, nrow=8, padding=2, coord_scale=1.0, minmax=None):
        calls.append(('joints', batch_joints, coord_scale, minmax))
        return torch.full((10, 20, 3), 7, dtype=torch.uint8)

    def heat(image, hm, normalize=True, minmax=None, preds=None):
        calls.append(('heat', hm, preds, minmax))
        return torch.full((12, 8, 3), 9, dtype=torch.uint8)
    monkeypatch.setattr(vis, 'image_minmax', lambda x: 'MM')
    monkeypatch.setattr(vis, 'max_preds', lambda hm: ('PREDS', 'MAXVALS'))
    monkeypatch.setattr(vis, 'render_image_with_joints', joints)
    monkeypatch.setattr(vis, 'render_heatmaps', heat)
    return vis, calls


def test_save_debug_images_flags_and_file_names(stubbed, tmp_path):
    from PIL import Image
    vis, calls = stubbed
    meta = {'joints': 'J', 'joints_vis': 'V'}
    names = {'gt': 'p_gt.jpg', 'pred': 'p_pred.jpg', 'hm_gt': 'p_hm_gt.jpg', 'hm_pred': 'p_hm_pred.jpg'}
    sizes = {'gt': (20, 10), 'pred': (20, 10), 'hm_gt': (8, 12), 'hm_pred': (8, 12)}
    for on in (['gt'], ['pred'], ['hm_gt'], ['hm_pred'], ['gt', 'hm_pred'], list(names)):
        d = tmp_path / '_'.join(on)
        d.mkdir()
        del calls[:]
        vis.save_debug_images(_config(True, **{k: True for k in on}), 'IN', meta, 'TGT', None, 'OUT', str(d / 'p'))
        assert sorted(os.listdir(str(d))) == sorted(names[k] for k in on)
        for k in on:
            assert Image.open(str(d / names[k])).size == sizes[k]
        assert all(c[3] == 'MM' for c in calls)                       # one min/max pair for every canvas of the call
        if 'pred' in on:                                              # get_max_preds(output) * 4
            assert ('joints', 'PREDS', 4.0, 'MM') in calls
        if 'gt' in on:
            assert ('joints', 'J', 1.0, 'MM') in calls
        if 'hm_gt' in on:
            assert ('heat', 'TGT', None, 'MM') in calls
        if 'hm_pred' in on:
            assert ('heat', 'OUT', 'PREDS', 'MM') in calls
    del calls[:]
    d = tmp_path / 'given'
    d.mkdir()
    vis.save_debug_images(_config(True, pred=True), 'IN', meta, 'TGT', 'GIVEN', 'OUT', str(d / 'p'))
    assert calls == [('joints', 'GIVEN', 1.0, 'MM')]                  # the caller's pred*4 is drawn as it is


def test_save_debug_images_does_nothing_when_off(stubbed, tmp_path):
    vis, calls = stubbed
    assert vis.save_debug_images(_config(False, True, True, True, True), 'IN', None, 'TGT', None, 'OUT', str(tmp_path / 'p')) is None
    vis.save_debug_images(_config(True), 'IN', None, 'TGT', None, 'OUT', str(tmp_path / 'p'))       # DEBUG on, no flag
    assert calls == [] and os.listdir(str(tmp_path)) == []


def test_save_debug_images_refuses_a_loader_without_joints(stubbed, tmp_path):
    from fpd_amd.runtime import FpdError
    vis, calls = stubbed
    with pytest.raises(FpdError, match="meta\\['joints'\\]"):
        vis.save_debug_images(_config(True, gt=True), 'IN', {'center': 0}, 'TGT', None, 'OUT', str(tmp_path / 'p'))
    with pytest.raises(FpdError, match="meta\\['joints_vis'\\]"):
        vis.save_debug_images(_config(True, pred=True), 'IN', {'joints': 0}, 'TGT', None, 'OUT', str(tmp_path / 'p'))
    assert calls == [] and os.listdir(str(tmp_path)) == []
    vis.save_debug_images(_config(True, hm_gt=True), 'IN', {'center': 0}, 'TGT', None, 'OUT', str(tmp_path / 'p'))    # needs no joints
    assert os.listdir(str(tmp_path)) == ['p_hm_gt.jpg']


def test_public_functions_refuse_cpu_tensors():
    from fpd_amd.lib.utils import vis
    from fpd_amd.runtime import FpdError
    img, hm = torch.zeros(1, 3, 16, 16), torch.zeros(1, 2, 4, 4)
    with pytest.raises(FpdError, match='no CPU path'):
        vis.save_batch_heatmaps(img, hm, 'x.jpg')
    with pytest.raises(FpdError, match='no CPU path'):
        vis.save_batch_image_with_joints(img, torch.zeros(1, 2, 3), torch.ones(1, 2, 1), 'x.jpg')


# ---- AsyncImageWriter ----

def test_async_writer_files_equal_the_direct_pil_call(tmp_path):
    import io

    from PIL import Image

    from fpd_amd.lib.utils.vis import AsyncImageWriter
    rng = np.random.RandomState(11)
    canvases = [rng.randint(0, 256, s + (3,)).astype(np.uint8) for s in ((38, 30), (8, 24), (1, 1))]
    w = AsyncImageWriter()
    for k, c in enumerate(canvases):
        w.put(str(tmp_path / ('c%d.jpg' % k)), c)
    w.close()
    w.close()                                                         # idempotent
    for k, c in enumerate(canvases):
        path = str(tmp_path / ('c%d.jpg' % k))
        assert Image.open(path).size == (c.shape[1], c.shape[0])
        direct = io.BytesIO()
        Image.fromarray(c[:, :, ::-1]).save(direct, format='JPEG', quality=95)
        with open(path, 'rb') as f:
            assert f.read() == direct.getvalue()
    with pytest.raises(Exception):
        w.put('x.jpg', canvases[0])


def test_async_writer_close_reraises_the_workers_error(tmp_path):
    from fpd_amd.lib.utils.vis import AsyncImageWriter
    w = AsyncImageWriter()
    w.put(str(tmp_path / 'no_such_dir' / 'c.jpg'), np.zeros((4, 4, 3), np.uint8))
    w.put(str(tmp_path / 'after.jpg'), np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(FileNotFoundError):
        w.close()
    assert not os.path.exists(str(tmp_path / 'after.jpg'))            # nothing is written after a failure
    w.close()                                                         # the error was handed over once
