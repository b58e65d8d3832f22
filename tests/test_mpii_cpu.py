"""The MPII dataset class, the parts that need no GPU (lib/dataset/mpii.py, lib/dataset/device_dataset.epoch_order,
lib/config.py) against the fixture written by the reference's own MPIIDataset (tests/golden/mpii_ref.npz, made by
tests/golden/make_golden_mpii.py) on the tree tests/_mpii_tree.py writes."""
import os

import numpy as np
import pytest

from tests import _mpii_tree as T

G = T.load_golden()


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return T.write_tree(tmp_path_factory.mktemp('mpii'), G, gt=True)


@pytest.mark.parametrize('image_set', ['valid', 'test'])
def test_db_records_equal_the_reference_bit_for_bit(tree, image_set):
    from fpd_amd.lib.dataset import MPIIDataset
    ds = MPIIDataset(T.make_cfg(tree), tree, image_set, False)
    n = len(G['in_image'])
    assert len(ds) == len(ds.db) == n == 12 and len(set(G['in_image'].tolist())) == 5
    assert sorted(ds.db[0]) == ['center', 'filename', 'image', 'imgnum', 'joints_3d', 'joints_3d_vis', 'scale']
    for k in ('center', 'scale', 'joints_3d', 'joints_3d_vis'):
        got = np.stack([rec[k] for rec in ds.db])
        want = G['%s/%s' % (image_set, k)]
        assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
        assert got.tobytes() == want.tobytes(), (image_set, k, np.abs(got - want).max())
    assert [os.path.relpath(rec['image'], tree) for rec in ds.db] == G[image_set + '/image'].tolist()
    assert [rec['filename'] for rec in ds.db] == G[image_set + '/filename'].tolist() == [''] * n
    assert [rec['imgnum'] for rec in ds.db] == G[image_set + '/imgnum'].tolist() == [0] * n
    # the placeholder record kept its scale and only lost the 1-based offset; every other box grew
    i = int(np.flatnonzero(G['in_center'][:, 0] == -1)[0])
    assert ds.db[i]['center'].tolist() == [-2.0, -2.0] and ds.db[i]['scale'].tolist() == [G['in_scale'][i]] * 2
    assert all(ds.db[k]['scale'][0] == G['in_scale'][k] * 1.25 for k in range(n) if k != i)
    if image_set == 'test':
        assert not G['test/joints_3d'].any() and not G['test/joints_3d_vis'].any()
    else:
        assert set(np.unique(G['valid/joints_3d_vis'])) == {0.0, 1.0} and not G['valid/joints_3d_vis'][:, :, 2].any()


def test_class_attributes_and_aspect_ratio(tree):
    from fpd_amd.lib.dataset import MPIIDataset
    cfg = T.make_cfg(tree)
    cfg.MODEL.IMAGE_SIZE = [48, 64]
    ds = MPIIDataset(cfg, tree, 'valid', True)
    assert ds.num_joints == 16 and ds.aspect_ratio == 0.75 and ds.pixel_std == 200
    assert ds.flip_pairs == [[0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13]]
    assert ds.parent_ids == [1, 2, 6, 6, 3, 4, 6, 6, 7, 8, 11, 12, 7, 7, 13, 14]
    assert ds.upper_body_ids == (7, 8, 9, 10, 11, 12, 13, 14, 15) and ds.lower_body_ids == (0, 1, 2, 3, 4, 5, 6)


def test_evaluate_equals_the_reference_pckh(tree, tmp_path):
    """The values are 100 x a ratio of small integers, the means sums of 16 such terms in float64: only the order of a
    summation can differ from the reference's, hence 1e-9."""
    from scipy.io import loadmat
    from fpd_amd.lib.dataset import MPIIDataset
    cfg = T.make_cfg(tree)
    ds = MPIIDataset(cfg, tree, 'valid', False)
    preds = G['in_preds'].copy()
    name_value, indicator = ds.evaluate(cfg, preds, str(tmp_path), None, None)
    assert np.array_equal(preds, G['in_preds'])
    assert type(name_value).__name__ == 'OrderedDict'
    assert list(name_value.keys()) == G['name_value_keys'].tolist() == ['Head', 'Shoulder', 'Elbow', 'Wrist', 'Hip', 'Knee', 'Ankle',
                                                                       'Mean', 'Mean@0.1']
    got = np.array([float(v) for v in name_value.values()])
    print('PCKh', got, 'max deviation', np.abs(got - G['name_value_values']).max())
    assert np.abs(got - G['name_value_values']).max() <= 1e-9
    assert indicator == name_value['Mean'] and abs(float(indicator) - float(G['indicator'])) <= 1e-9
    assert 0 < got.min() and got.max() < 100 and got[8] < got[7]              # joints on both sides of the thresholds
    mat = loadmat(os.path.join(str(tmp_path), 'pred.mat'))['preds']
    want = G['in_preds'][:, :, 0:2] + np.float32(1.0)
    assert mat.dtype == np.float32 and want.dtype == np.float32 and np.array_equal(mat, want) and np.array_equal(mat, G['pred_mat'])
    assert ds.evaluate(cfg, preds, '')[1] == indicator                          # no output_dir: nothing to write


def test_fixture_meets_the_threshold_margin_precondition():
    e, visible = T.scaled_errors(G)
    margin = T.threshold_margin(G)
    print('threshold margin', margin)
    assert len(T.THRESHOLDS) == 51 and margin >= 1e-6
    assert visible.any(axis=1).all() and (e[visible] < 0.5).any() and (e[visible] > 0.5).any()


def test_evaluate_on_the_test_set_returns_null_and_writes_the_predictions(tree, tmp_path):
    from fpd_amd.lib.dataset import MPIIDataset
    cfg = T.make_cfg(tree, TEST_SET='test')
    ds = MPIIDataset(cfg, tree, 'test', False)
    assert ds.evaluate(cfg, G['in_preds'], str(tmp_path)) == ({'Null': 0.0}, 0.0)
    assert os.path.exists(os.path.join(str(tmp_path), 'pred.mat'))


@pytest.mark.parametrize('n', [12, 13])
@pytest.mark.parametrize('world', [1, 2, 3])
def test_rank_slices_partition_the_padded_permutation(n, world):
    from fpd_amd.lib.dataset import epoch_order
    per_rank = (n + world - 1) // world
    for epoch in (0, 1):
        whole = epoch_order(n, 7, epoch, True)[0]
        assert whole.dtype == np.int32 and sorted(whole.tolist()) == list(range(n))
        parts = [epoch_order(n, 7, epoch, True, rank, world)[0] for rank in range(world)]
        assert all(len(p) == per_rank and p.dtype == np.int32 for p in parts)
        merged = np.stack(parts, 1).reshape(-1)                      # rank r took r::world
        pad = per_rank * world - n
        assert np.array_equal(merged[:n], whole) and np.array_equal(merged[n:], whole[:pad])
        if pad == 0:
            assert len(set(merged.tolist())) == n                    # disjoint
        assert set(merged.tolist()) == set(range(n))                 # together they cover everything
    assert not np.array_equal(epoch_order(n, 7, 0, True, 0, world)[0], epoch_order(n, 7, 1, True, 0, world)[0])
    assert np.array_equal(epoch_order(n, 7, 0, False, world - 1, world)[0], np.resize(np.arange(n), per_rank * world)[world - 1::world])


def test_one_process_order_and_draws_are_the_single_generator_of_before_and_ranks_draw_their_own():
    from fpd_amd.lib.dataset import epoch_order
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([3, 2])))
    want = rng.permutation(10).astype(np.int32)
    order, g = epoch_order(10, 3, 2, True)
    assert np.array_equal(order, want) and np.array_equal(g.random(5), rng.random(5))
    draws = [epoch_order(10, 3, 2, True, r, 2)[1].random(4) for r in (0, 1)]
    assert not np.array_equal(draws[0], draws[1])
    assert np.array_equal(draws[1], np.random.Generator(np.random.PCG64(np.random.SeedSequence([3, 2, 1]))).random(4))
    from fpd_amd.runtime import FpdError
    with pytest.raises(FpdError):
        epoch_order(10, 3, 2, True, 2, 2)


def test_a_reference_style_mpii_yaml_loads(tmp_path):
    """The keys of experiments/fpd_mpii/hourglass/*.yaml of the reference that this library had no default for."""
    from fpd_amd.lib.config import _defaults
    import types
    cfg = _defaults()
    d = cfg.DATASET
    assert (d.DATA_FORMAT, d.COLOR_RGB, d.SELECT_DATA, d.CACHE_ROOT, d.HYBRID_JOINTS_TYPE) == ('jpg', False, False, '', '')
    path = tmp_path / 'hg4.yaml'
    path.write_text('''AUTO_RESUME: false
GPUS: (0,)
WORKERS: 12
DATASET:
  COLOR_RGB: true
  DATASET: mpii
  DATA_FORMAT: jpg
  CACHE_ROOT: 'data/cache'
  SELECT_DATA: false
  HYBRID_JOINTS_TYPE: ''
  FLIP: true
  NUM_JOINTS_HALF_BODY: 8
  PROB_HALF_BODY: -1.0
  ROOT: 'data/mpii/'
  ROT_FACTOR: 30
  SCALE_FACTOR: 0.25
  TEST_SET: valid
  TRAIN_SET: train
MODEL:
  NAME: hourglass
  NUM_JOINTS: 16
  IMAGE_SIZE:
  - 256
  - 256
  HEATMAP_SIZE:
  - 64
  - 64
  EXTRA:
    NUM_FEATURES: 128
    NUM_STACKS: 4
KD:
  TRAIN_TYPE: FPD
  ALPHA: 0.5
''')
    from fpd_amd.lib.config import update_config
    update_config(cfg, types.SimpleNamespace(cfg=str(path), opts=['DATASET.ROOT', str(tmp_path)]))
    assert cfg.DATASET.DATASET == 'mpii' and cfg.DATASET.COLOR_RGB is True and cfg.DATASET.CACHE_ROOT == 'data/cache'
    assert cfg.DATASET.ROOT == str(tmp_path) and cfg.WORKERS == 12 and cfg.MODEL.EXTRA.NUM_STACKS == 4
    assert _defaults().DATASET.DATASET == 'synthetic' and _defaults().DATASET.PROB_HALF_BODY == 0.0


def test_unsupported_settings_and_a_missing_image_raise(tree, tmp_path):
    import shutil
    from fpd_amd.lib.dataset import MPIIDataset
    from fpd_amd.lib.dataset.mpii import image_shape, read_image
    from fpd_amd.runtime import FpdError
    with pytest.raises(FpdError, match='zip'):
        MPIIDataset(T.make_cfg(tree, DATA_FORMAT='zip'), tree, 'valid', False)
    with pytest.raises(FpdError, match='SELECT_DATA'):
        MPIIDataset(T.make_cfg(tree, SELECT_DATA=True), tree, 'train', True)
    with pytest.raises(FpdError, match='nowhere.json'):
        MPIIDataset(T.make_cfg(tree), tree, 'nowhere', False)
    gone = os.path.join(tree, 'images', 'absent.jpg')
    for f in (image_shape, read_image):
        with pytest.raises(FpdError, match='absent.jpg'):
            f(gone)
    bad = str(tmp_path / 'float.npy')
    np.save(bad, np.zeros((4, 5, 3), np.float32))
    with pytest.raises(FpdError, match='float.npy'):
        read_image(bad)
    assert image_shape(os.path.join(tree, 'images', 'im1.npy')) == T.IMAGE_SHAPES[1]
    assert np.array_equal(read_image(os.path.join(tree, 'images', 'im1.npy')), T.image(1))
    # through to_device as well, before anything touches a device: the shapes are read first
    broken = str(tmp_path / 'broken')
    shutil.copytree(tree, broken)
    os.remove(os.path.join(broken, 'images', 'im3.npy'))
    with pytest.raises(FpdError, match='im3.npy'):
        MPIIDataset(T.make_cfg(broken), broken, 'valid', False).to_device('cuda')


def test_a_png_decodes_to_bgr_and_to_rgb_with_color_rgb(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from fpd_amd.lib.dataset.mpii import image_shape, read_image
    rgb = np.zeros((7, 9, 3), np.uint8)
    rgb[..., 0], rgb[..., 1], rgb[..., 2] = 200, np.arange(9)[None, :] * 3, np.arange(7)[:, None] + 100
    path = str(tmp_path / 'planes.png')
    Image.fromarray(rgb).save(path)
    assert image_shape(path) == (7, 9)
    bgr = read_image(path)
    assert bgr.dtype == np.uint8 and bgr.flags['C_CONTIGUOUS'] and np.array_equal(bgr, rgb[:, :, ::-1])
    assert np.array_equal(read_image(path, color_rgb=True), rgb)
    # EXIF orientation is not applied (IMREAD_IGNORE_ORIENTATION): a JPEG tagged "rotated 90 degrees" keeps its stored shape
    exif = Image.Exif()
    exif[0x0112] = 6
    jpg = str(tmp_path / 'turned.jpg')
    Image.fromarray(rgb).save(jpg, exif=exif)
    assert image_shape(jpg) == (7, 9) and read_image(jpg).shape == (7, 9, 3)
