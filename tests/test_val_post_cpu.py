"""The fused validation step, the parts that need no GPU: a HOST build of the kernel's per-sample arithmetic
(csrc/val_post_math.h) against utils.transforms.get_affine_transform(..., inv=1) bit for bit, the same text under the host
sanitizers as a stand-alone program, the ABI surface and refusals of fpd_val_post, the 'block' partition of the validation
loader and dist.make_gather over gloo."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'fast-human-pose-estimation.pytorch_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'native', 'val_post_host.cpp')
SIZES = [(64, 64), (48, 64), (72, 96), (64, 48), (96, 72), (4, 16), (8, 8), (12, 16), (5, 40)]      # (W, H) of the heat map


def _cxx():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler for the host build of csrc/val_post_math.h')
    return cxx


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('valpost') / 'libval_post_host.so')
    subprocess.check_call([_cxx(), '-O2', '-ffp-contract=off', '-Wno-unknown-pragmas', '-shared', '-fPIC', '-I' + CSRC, SRC, '-o', so])
    lib = C.CDLL(so)
    lib.val_box_area_host.restype = C.c_double
    return lib


def seeded_boxes(seed, n, f32):
    """n centres and scales as a dataset delivers them (float64, or float32 for COCO's _box2cs); sample 0 has scale 0,
    sample 1 a zero width only."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-50, 900, (n, 2))
    s = rng.uniform(0.05, 4.0, (n, 2))
    s[0] = 0.0
    s[1, 0] = 0.0
    dt = np.float32 if f32 else np.float64
    return c.astype(dt), s.astype(dt)


@pytest.mark.parametrize('f32', [0, 1])
@pytest.mark.parametrize('size', SIZES)
def test_host_build_of_the_inverse_affine_is_numpys_bit_for_bit(host_lib, size, f32):
    from fpd_amd.lib.utils.transforms import get_affine_transform
    w, h = size
    c, s = seeded_boxes(w * 1000 + h + f32, 300, f32)
    for k in range(len(c)):
        ref = get_affine_transform(c[k], s[k], 0, [w, h], inv=1)
        cd, sd, t = c[k].astype(np.float64), s[k].astype(np.float64), np.zeros(6)
        host_lib.val_inverse_affine_host(cd.ctypes.data_as(C.c_void_p), sd.ctypes.data_as(C.c_void_p), f32, w, h,
                                         t.ctypes.data_as(C.c_void_p))
        assert ref.dtype == np.float64 and t.tobytes() == ref.tobytes(), (size, f32, k, c[k], s[k], t.reshape(2, 3) - ref)
        area = host_lib.val_box_area_host(sd.ctypes.data_as(C.c_void_p), f32)
        assert np.float64(area).tobytes() == np.float64(np.prod(s[k] * 200)).tobytes(), (size, f32, k)


def test_the_header_walks_seeded_cases_clean_under_the_host_sanitizers(tmp_path):
    """The same text with a small main, built with -fsanitize=address,undefined and run as a program of its own."""
    exe = str(tmp_path / 'val_post_san')
    subprocess.check_call([_cxx(), '-O1', '-g', '-ffp-contract=off', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DVAL_POST_MAIN', '-I' + CSRC, SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b'cases ok' in r.stdout, r.stdout.decode()


def test_abi_has_val_post_and_it_refuses_bad_arguments_without_a_device():
    from fpd_amd import runtime as R
    lib = R.lib()
    assert lib.fpd_abi_sizeof(b'fpd_val_post_t') == C.sizeof(R.ValPostT) > 0
    assert hasattr(lib, 'fpd_val_post')

    def args():
        a = R.ValPostT()
        a.N, a.J, a.H, a.W, a.dtype, a.rows = 2, 16, 8, 8, R.F32, 2
        a.a, a.b, a.merged = 0x1000, 0x2000, 0x3000            # never dereferenced: every case is refused before a launch
        a.center, a.scale, a.score, a.all_preds, a.all_boxes = 0x4000, 0x5000, 0x6000, 0x7000, 0x8000
        for j in range(16):
            a.src[j] = j
        return a
    for field in ('a', 'center', 'scale', 'score', 'merged', 'all_preds', 'all_boxes'):
        a = args()
        setattr(a, field, None)
        assert lib.fpd_val_post(a, None) < 0 and b'null' in lib.fpd_last_error(), field
    assert lib.fpd_val_post(None, None) < 0
    a = args()
    a.J = R.MAX_JOINTS + 1
    assert lib.fpd_val_post(a, None) < 0 and b'J <=' in lib.fpd_last_error()
    for other in ('a', 'b'):
        a = args()
        a.merged = getattr(a, other)
        assert lib.fpd_val_post(a, None) < 0 and b'alias' in lib.fpd_last_error(), other
    a = args()
    a.row0 = -1
    assert lib.fpd_val_post(a, None) < 0 and b'negative' in lib.fpd_last_error()
    a = args()
    a.row0 = 1                                                 # rows 1..2 of 2
    assert lib.fpd_val_post(a, None) < 0 and b'outside' in lib.fpd_last_error()
    a = args()
    a.src[3] = 16
    assert lib.fpd_val_post(a, None) < 0 and b'src[3]' in lib.fpd_last_error()
    a = args()
    a.dtype = 7
    assert lib.fpd_val_post(a, None) < 0 and b'dtype' in lib.fpd_last_error()


class _StubDB:
    """What DeviceAugmentLoader's constructor looks at, without a device."""
    device = torch.device('cpu')
    joints_weight = None

    def __init__(self, n, row0=0, n_total=None):
        self.n, self.row0, self.n_total = n, row0, n if n_total is None else n_total

    def __len__(self):
        return self.n


def test_block_partition_tiles_the_rows_and_is_validation_only():
    from fpd_amd.lib.config import _defaults
    from fpd_amd.lib.dataset.device_dataset import DeviceAugmentLoader, block_range
    from fpd_amd.runtime import FpdError
    cfg = _defaults()
    for n in (0, 1, 7, 64):
        for world in (1, 2, 5, 8):
            seen = []
            for r in range(world):
                loader = DeviceAugmentLoader(_StubDB(n), cfg, 4, False, rank=r, world_size=world, partition='block')
                lo, hi = loader.rows
                assert (lo, hi) == block_range(n, r, world) == (n * r // world, n * (r + 1) // world)
                assert len(loader) == (hi - lo + 3) // 4
                seen.extend(range(lo, hi))
                # a database that holds just this block serves it; one that holds another block is refused
                assert DeviceAugmentLoader(_StubDB(hi - lo, lo, n), cfg, 4, False, rank=r, world_size=world, partition='block').rows == (lo, hi)
                if hi > lo:
                    with pytest.raises(FpdError):
                        DeviceAugmentLoader(_StubDB(hi - lo, lo + 1, n), cfg, 4, False, rank=r, world_size=world, partition='block')
            assert seen == list(range(n)), (n, world)
    with pytest.raises(FpdError):
        DeviceAugmentLoader(_StubDB(8), cfg, 4, True, partition='block')
    with pytest.raises(FpdError):
        DeviceAugmentLoader(_StubDB(8), cfg, 4, False, shuffle=True, partition='block')
    with pytest.raises(FpdError):
        DeviceAugmentLoader(_StubDB(8), cfg, 4, False, partition='rows')
    assert DeviceAugmentLoader(_StubDB(8), cfg, 4, False).partition == 'strided'          # the default: today's rule
    with pytest.raises(FpdError):
        block_range(4, 2, 2)


def _rank_rows(rank, j):
    """Rank 0 holds dataset rows 0..2, rank 1 rows 3..4; every value names its rank, row and column."""
    rows = np.arange(3) if rank == 0 else np.arange(3, 5)
    preds = (rows[:, None, None] * 100 + np.arange(j)[None, :, None] * 3 + np.arange(3)[None, None, :]).astype(np.float32) + 0.1
    boxes = rows[:, None] * 10.0 + np.arange(6)[None, :] + 1.0 / 3.0
    sums = np.array([1.5 + rank, 3 - rank, 0.25 * (rank + 1), 16 - rank])
    return preds, boxes, rows, sums


def _gather_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from fpd_amd import dist as fdist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    gather = fdist.make_gather(dist)
    got = gather(*_rank_rows(rank, 4))
    perf = gather.broadcast(0.625 if rank == 0 else None)
    q.put((rank, got, perf))
    dist.destroy_process_group()


def test_make_gather_over_gloo_concatenates_unequal_shards_in_rank_order():
    world, port = 2, 30000 + os.getpid() % 500
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    ps = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in ps]
    res = dict((r[0], r[1:]) for r in (q.get(timeout=300) for _ in ps))
    [p.join(60) for p in ps]
    assert res[1][0] is None and res[1][1] == 0.625 and res[0][1] == 0.625
    preds, boxes, rows, sums = res[0][0]
    want = [_rank_rows(r, 4) for r in range(world)]
    assert preds.dtype == np.float32 and preds.shape == (5, 4, 3) and boxes.dtype == np.float64 and rows.dtype == np.int64
    assert preds.tobytes() == np.concatenate([w[0] for w in want]).tobytes()
    assert boxes.tobytes() == np.concatenate([w[1] for w in want]).tobytes()
    assert rows.tolist() == [0, 1, 2, 3, 4]
    assert np.array_equal(sums, np.stack([w[3] for w in want]))
