"""Preconditions of tests/test_teacher_persistent_gpu.py, checked without a device, for every case of tests/_teacher_cases.py:
  * grid split: every row of the case tables has the properties it names (several tiles per block, ranges that start
    mid-image, the proportional pair split, the head's permutation, ...) under a restatement of the launch arithmetic;
  * storage equality: on the exact inputs the interpreter with fp32 storage equals the interpreter with bf16 storage bit for bit
    on every compared buffer (Bottleneck y; head score and next) -- by construction, not by single rounding;
  * non-degeneracy: every compared buffer has non-zero entries and every ReLU clamps some but not all of what it sees."""
import pytest
import torch

from tests import _teacher_cases as T

BNECK = sorted({(shape, P) for shape, _, P in T.bneck_params()})
PAIRS = [(a, b, P) for a, b, P, _, _ in T.PAIR_CASES]
HEADS = sorted({(shape, nx) for shape, _, _ in T.HEAD_CASES for nx in (True, False)})
_ids = lambda v: '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize('row', T.BNECK_CASES, ids=lambda r: '%s-cap%s' % (_ids(r[0]), r[1]))
def test_bottleneck_rows_have_their_properties(row):
    T.check_bneck_row(row)
    if row[1] is not None:                               # a capped row is there for the persistent loop, whatever else it names
        assert 'several tiles in every block' in row[3] and T.ntiles(*row[0]) > row[1]


@pytest.mark.parametrize('row', T.PAIR_CASES, ids=lambda r: '%s+%s-cap%s' % (_ids(r[0]), _ids(r[1]), r[3]))
def test_pair_rows_have_their_properties(row):
    T.check_pair_row(row)
    assert 'proportional split' in row[4] and 'several tiles in every block' in row[4]


@pytest.mark.parametrize('row', T.HEAD_CASES, ids=lambda r: '%s-cap%s' % (_ids(r[0]), r[1]))
def test_head_rows_have_their_properties(row):
    T.check_head_row(row)
    if row[1] is not None:
        assert 'several tiles in every block' in row[2] and T.ntiles(*row[0]) > row[1]


def test_split_restatement_on_known_grids():
    """The restatement itself, on the grids the step launches at batch 32 and on the tables' rows worked out by hand."""
    assert T.bneck_blocks(1024, 128) == 128 and T.head_blocks(1024, 160) == 147          # 8 tiles / up to 7 tiles per block
    assert [e - b for b, e in T.bneck_ranges(24, T.bneck_blocks(24, 5))] == [4, 5, 5, 5, 5]
    assert [e - b for b, e in T.bneck_ranges(10, T.bneck_blocks(10, 3))] == [3, 3, 4]
    assert T.bneck_ranges(14, T.bneck_blocks(14, 1)) == [(0, 14)]
    assert T.bneck_ranges(9, T.bneck_blocks(9, 2)) == [(0, 4), (4, 9)]
    assert T.bneck_blocks(160, 128) == 80 and T.head_blocks(192, 160) == 96
    assert T.pair_split(24, 6, 8) == (6, 1) and T.pair_split(64, 16, 8) == (7, 1) and T.pair_split(6, 2, 128) == (6, 2)
    assert T.head_walk(16, 3)[0] == [0, 6, 12, 3, 9, 15] and [len(w) for w in T.head_walk(10, 4)] == [3, 3, 2, 2]
    assert T.head_walk(10, 4)[1] == [1, 5, 9]


def _storage_pair(build):
    """-> (case, bf16 arenas, fp32 arenas) of the same constructed inputs, both run through the interpreter"""
    bt = T.CpuBench(1)
    c = build(bt)
    bt.realise().run(c.ops)
    f = T.CpuBench(0)
    f.sizes, f.fills = dict(bt.sizes), list(bt.fills)
    f.realise().run(c.ops)
    return c, bt.cpu, f.cpu


def _check_exact_case(build, label):
    c, A16, A32 = _storage_pair(build)
    for name, act in c.compare:
        v16, v32 = A16.view(act.buf).double(), A32.view(act.buf).double()
        assert torch.equal(v16, v32), '%s %s: fp32 and bf16 storage differ in %d elements' % (label, name, int((v16 != v32).sum()))
        assert float(v16.abs().max()) > 0 and float((v16 != 0).float().mean()) > 0.25, '%s %s: degenerate output' % (label, name)
    shares = T.clamp_shares(A16, c)
    assert shares == T.clamp_shares(A32, c)
    msg = '%s: ReLU clamp shares %s' % (label, ', '.join('%s %.1f %%' % (n, 100 * s) for n, s in shares))
    print(msg)
    assert all(0.05 < s < 0.95 for _, s in shares), msg
    return shares


@pytest.mark.parametrize('shape,P', BNECK, ids=_ids)
def test_bottleneck_exact_inputs(shape, P):
    _check_exact_case(lambda bt: T.bneck_case(bt, shape, P, False, True), 'bneck %r P=%d' % (shape, P))


@pytest.mark.parametrize('a,b,P', PAIRS, ids=_ids)
def test_pair_exact_inputs(a, b, P):
    _check_exact_case(lambda bt: T.pair_case(bt, a, b, P, False, True), 'pair %r + %r P=%d' % (a, b, P))


@pytest.mark.parametrize('shape,has_next', HEADS, ids=_ids)
def test_head_exact_inputs(shape, has_next):
    build = lambda bt: T.head_case(bt, shape, has_next, False, True)
    _check_exact_case(build, 'head %r next=%s' % (shape, has_next))
    if has_next:                                         # the bound of the module docstring: 8 significant bits suffice
        c, A16, _ = _storage_pair(build)
        nxt = A16.view(c.members[0].next.buf).double()
        assert torch.equal(nxt * 8, torch.round(nxt * 8)) and float(nxt.abs().max()) * 8 < 256
