"""Preconditions of the bit-exact device tests (tests/test_exact_stream_gpu.py, tests/test_exact_stem_gpu.py,
tests/test_exact_tile_gpu.py), checked without a device: for every input
construction of tests/_exact_inputs.py and every case of its lists
  * the BatchNorm coefficient identities hold bit for bit -- in the interpreter and in the arithmetic of the device (statistics
    through the limb split, eps = (double)(float)1e-5): invstd == 1.0f, scale == gamma, shift == beta - mu*gamma, mean == mu, and
    the folded apply's A == gamma, B == -gamma*m2, D == gamma*(mu*m2 - m1);
  * the headroom, non-degeneracy, mask-share and mask-boundary assertions of check_reference() pass;
  * with 'sparse' weights the interpreter with fp32 storage equals the interpreter with bf16 storage bit for bit on every
    compared buffer (with 'dense' weights the bf16 result is the single rounding of an exact fp32 accumulator).
So an edit of a case list cannot silently turn an exact test into a rounding lottery."""
import pytest
import torch

from oracle import plan_interp as PI
from tests import _exact_inputs as X

PARAMS = [pytest.param(fn, p, id='%s-%s' % (fn.__name__, '-'.join(str(v) for v in p))) for fn, ps in X.FAMILIES for p in ps]


def _view(A, b):
    return A.view(b.buf if hasattr(b, 'buf') else b)


@pytest.mark.parametrize('fn,params', PARAMS)
def test_inputs_are_exact_for_the_specification(fn, params):
    bt = X.CpuBench(1)
    b = fn(bt, *params)
    bt.realise().run(b.ops)
    A = bt.cpu
    X.check_reference(A, b, fn.__name__)
    for bn, ex in b.bns.items():                          # the device's arithmetic on the device's representation of the sums
        for eps in (PI.EPS, X.EPS_DEVICE):
            sc, sh, mu, inv = X.device_bn_coef(A.view(bn.stats), A.view(bn.gamma), A.view(bn.beta), bn.count, eps)
            assert torch.equal(sc.double(), ex['gamma']) and torch.equal(sh.double(), ex['shift'])
            assert torch.equal(mu.double(), ex['mu']) and bool((inv == 1.0).all())
    for ap, (m1, m2) in b.applies.items():
        ex = b.bns[ap.bn]
        for eps in (PI.EPS, X.EPS_DEVICE):
            ca, cb, cd = X.device_fold_coef(A.view(ap.bn.stats), A.view(ap.bstats), A.view(ap.bn.gamma), ap.bn.count, eps)
            assert torch.equal(ca.double(), ex['gamma']) and torch.equal(cb.double(), -ex['gamma'] * m2)
            assert torch.equal(cd.double(), ex['gamma'] * (ex['mu'] * m2 - m1))
    if 'sparse' in params:
        f = X.CpuBench(0)
        f.sizes, f.fills = dict(bt.sizes), list(bt.fills)
        f.realise().run(b.ops)
        for label, buf in b.compare + ([('du', b.h['du'])] if 'du' in b.h else []):
            assert torch.equal(_view(f.cpu, buf).double(), _view(A, buf).double()), '%s: fp32 and bf16 storage differ' % label
