"""FusedAdamW / fpd_adamw, the parts that need no GPU: a HOST build of the kernel's arithmetic (csrc/adamw_math.h) against the
numpy restatement (tests/_adamw_ref.py) bit for bit and under the host sanitizers as a stand-alone program; the restatement
and its mutants against torch.optim.AdamW; the dyadic trajectory's precondition; the exemption mask; the state dict through
stock torch.optim.AdamW; get_optimizer's keys; the ABI surface, geometry query and refusals of fpd_adamw."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import _adamw_ref as W, _sgd_ref
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'fast-human-pose-estimation.pytorch_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'native', 'adamw_host.cpp')


def _cxx():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler for the host build of csrc/adamw_math.h')
    return cxx


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('adamw') / 'libadamw_host.so')
    subprocess.check_call([_cxx(), '-O2', '-ffp-contract=off', '-Wno-unknown-pragmas', '-shared', '-fPIC', '-I' + CSRC, SRC, '-o', so])
    lib = C.CDLL(so)
    lib.adamw_array_host.restype = None
    lib.adamw_array_host.argtypes = [C.c_void_p] * 6 + [C.c_int64] + [C.c_float] * 6 + [C.c_int64]
    lib.adamw_bias_host.restype = None
    lib.adamw_bias_host.argtypes = [C.c_float, C.c_float, C.c_int64, C.c_void_p]
    return lib


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(got, want):
    """Bit equality, a NaN matching any NaN."""
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan])


def _host_run(lib, p0, grads, lrs, betas, eps, wd, amsgrad, grad_scale=1.0, exempt=None):
    f = np.float32
    p = p0.numpy().astype(f).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    x = np.zeros_like(p) if amsgrad else None
    words = W.mask_words(exempt) if exempt is not None else None
    for t, (g, lr) in enumerate(zip(grads, lrs)):
        g = np.ascontiguousarray(g.numpy().astype(f))
        lib.adamw_array_host(p.ctypes.data, g.ctypes.data, m.ctypes.data, v.ctypes.data, x.ctypes.data if amsgrad else None,
                             words.ctypes.data if words is not None else None, p.size, lr, betas[0], betas[1], eps, wd, grad_scale, t)
    t = torch.from_numpy
    return dict(p=t(p), m=t(m), v=t(v), vmax=t(x) if amsgrad else None)


# ---- the host build of csrc/adamw_math.h ----

@pytest.mark.parametrize('amsgrad', [False, True])
@pytest.mark.parametrize('wd', [0.0, 0.25])
def test_host_build_is_the_restatement_bit_for_bit(host_lib, wd, amsgrad):
    n = 4099
    exempt = W.exempt_of(n, W.mask_ranges(n))
    for regime in W.ALL_REGIMES:
        for kind in W.STARTS:
            p0, grads = W.start(kind, n), W.gradients(regime, n)
            for ex, gs in ((None, 1.0), (exempt, 0.5)):
                got = _host_run(host_lib, p0, grads, W.LRS, W.BETAS, W.EPS, wd, amsgrad, gs, ex)
                want = W.restated(p0, grads, W.LRS, W.BETAS, W.EPS, wd, amsgrad, gs, ex)
                for k in ('p', 'm', 'v') + (('vmax',) if amsgrad else ()):
                    assert _same_bits(got[k], want[k]), (regime, kind, ex is not None, k)
    # the bias corrections the kernel forms on the device schedule are those of tests/_adam_ref.bias_corrections
    out = np.zeros(2, np.float32)
    for t in (1, 2, 3, 1000, 100000):
        host_lib.adamw_bias_host(W.BETAS[0], W.BETAS[1], t - 1, out.ctypes.data)
        assert tuple(out) == W.bias_corrections(t)


def test_host_build_masked_elements_skip_the_decay_and_nothing_else(host_lib):
    n = 4099
    exempt = W.exempt_of(n, W.mask_ranges(n))
    p0, grads = W.start('randn', n), W.gradients('small', n)
    run = lambda wd, ex: _host_run(host_lib, p0, grads, W.LRS, W.BETAS, W.EPS, wd, True, 1.0, ex)
    masked, full, none = run(0.25, exempt), run(0.25, None), run(0.0, None)
    ex = torch.from_numpy(exempt)
    assert torch.equal(_bits(masked['p'])[ex], _bits(none['p'])[ex]) and torch.equal(_bits(masked['p'])[~ex], _bits(full['p'])[~ex])
    assert not torch.equal(masked['p'][ex], full['p'][ex])
    for k in ('m', 'v', 'vmax'):                                 # the decay is decoupled: the moments never see it
        assert torch.equal(_bits(masked[k]), _bits(full[k])) and torch.equal(_bits(full[k]), _bits(none[k]))
    # a NaN second moment wins the maximum, as in torch.maximum
    g = [torch.tensor([1.0, float('nan'), 1.0])] * 2
    r, w = _host_run(host_lib, torch.zeros(3), g, (0.1, 0.1), W.BETAS, W.EPS, 0.0, True), W.restated(torch.zeros(3), g, (0.1, 0.1), W.BETAS, W.EPS, 0.0, True)
    assert torch.isnan(r['vmax'][1]) and not torch.isnan(r['vmax'][0]) and _same_bits(r['vmax'], w['vmax']) and _same_bits(r['p'], w['p'])


def test_the_header_walks_its_cases_clean_under_the_host_sanitizers(tmp_path):
    """The same text with a small main, built with -fsanitize=address,undefined and run as a program of its own."""
    exe = str(tmp_path / 'adamw_san')
    subprocess.check_call([_cxx(), '-O1', '-g', '-ffp-contract=off', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DADAMW_MAIN', '-I' + CSRC, SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b'cases ok' in r.stdout, r.stdout.decode()


# ---- the restatement and its mutants against torch.optim.AdamW ----

N = 100003
B32 = tuple(float(np.float32(b)) for b in W.BETAS)


@functools.lru_cache(maxsize=None)
def _torch_pair(regime, kind, wd, amsgrad, betas=W.BETAS):
    p0, grads = W.start(kind, N), W.gradients(regime, N)
    return tuple(W.adamw_trajectory(p0, grads, W.LRS, betas, W.EPS, wd, amsgrad, dt) for dt in (torch.float32, torch.float64))


@pytest.mark.parametrize('amsgrad', [False, True])
@pytest.mark.parametrize('wd', W.WDS)
@pytest.mark.parametrize('regime', W.ALL_REGIMES)
def test_restatement_is_as_close_to_fp64_torch_as_fp32_torch_is_and_the_mutants_are_not(regime, wd, amsgrad):
    for kind in W.STARTS:
        p0, grads = W.start(kind, N), W.gradients(regime, N)
        r32, r64 = _torch_pair(regime, kind, wd, amsgrad)
        ours = W.restated(p0, grads, W.LRS, W.BETAS, W.EPS, wd, amsgrad)
        rp = _sgd_ref.assert_as_close_as_fp32(ours['p'], r32[0], r64[0], 'parameters, %s start, %s gradients' % (kind, regime))
        q32, q64 = _torch_pair(regime, kind, wd, amsgrad, B32)                   # m, v, vmax: at the betas the struct carries
        rs = [_sgd_ref.assert_as_close_as_fp32(ours[k], q32[i], q64[i], '%s, %s start, %s gradients' % (k, kind, regime))
              for k, i in (('m', 1), ('v', 2)) + ((('vmax', 3),) if amsgrad else ())]
        mut = {}
        for name in ('l2', 'no_decay') + (('no_max',) if amsgrad else ()):
            mut[name] = W.ratio(W.restated(p0, grads, W.LRS, W.BETAS, W.EPS, wd, amsgrad, mutant=name)['p'], r32[0], r64[0])
        print('adamw restated, %s start, %s gradients, wd %g, amsgrad %s: parameters %.3f, moments %s, mutants %s' % (
            kind, regime, wd, amsgrad, rp, ['%.3f' % r for r in rs], {k: '%.1f' % v for k, v in mut.items()}))
        assert mut['l2'] > 2 and mut['no_decay'] > 2, mut         # from both starts: after step 1 a zero start decays too
        if amsgrad and kind == 'zero':      # from randn the parameter's own rounding hides the missing maximum (ratio 1.0-1.2)
            assert mut['no_max'] > 2, mut


def test_dyadic_trajectory_is_exact_in_float32_and_float64_torch():
    """The precondition of the GPU test: float32 and float64 torch agree bit for bit, and so does the restatement."""
    p0, grads = W.dyadic_inputs(4099)
    for amsgrad in (False, True):
        r32, r64 = W.dyadic_trajectory(p0, grads, amsgrad), W.dyadic_trajectory(p0, grads, amsgrad, torch.float64)
        ours = W.restated(p0, grads, W.DYADIC_LRS, (0.0, 0.0), 0.0, W.DYADIC_WD, amsgrad)
        for i, k in enumerate(('p', 'm', 'v') + (('vmax',) if amsgrad else ())):
            assert torch.equal(r32[i].double(), r64[i]) and torch.equal(_bits(ours[k]), _bits(r32[i])), (amsgrad, k)
    plain, ams = W.dyadic_trajectory(p0, grads, False), W.dyadic_trajectory(p0, grads, True)
    assert not torch.equal(plain[0], ams[0]) and not torch.equal(ams[2], ams[3])     # the maximum does something on these inputs
    assert not torch.equal(plain[0], W.adamw_trajectory(p0, grads, W.DYADIC_LRS, (0.0, 0.0), 0.0, 0.0)[0])      # ... and so does the decay


# ---- the exemption mask, the state dict, get_optimizer: a tiny model on the CPU ----

class AD(dict):
    __getattr__ = dict.__getitem__


def _model():
    from fpd_amd.lib.models import hourglass
    torch.manual_seed(0)
    return hourglass.get_pose_net(AD(MODEL=AD(NUM_JOINTS=3, DTYPE='fp32', EXTRA=AD(NUM_FEATURES=16, NUM_STACKS=2, NUM_BLOCKS=1))), is_train=True)


@pytest.fixture(scope='module')
def runtime():
    from fpd_amd import runtime as R
    if not os.path.exists(R.LIB_PATH):
        subprocess.check_call(['bash', os.path.join(os.path.dirname(R.LIB_PATH), 'build.sh')])
    R.lib()
    return R


def test_mask_is_exactly_the_tensors_with_fewer_than_two_dimensions(runtime):
    from fpd_amd.lib.utils.utils import FusedAdamW, no_decay_mask
    model = _model()
    t = model.table
    ranges, words = no_decay_mask(t)
    want = [(t[k].off, t[k].off + t[k].numel) for k in t.trainable_keys() if len(t[k].shape) < 2]
    assert ranges == want and 0 < len(ranges) < len(t.trainable_keys())
    named = dict(model.named_parameters())
    assert sorted(k for k in t.trainable_keys() if len(t[k].shape) < 2) == sorted(k for k, p in named.items() if p.dim() < 2)
    n = t.sizes['param']
    assert words.dtype == np.uint32 and words.size == (n + 31) // 32
    assert np.array_equal(words, W.mask_words(W.exempt_of(n, ranges)))          # a direct loop over the elements
    covered = W.exempt_of(n, ranges).sum() + sum(t[k].numel for k in t.trainable_keys() if len(t[k].shape) >= 2)
    assert covered <= n                                                         # alignment gaps carry no bit
    opt = FusedAdamW(model, no_decay_norm_bias=True, amsgrad=True)
    assert np.array_equal(opt.mask.numpy().view(np.uint32), words) and opt.no_decay_ranges == ranges and opt.vmax is not None
    assert [len(g['params']) for g in opt.param_groups] == [len(named) - len(ranges), len(ranges)]
    assert all(p.dim() >= 2 for p in opt.param_groups[0]['params']) and all(p.dim() < 2 for p in opt.param_groups[1]['params'])
    assert opt.param_groups[0]['weight_decay'] == 1e-2 and opt.param_groups[1]['weight_decay'] == 0
    plain = FusedAdamW(model)
    assert plain.mask is None and plain.vmax is None and len(plain.param_groups) == 1
    with pytest.raises(runtime.FpdError, match='CUDA'):
        plain.step()


def _stock(model, opt):
    """A stock torch.optim.AdamW over stand-ins of the model's parameters, grouped as `opt` groups them."""
    groups = [dict(params=[torch.nn.Parameter(torch.zeros(p.shape)) for p in g['params']], weight_decay=g['weight_decay']) for g in opt.param_groups]
    return torch.optim.AdamW(groups, lr=opt.param_groups[0]['lr'], amsgrad=opt.amsgrad)


@pytest.mark.parametrize('exempt', [False, True])
@pytest.mark.parametrize('amsgrad', [False, True])
def test_state_dict_round_trips_through_stock_adamw(runtime, amsgrad, exempt):
    from fpd_amd.lib.utils.utils import FusedAdamW
    model = _model()
    kw = dict(lr=3e-4, weight_decay=0.05, amsgrad=amsgrad, no_decay_norm_bias=exempt)
    opt = FusedAdamW(model, **kw)
    assert opt.state_dict()['state'] == {}                                      # before the first step: no entries, like torch
    gen = torch.Generator().manual_seed(5)
    live = torch.zeros_like(opt.m, dtype=torch.bool)
    for k in model.table.trainable_keys():
        b = model.table[k]
        live[b.off:b.off + b.numel] = True
    for t in (opt.m, opt.v) + ((opt.vmax,) if amsgrad else ()):
        t.copy_(torch.rand(t.shape, generator=gen) * live)
    opt.step_dev.fill_(7)
    opt.param_groups[0]['lr'] = 1e-4                                            # a schedule wrote group 0: both groups show it
    sd = opt.state_dict()
    params = list(model.parameters())
    assert len(sd['param_groups']) == (2 if exempt else 1) and sorted(sd['state']) == list(range(len(params)))
    ids = [i for g in sd['param_groups'] for i in g['params']]
    assert ids == list(range(len(params))) and all(g['lr'] == 1e-4 and g['amsgrad'] == amsgrad for g in sd['param_groups'])
    ordered = [p for g in opt.param_groups for p in g['params']]
    for i, p in enumerate(ordered):
        e = sd['state'][i]
        assert set(e) == {'step', 'exp_avg', 'exp_avg_sq'} | ({'max_exp_avg_sq'} if amsgrad else set())
        assert float(e['step']) == 7 and all(e[k].shape == p.shape for k in e if k != 'step')
    if exempt:
        k = len(sd['param_groups'][0]['params'])
        assert all(p.dim() >= 2 for p in ordered[:k]) and all(p.dim() < 2 for p in ordered[k:])
        assert sd['param_groups'][0]['weight_decay'] == 0.05 and sd['param_groups'][1]['weight_decay'] == 0
    stock = _stock(model, opt)
    stock.load_state_dict(sd)
    for i, p in enumerate(p for g in stock.param_groups for p in g['params']):  # what torch now holds per parameter
        assert torch.equal(stock.state[p]['exp_avg'], sd['state'][i]['exp_avg'])
    back = FusedAdamW(model, **kw)
    back.load_state_dict(stock.state_dict())
    assert torch.equal(back.m, opt.m) and torch.equal(back.v, opt.v) and int(back.step_dev) == 7
    assert not amsgrad or torch.equal(back.vmax, opt.vmax)
    assert back.param_groups[0]['lr'] == 1e-4 and float(back.lr_dev) == np.float32(1e-4) and back.param_groups[0]['weight_decay'] == 0.05
    # refusals: another partition, another amsgrad, a decaying exempt group
    other = FusedAdamW(model, **dict(kw, no_decay_norm_bias=not exempt))
    with pytest.raises(ValueError, match='partitions'):
        other.load_state_dict(sd)
    with pytest.raises(ValueError, match='amsgrad'):
        FusedAdamW(model, **dict(kw, amsgrad=not amsgrad)).load_state_dict(sd)
    assert not other.m.any() and int(other.step_dev) == 0                       # a refused state writes nothing
    if exempt:
        bad = {'state': sd['state'], 'param_groups': [dict(g) for g in sd['param_groups']]}
        bad['param_groups'][1]['weight_decay'] = 0.05
        with pytest.raises(ValueError, match='exempt group'):
            back.load_state_dict(bad)


def test_constructor_checks_are_torchs(runtime):
    from fpd_amd.lib.utils.utils import FusedAdamW
    model = _model()
    for kw, word in ((dict(lr=-1.0), 'learning rate'), (dict(eps=-1e-8), 'epsilon'), (dict(betas=(1.0, 0.999)), 'index 0'),
                     (dict(betas=(0.9, -0.1)), 'index 1'), (dict(weight_decay=-0.01), 'weight_decay'), (dict(weight_decay=float('inf')), 'weight_decay')):
        with pytest.raises(ValueError, match=word):
            FusedAdamW(model, **kw)
        if 'inf' not in repr(kw):
            with pytest.raises(ValueError, match=word):
                torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], **kw)


def test_get_optimizer_keys(runtime):
    from fpd_amd.lib.config import _defaults
    from fpd_amd.lib.utils.utils import FusedAdam, FusedAdamW, get_optimizer
    model = _model()
    cfg = _defaults()
    assert cfg.TRAIN.AMSGRAD is False and cfg.TRAIN.NO_DECAY_NORM_BIAS is False
    assert type(get_optimizer(cfg, model)) is FusedAdam                          # adam without AMSGRAD: untouched
    cfg.merge_from_list(['TRAIN.AMSGRAD', 'true'])
    o = get_optimizer(cfg, model)
    assert type(o) is FusedAdamW and o.amsgrad and o.param_groups[0]['weight_decay'] == 0 and o.mask is None and o.param_groups[0]['lr'] == cfg.TRAIN.LR
    cfg.merge_from_list(['TRAIN.OPTIMIZER', 'adamw', 'TRAIN.WD', '0.05', 'TRAIN.LR', '0.001'])
    o = get_optimizer(cfg, model)
    assert type(o) is FusedAdamW and o.amsgrad and o.mask is None and len(o.param_groups) == 1
    assert (o.param_groups[0]['weight_decay'], o.param_groups[0]['lr'], o.param_groups[0]['betas'], o.param_groups[0]['eps']) == (0.05, 0.001, (0.9, 0.999), 1e-8)
    cfg.merge_from_list(['TRAIN.AMSGRAD', 'false', 'TRAIN.NO_DECAY_NORM_BIAS', 'true'])
    o = get_optimizer(cfg, model)
    assert not o.amsgrad and o.vmax is None and o.mask is not None and len(o.param_groups) == 2
    cfg.merge_from_list(['TRAIN.OPTIMIZER', 'lion'])
    with pytest.raises(ValueError, match='unknown optimizer'):
        get_optimizer(cfg, model)
    shipped = _defaults()
    shipped.merge_from_file(os.path.join(ROOT, 'experiments', 'fpd_synthetic', 'hg4x128_student_adamw.yaml'))
    assert shipped.TRAIN.OPTIMIZER == 'adamw' and shipped.TRAIN.NO_DECAY_NORM_BIAS is True and shipped.TRAIN.WD > 0
    assert isinstance(get_optimizer(shipped, model), FusedAdamW)
    plain = _defaults()
    plain.merge_from_file(os.path.join(ROOT, 'experiments', 'fpd_synthetic', 'hg4x128_student.yaml'))
    assert plain.TRAIN.OPTIMIZER == 'adam' and plain.TRAIN.AMSGRAD is False and type(get_optimizer(plain, model)) is FusedAdam


def test_fused_step_key_and_the_optimizer_check_know_adamw(runtime):
    from fpd_amd.lib.core import function as F
    from fpd_amd.lib.core.loss import JointsMSELoss
    model = _model()
    from fpd_amd.lib.utils.utils import FusedAdamW
    crit = JointsMSELoss(True)
    assert F._check_supported(FusedAdamW(model), crit, crit) == ((True, True), None)
    with pytest.raises(runtime.FpdError, match='AdamW'):
        F._check_supported(torch.optim.AdamW(model.parameters()), crit, crit)
    # what each optimizer adds to the step-cache key: the tuples fused_step_for used to assemble per class
    from fpd_amd.lib.utils.utils import FusedAdam, FusedSGD
    assert FusedAdam(model, lr=1e-3, betas=(0.8, 0.9), eps=1e-6).plan_key() == ()
    assert FusedSGD(model, lr=0.1, momentum=0.5, weight_decay=1e-4, nesterov=True).plan_key() == (('sgd', 0.5, 1e-4, True),)
    w = FusedAdamW(model, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.05, amsgrad=True, no_decay_norm_bias=True)
    assert w.plan_key() == (('adamw', 0.05, True, True), ('betas', 0.8, 0.9, 1e-6))
    assert all(type(x) is float for x in w.plan_key()[0][1:2] + w.plan_key()[1][1:]) and (FusedAdam.keyword, FusedAdamW.keyword, FusedSGD.keyword) == ('adam', 'adam', 'sgd')


# ---- the C ABI ----

# never dereferenced: every call is a query or refused; 1 GiB apart, so that the largest n of the geometry test fits
P, GRAD, M, V, VMAX, LP, MASK, LR, STEP = (k << 30 for k in range(1, 10))


def _args(R, n=4099, off=0, vmax=True, lp=True, mask=True):
    a = R.AdamWT()
    a.n = n
    a.param, a.grad, a.m, a.v = P + 4 * off, GRAD + 4 * off, M + 4 * off, V + 4 * off
    a.vmax, a.param_lp, a.no_decay_bits = (VMAX + 4 * off if vmax else None), (LP + 2 * off if lp else None), (MASK if mask else None)
    a.lr, a.beta1, a.beta2, a.eps, a.bias_corr1, a.bias_corr2, a.grad_scale, a.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, 1.0, 0.01
    a.lr_dev, a.step_dev = LR, STEP
    return a


def test_abi_has_fpd_adamw_with_the_mirrors_size_and_the_plan_takes_the_op(runtime):
    R, lib = runtime, runtime.lib()
    assert lib.fpd_abi_sizeof(b'fpd_adamw_t') == C.sizeof(R.AdamWT) == 120
    assert lib.fpd_abi_sizeof(b'fpd_adam_t') == C.sizeof(R.AdamT) == 96            # additions only: fpd_adam_t did not grow
    assert lib.fpd_abi_version() == R.ABI_VERSION == 2 and R.OP_ADAMW == 31 and R.OP_GRAD_ACCUM == 30 and R.OP_ADAM == 6
    hdr = open(os.path.join(ROOT, 'include', 'fpd_amd.h')).read()
    assert 'FPD_OP_ADAMW = 31' in hdr and '} fpd_adamw_t;' in hdr and '#define FPD_ABI_VERSION 2' in hdr
    assert 'int fpd_adamw(const fpd_adamw_t*' in hdr
    p = lib.fpd_plan_create()
    assert lib.fpd_plan_add(p, R.OP_ADAMW, C.byref(_args(R)), C.sizeof(R.AdamWT)) == 0
    assert lib.fpd_plan_add(p, R.OP_ADAMW, C.byref(_args(R)), C.sizeof(R.AdamT)) < 0
    assert lib.fpd_plan_size(p) == 1
    lib.fpd_plan_destroy(p)


CAP = 4 * 256 * 4096


def test_geometry_query_over_alignment_and_the_cap(runtime):
    R, lib = runtime, runtime.lib()
    blocks, vec = C.c_int32(-1), C.c_int64(-1)

    def geo(a):
        assert lib.fpd_adamw_geometry(a, blocks, vec) == 0, lib.fpd_last_error()
        return blocks.value, vec.value
    assert geo(_args(R, 0)) == (1, 0) and geo(_args(R, 1)) == (1, 0) and geo(_args(R, 4099)) == (4, 4096)
    assert geo(_args(R, CAP + 4099)) == (4096, CAP + 4096) and geo(_args(R, 3287936)) == (3211, 3287936)
    assert geo(_args(R, 4099, off=1)) == (17, 0) and geo(_args(R, 4099, off=2)) == (17, 0)
    a = _args(R, 4099)
    a.vmax = VMAX + 4                                            # any one arena off the 16-byte grid: element by element
    assert geo(a) == (17, 0)
    a = _args(R, 4099)
    a.param_lp = LP + 4                                          # the bf16 copy needs 8 bytes for a vector of four
    assert geo(a) == (17, 0)
    assert geo(_args(R, 4099, vmax=False, lp=False, mask=False)) == (4, 4096)


def test_fpd_adamw_refuses_bad_arguments_without_a_device(runtime):
    R, lib = runtime, runtime.lib()
    blocks, vec = C.c_int32(), C.c_int64()
    assert lib.fpd_adamw(None, None) < 0 and b'null' in lib.fpd_last_error()
    cases = [('negative n', b'negative', dict(n=-1)), ('n too large', b'too large', dict(n=1 << 60)),
             ('null param', b'null', dict(param=None)), ('null grad', b'null', dict(grad=None)), ('null m', b'null', dict(m=None)),
             ('null v', b'null', dict(v=None)), ('negative decay', b'weight_decay', dict(weight_decay=-0.01)),
             ('infinite decay', b'weight_decay', dict(weight_decay=float('inf'))), ('nan decay', b'weight_decay', dict(weight_decay=float('nan'))),
             ('beta1 1', b'index 0', dict(beta1=1.0)), ('beta2 < 0', b'index 1', dict(beta2=-0.5)), ('eps < 0', b'epsilon', dict(eps=-1e-8)),
             ('eps nan', b'epsilon', dict(eps=float('nan'))), ('misaligned', b'misaligned', dict(m=M + 2)),
             ('m is param', b'overlaps', dict(m=P)), ('v inside m', b'overlaps', dict(v=M + 4 * 4098)), ('vmax is v', b'overlaps', dict(vmax=V)),
             ('grad is param', b'overlaps', dict(grad=P)), ('lp inside param', b'overlaps', dict(param_lp=P + 8)),
             ('mask inside v', b'overlaps', dict(no_decay_bits=V + 16)), ('counter inside m', b'overlaps', dict(step_dev=M + 8)),
             ('lr inside param', b'overlaps', dict(lr_dev=P + 4))]
    for label, word, kw in cases:
        a = _args(R)
        for k, v in kw.items():
            setattr(a, k, v)
        assert lib.fpd_adamw(a, None) < 0 and word in lib.fpd_last_error(), (label, lib.fpd_last_error())
        assert lib.fpd_adamw_geometry(a, blocks, vec) < 0 and word in lib.fpd_last_error(), label
    # what is NOT refused: a NULL vmax (no AMSGrad), no mask, no bf16 copy, the host schedule, adjacent arenas, weight_decay 0
    a = _args(R, vmax=False, lp=False, mask=False)
    a.lr_dev, a.step_dev, a.weight_decay = None, None, 0.0
    a.m, a.v = P + 4 * 4099 + 4, P + 8 * 4099 + 8
    assert lib.fpd_adamw_geometry(a, blocks, vec) == 0, lib.fpd_last_error()
