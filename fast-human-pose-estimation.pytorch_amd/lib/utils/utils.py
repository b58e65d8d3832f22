"""Optimizer factory and checkpoint I/O with the reference's interface (/root/reference/lib/utils/utils.py:59-83,204-258)."""
import os

import torch

from ... import runtime as R


def fill_flat_args(a, st, lr_dev, step_dev):
    """What fpd_adam_t, fpd_adamw_t and fpd_sgd_t share, over the arenas of the device state `st`: the parameter and gradient
    arenas and their size, no bf16 copy, grad_scale 1 (in the fused step the loss kernel already folds 1 / world_size into the
    gradient) and the schedule through the device scalars lr_dev / step_dev."""
    a.n = st.table.sizes['param']
    a.param, a.grad = st.A.tensor('param').data_ptr(), st.A.tensor('grad').data_ptr()
    a.param_lp = None
    a.grad_scale = 1.0
    a.lr_dev, a.step_dev = lr_dev.data_ptr(), step_dev.data_ptr()
    return a


def fill_adam_args(a, st, m, v, lr, betas, eps, lr_dev, step_dev):
    """The Adam part of an fpd_adam_t or fpd_adamw_t on top of fill_flat_args: the moment arenas and the hyperparameters, the
    bias corrections left to the kernel (it forms them from step_dev)."""
    fill_flat_args(a, st, lr_dev, step_dev)
    a.m, a.v = m.data_ptr(), v.data_ptr()
    a.lr, a.beta1, a.beta2, a.eps = lr, betas[0], betas[1], eps
    a.bias_corr1 = a.bias_corr2 = 1.0
    return a


class _FlatOptimizer(torch.optim.Optimizer):
    """What FusedAdam, FusedAdamW and FusedSGD share: one param group over the model's flat arenas (FusedAdamW splits it in two
    under its exemption), the device lr / step scalars the kernels read, the per-parameter views of a flat state arena
    in the reference's shapes, and the seam to the fused step: plan_op() and plan_key()."""

    keyword = 'adam'                             # the FusedFPDStep argument that takes this optimizer

    def _check_covers(self, st, *arenas, bits=None):
        """plan_op(st) refuses a device state whose parameter arena this optimizer's own arenas (and mask bits) do not cover."""
        n = st.table.sizes['param']
        if (any(t is not None and t.numel() < n for t in arenas) or (bits is not None and 32 * bits.numel() < n)
                or self.model._flat['param'].data_ptr() != st.A.tensor('param').data_ptr()):
            raise R.FpdError('FusedFPDStep: %s= is the %s of another model than the student of this step '
                             '(its state arenas do not cover the %d elements of this parameter arena)'
                             % (self.keyword, type(self).__name__, n))

    def plan_key(self):
        """What core.function keys its step cache on: the hyperparameters that live in the op plan_op() records (lr and the
        step count travel through device scalars and are not among them)."""
        return ()

    def _init_flat(self, model, defaults):
        self.model = model.module if hasattr(model, 'module') else model
        super().__init__(list(self.model.parameters()), defaults)
        flat = self.model._flat['param']         # the flat fp32 arena every parameter is a view of (create the optimizer
        lr = defaults['lr']                      # AFTER .to(device), like any torch optimizer)
        self.lr_dev = torch.full((1,), lr, dtype=torch.float32, device=flat.device)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=flat.device)
        self._lr_host = lr
        return flat

    def sync_lr(self):
        """param_groups[0]['lr'] (what LR schedules write) -> the device scalar the optimizer kernel reads."""
        lr = float(self.param_groups[0]['lr'])
        if lr != self._lr_host:
            self.lr_dev.fill_(lr)
            self._lr_host = lr

    def zero_grad(self, set_to_none=True):
        st = self.model.device_state()
        st.A.tensor('grad').zero_()

    def _views(self, flat):
        """Per trainable tensor, the slice of a flat arena in the reference's shape (OIHW for conv weights)."""
        m = self.model
        out = []
        for key in m.table.trainable_keys():
            b = m.table[key]
            v = flat[b.off:b.off + b.numel].view(b.shape)
            out.append(v.permute(0, 3, 1, 2) if len(b.shape) == 4 else v)
        return out


class FusedAdam(_FlatOptimizer):
    """torch.optim.Adam(lr) semantics (utils.py:69-73: betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad) as ONE
    HIP launch over the model's flat parameter / gradient arenas instead of 752 per-tensor launches.  lr is read from
    param_groups[0]['lr'] at every step, so torch LR schedulers (MultiStepLR, tools/fpd_train.py:236-239) work."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        flat = self._init_flat(model, dict(lr=lr, betas=betas, eps=eps))
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)

    def adam_args(self, st=None):
        g = self.param_groups[0]
        return fill_adam_args(R.AdamT(), self.model.device_state() if st is None else st, self.m, self.v, g['lr'], g['betas'],
                              g['eps'], self.lr_dev, self.step_dev)

    def plan_op(self, st):
        """(op code, filled struct) of the update over the arenas of the device state `st`, for FusedFPDStep to record."""
        self._check_covers(st, self.m, self.v)
        return R.OP_ADAM, self.adam_args(st)

    @torch.no_grad()
    def step(self, closure=None):
        self.sync_lr()
        R.check(R.lib().fpd_adam(self.adam_args(), R.current_stream()), 'fpd_adam')

    # ---- checkpoint interop: the state dict has torch.optim.Adam's layout (per-parameter exp_avg / exp_avg_sq in the
    #      reference's OIHW shapes), so `checkpoint['optimizer']` written here loads into the reference's Adam and a
    #      reference checkpoint resumes here (tools/fpd_train.py:224-234, AUTO_RESUME) ----
    def state_dict(self):
        step = self.step_dev.to(torch.float32).reshape(())
        state = {}
        if int(self.step_dev.item()) > 0:
            for i, (m, v) in enumerate(zip(self._views(self.m), self._views(self.v))):
                state[i] = {'step': step.clone(), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
        g = {k: v for k, v in self.param_groups[0].items() if k != 'params'}
        g.setdefault('weight_decay', 0)
        g.setdefault('amsgrad', False)
        g['params'] = list(range(len(self.param_groups[0]['params'])))
        return {'state': state, 'param_groups': [g]}

    def load_state_dict(self, sd):
        if 'm' in sd and 'v' in sd:
            # the round-1 checkpoints held the two moment arenas as flat tensors in the parameter order of THAT round; the
            # table has been re-ordered since (backward-completion buckets), so copying them would hand every parameter
            # another parameter's moments.  Refuse instead of mis-assigning.
            raise ValueError('optimizer state in the retired flat {m, v, step} layout cannot be mapped onto the current '
                             'parameter order; resume from a torch.optim.Adam-style state_dict (state / param_groups)')
        st = sd.get('state', {})
        mv, vv = self._views(self.m), self._views(self.v)
        if len(st) not in (0, len(mv)):
            raise ValueError('optimizer state has %d parameter entries, the model has %d' % (len(st), len(mv)))
        self.m.zero_(); self.v.zero_(); self.step_dev.zero_()
        ids = sd['param_groups'][0]['params']
        for dst_m, dst_v, pid in zip(mv, vv, ids):
            e = st.get(pid)
            if e is None:
                continue
            dst_m.copy_(e['exp_avg']); dst_v.copy_(e['exp_avg_sq'])
            self.step_dev.fill_(int(float(e['step'])))
        g = sd['param_groups'][0]
        for k in ('lr', 'betas', 'eps', 'initial_lr'):   # initial_lr: what torch's LR schedulers resume from
            if k in g:
                self.param_groups[0][k] = tuple(g[k]) if k == 'betas' else g[k]
        self.param_groups[0].setdefault('initial_lr', self.param_groups[0]['lr'])
        self._lr_host = None
        self.sync_lr()


def no_decay_mask(table):
    """The exemption of `no_decay_norm_bias` over a graph.ParamTable: every trainable tensor whose logical shape has fewer than
    2 dimensions (BN weight and bias, conv bias).  -> (ranges, words): the exempt [first, end) element ranges of the parameter
    arena in table order, and the numpy uint32 mask fpd_adamw_t.no_decay_bits takes -- bit i & 31 of word i >> 5 set = element
    i is exempt, ceil(n / 32) words.  The alignment gaps between tensors get no bit: their parameters and gradients are zero,
    which the decay leaves alone."""
    import numpy as np
    n = table.sizes['param']
    ranges = [(table[k].off, table[k].off + table[k].numel) for k in table.trainable_keys() if len(table[k].shape) < 2]
    bits = np.zeros((n + 31) // 32 * 32, dtype=np.uint8)
    for lo, hi in ranges:
        bits[lo:hi] = 1
    return ranges, np.packbits(bits, bitorder='little').view('<u4').astype(np.uint32)


class FusedAdamW(_FlatOptimizer):
    """torch.optim.AdamW(lr, betas, eps, weight_decay, amsgrad) semantics -- decoupled weight decay, optionally the AMSGrad
    maximum -- as ONE HIP launch (csrc/adamw.hip) over the model's flat parameter / gradient arenas.  no_decay_norm_bias: the
    tensors with fewer than 2 dimensions (BN weight and bias, conv bias) are exempt from the decay, through a bit mask the
    kernel reads (1/8 byte per element); they form a second param group with weight_decay 0, the way the recipes that exempt
    them hand two groups to torch.  weight_decay = 0 with amsgrad is torch.optim.Adam(amsgrad=True).  One lr serves both
    groups: param_groups[0]['lr'] is read at every step, like FusedAdam's.  The second moment maximum is allocated only under
    amsgrad.  Create it after .to(device), like any torch optimizer."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, no_decay_norm_bias=False):
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: %r' % (eps,))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError('Invalid beta parameter at index 0: %r' % (betas[0],))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError('Invalid beta parameter at index 1: %r' % (betas[1],))
        if not 0.0 <= weight_decay < float('inf'):
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        self.amsgrad, self.no_decay_norm_bias = bool(amsgrad), bool(no_decay_norm_bias)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=self.amsgrad, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None)
        m = model.module if hasattr(model, 'module') else model
        table = m.table
        exempt = [self.no_decay_norm_bias and len(table[k].shape) < 2 for k in table.trainable_keys()]
        # position in the state dict -> index of the trainable tensor: torch numbers the parameters group by group
        self._order = [i for i, e in enumerate(exempt) if not e] + [i for i, e in enumerate(exempt) if e]
        self._group_sizes = [len(exempt) - sum(exempt)] + ([sum(exempt)] if self.no_decay_norm_bias else [])
        flat = self._init_flat(model, defaults)
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        self.vmax = torch.zeros_like(flat) if self.amsgrad else None
        self.no_decay_ranges, self.mask = [], None
        if self.no_decay_norm_bias:
            self.no_decay_ranges, words = no_decay_mask(table)
            self.mask = torch.from_numpy(words.view('int32').copy()).to(flat.device)

    def _init_flat(self, model, defaults):
        flat = super()._init_flat(model, defaults)
        if self.no_decay_norm_bias:              # re-group: the decayed tensors first, then the exempt ones at weight_decay 0
            params = self.param_groups[0]['params']
            if len(params) != len(self._order):
                raise R.FpdError('FusedAdamW: the model has %d parameters, its table %d trainable tensors' % (len(params), len(self._order)))
            k = self._group_sizes[0]
            g1 = {key: v for key, v in self.param_groups[0].items() if key != 'params'}
            g1.update(weight_decay=0.0, params=[params[i] for i in self._order[k:]])
            self.param_groups[0]['params'] = [params[i] for i in self._order[:k]]
            self.param_groups.append(g1)
        return flat

    def sync_lr(self):
        for g in self.param_groups[1:]:          # one lr: the schedule writes group 0, the state dict shows it in both
            g['lr'] = self.param_groups[0]['lr']
            if 'initial_lr' in self.param_groups[0]:
                g['initial_lr'] = self.param_groups[0]['initial_lr']
        super().sync_lr()

    def adamw_args(self, st=None):
        """The filled fpd_adamw_t over the arenas of the model's device state: hyperparameters of group 0 as they are now, the
        schedule through lr_dev / step_dev."""
        g = self.param_groups[0]
        a = fill_adam_args(R.AdamWT(), self.model.device_state() if st is None else st, self.m, self.v, g['lr'], g['betas'],
                           g['eps'], self.lr_dev, self.step_dev)
        a.weight_decay = g['weight_decay']
        a.vmax = self.vmax.data_ptr() if self.vmax is not None else None
        a.no_decay_bits = self.mask.data_ptr() if self.mask is not None else None
        return a

    def plan_op(self, st):
        self._check_covers(st, self.m, self.v, self.vmax, bits=self.mask)
        return R.OP_ADAMW, self.adamw_args(st)

    def plan_key(self):
        g = self.param_groups[0]
        return (('adamw', float(g['weight_decay']), bool(self.amsgrad), bool(self.no_decay_norm_bias)),
                ('betas', float(g['betas'][0]), float(g['betas'][1]), float(g['eps'])))

    @torch.no_grad()
    def step(self, closure=None):
        if not self.m.is_cuda:
            raise R.FpdError('FusedAdamW.step needs the model on a CUDA (ROCm) device; there is no CPU path')
        self.sync_lr()
        R.check(R.lib().fpd_adamw(self.adamw_args(), R.current_stream()), 'fpd_adamw')

    # ---- checkpoint interop: torch.optim.AdamW's layout (per-parameter step / exp_avg / exp_avg_sq [/ max_exp_avg_sq] in the
    #      reference's OIHW shapes).  One param group, or with the exemption two -- decayed first, exempt at weight_decay 0,
    #      ids numbered group by group as torch numbers them -- so the dict loads into a stock AdamW built with the same
    #      groups, and back ----
    def _state_arenas(self):
        names = [('exp_avg', self.m), ('exp_avg_sq', self.v)]
        return names + ([('max_exp_avg_sq', self.vmax)] if self.amsgrad else [])

    def state_dict(self):
        self.sync_lr()
        step = self.step_dev.to(torch.float32).reshape(())
        state = {}
        if int(self.step_dev.item()) > 0:
            views = [(name, self._views(t)) for name, t in self._state_arenas()]
            for pos, i in enumerate(self._order):
                state[pos] = dict({'step': step.clone()}, **{name: v[i].clone() for name, v in views})
        groups, first = [], 0
        for g, k in zip(self.param_groups, self._group_sizes):
            d = {key: v for key, v in g.items() if key != 'params'}
            d['params'] = list(range(first, first + k))
            groups.append(d)
            first += k
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, sd):
        groups = sd['param_groups']
        if [len(g['params']) for g in groups] != self._group_sizes:
            raise ValueError('optimizer state partitions the parameters into groups of %r, this FusedAdamW (no_decay_norm_bias=%s) '
                             'into %r' % ([len(g['params']) for g in groups], self.no_decay_norm_bias, self._group_sizes))
        if any(bool(g.get('amsgrad', False)) != self.amsgrad for g in groups):
            raise ValueError('optimizer state has amsgrad=%r, this FusedAdamW amsgrad=%r' % (groups[0].get('amsgrad', False), self.amsgrad))
        if any(g.get('maximize', False) for g in groups):
            raise ValueError('FusedAdamW implements maximize False; the state has maximize True')
        if len(groups) == 2 and float(groups[1].get('weight_decay', 0)) != 0.0:
            raise ValueError('the exempt group of the optimizer state has weight_decay %r, not 0' % (groups[1]['weight_decay'],))
        if float(groups[0].get('weight_decay', 0)) < 0.0:
            raise ValueError('Invalid weight_decay value: %r' % (groups[0]['weight_decay'],))
        st = sd.get('state', {})
        ids = [pid for g in groups for pid in g['params']]
        if len(st) not in (0, len(ids)):
            raise ValueError('optimizer state has %d parameter entries, the model has %d' % (len(st), len(ids)))
        arenas = self._state_arenas()
        views = [(name, self._views(t)) for name, t in arenas]
        for pid, i in zip(ids, self._order):     # every entry is looked at before anything is written
            e = st.get(pid)
            for name, v in views:
                if e is not None and (name not in e or tuple(e[name].shape) != tuple(v[i].shape)):
                    raise ValueError('optimizer state entry %r: %s is missing or has another shape than the parameter' % (pid, name))
        for _, t in arenas:
            t.zero_()
        self.step_dev.zero_()
        for pid, i in zip(ids, self._order):
            e = st.get(pid)
            if e is None:
                continue
            for name, v in views:
                v[i].copy_(e[name])
            self.step_dev.fill_(int(float(e['step'])))
        for k in ('lr', 'betas', 'eps', 'weight_decay', 'initial_lr'):   # initial_lr: what torch's LR schedulers resume from
            if k in groups[0]:
                self.param_groups[0][k] = tuple(groups[0][k]) if k == 'betas' else groups[0][k]
        for g in self.param_groups[1:]:
            g.update({k: self.param_groups[0][k] for k in ('lr', 'betas', 'eps', 'initial_lr') if k in self.param_groups[0]})
        self.param_groups[0].setdefault('initial_lr', self.param_groups[0]['lr'])
        self._lr_host = None
        self.sync_lr()


class FusedSGD(_FlatOptimizer):
    """torch.optim.SGD(lr, momentum, dampening 0, weight_decay, nesterov) semantics (utils.py:61-67) as ONE HIP launch
    (csrc/loss_adam.hip sgd_kernel) over the flat parameter / gradient arenas.  The decay covers every parameter, BN
    gamma / beta included: the reference hands model.parameters() over as one group.  lr is read from
    param_groups[0]['lr'] at every step like FusedAdam's."""

    keyword = 'sgd'

    def __init__(self, model, lr=1e-3, momentum=0, weight_decay=0, nesterov=False):
        if lr < 0.0:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if momentum < 0.0:
            raise ValueError('Invalid momentum value: %r' % (momentum,))
        if weight_decay < 0.0:
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        if nesterov and momentum <= 0:
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        flat = self._init_flat(model, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay,
                                           nesterov=bool(nesterov), maximize=False, foreach=None, differentiable=False,
                                           fused=None))
        self.buf = torch.zeros_like(flat) if momentum != 0 else None
        self._resumed = False                    # a loaded state carries buffers but no step count

    def sgd_args(self, st=None):
        g = self.param_groups[0]
        a = fill_flat_args(R.SgdT(), self.model.device_state() if st is None else st, self.lr_dev, self.step_dev)
        a.buf = self.buf.data_ptr() if self.buf is not None else None
        a.lr, a.momentum, a.weight_decay, a.nesterov = g['lr'], g['momentum'], g['weight_decay'], int(g['nesterov'])
        return a

    def plan_op(self, st):
        self._check_covers(st, self.buf)
        return R.OP_SGD, self.sgd_args(st)

    def plan_key(self):
        g = self.param_groups[0]
        return (('sgd', float(g['momentum']), float(g['weight_decay']), bool(g['nesterov'])),)

    @torch.no_grad()
    def step(self, closure=None):
        self.sync_lr()
        R.check(R.lib().fpd_sgd(self.sgd_args(), R.current_stream()), 'fpd_sgd')

    # ---- checkpoint interop: torch.optim.SGD's layout (one momentum_buffer per parameter in the reference's OIHW shapes,
    #      no step count), so the reference's SGD loads what is written here and a reference checkpoint resumes here ----
    def state_dict(self):
        state = {}
        if self.buf is not None and (self._resumed or int(self.step_dev.item()) > 0):
            for i, b in enumerate(self._views(self.buf)):
                state[i] = {'momentum_buffer': b.clone()}
        g = {k: v for k, v in self.param_groups[0].items() if k != 'params'}
        g['params'] = list(range(len(self.param_groups[0]['params'])))
        return {'state': state, 'param_groups': [g]}

    def load_state_dict(self, sd):
        g = sd['param_groups'][0]
        if g.get('dampening', 0) != 0 or g.get('maximize', False):
            raise ValueError('FusedSGD implements dampening 0 and maximize False; the state has dampening %r, maximize %r'
                             % (g.get('dampening', 0), g.get('maximize', False)))
        momentum, nesterov = g.get('momentum', self.param_groups[0]['momentum']), g.get('nesterov', self.param_groups[0]['nesterov'])
        if nesterov and momentum <= 0:
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        st = sd.get('state', {})
        n = len(self.param_groups[0]['params'])
        if len(st) not in (0, n):
            raise ValueError('optimizer state has %d parameter entries, the model has %d' % (len(st), n))
        if momentum != 0 and self.buf is None:
            self.buf = torch.zeros_like(self.model._flat['param'])
        self.step_dev.zero_()
        self._resumed = False
        if self.buf is not None:
            self.buf.zero_()
            for dst, pid in zip(self._views(self.buf), g['params']):
                b = (st.get(pid) or {}).get('momentum_buffer')
                if b is not None:                # None: what torch keeps before a parameter's first step = a zero buffer
                    dst.copy_(b)
                    self._resumed = True
        for k in ('lr', 'momentum', 'weight_decay', 'nesterov', 'initial_lr'):   # initial_lr: what torch's LR schedulers resume from
            if k in g:
                self.param_groups[0][k] = g[k]
        self.param_groups[0].setdefault('initial_lr', self.param_groups[0]['lr'])
        self._lr_host = None
        self.sync_lr()


class _EmaOutputs(torch.autograd.Function):
    """Identity on the averaged model's outputs whose backward is the refusal: nothing trains through an average."""

    @staticmethod
    def forward(ctx, anchor, *outs):
        return tuple(o.view_as(o) for o in outs)

    @staticmethod
    def backward(ctx, *g):
        raise R.FpdError('ModelEma.module holds averaged weights: it is evaluated, never trained (backward through it refused)')


class _EmaModule:
    """Mixed in front of the model's class for ModelEma.module: always in eval mode, no backward."""

    def train(self, mode=True):
        if mode:
            raise R.FpdError('ModelEma.module holds averaged weights and stays in eval mode (train() refused)')
        return super().train(False)

    def forward(self, x):
        outs = super().forward(x)
        if not torch.is_grad_enabled():
            return outs
        wrapped = _EmaOutputs.apply(next(self.parameters()), *(outs if isinstance(outs, list) else [outs]))
        return list(wrapped) if isinstance(outs, list) else wrapped[0]


class ModelEma:
    """Exponential moving average of a HIP-backed model's state (timm ModelEmaV3 / the ExpMomentumEMA hook of RTMPose):
    EMA copies of the model's three flat arenas and a device update counter, advanced by ONE fpd_ema launch (csrc/ema.hip) --
    by update() on the module-API path, or as a plan op inside the fused step's optimizer range (FusedFPDStep(ema=)).
    Parameters and BN running statistics are averaged, e += w (x - e) with w = 1 - min(decay, (1 + u) / (10 + u)) under
    warm-up (csrc/ema_math.h); num_batches_tracked is copied.  `.module` is a second instance of the model's class whose
    tensors are views of the EMA arenas: validate, tools/test.py and load_checkpoint take it like the model.  Create it after
    .to(device), like the optimizer."""

    def __init__(self, model, decay=0.9998, warmup=True):
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError('Invalid EMA decay: %r (expected 0 <= decay < 1)' % (decay,))
        self.model = model.module if hasattr(model, 'module') else model
        if not hasattr(self.model, '_flat') or not hasattr(self.model, 'clone_structure'):
            raise R.FpdError('ModelEma: %s is not a HIP-backed model (lib.models)' % type(self.model).__name__)
        self.decay, self.warmup = float(decay), bool(warmup)
        self.flat = {n: t.clone() for n, t in self.model._flat.items()}
        self.updates_dev = torch.zeros(1, dtype=torch.int64, device=self.flat['param'].device)
        cls = type(self.model)
        with torch.random.fork_rng(devices=[]):            # the second instance's own initialisation draws nothing from the run
            self.module = self.model.clone_structure(type('Ema' + cls.__name__, (_EmaModule, cls), {}))
        self.module._flat = self.flat
        self.module._flat_grad = self.module._state = None
        self.module._instances = {}
        self.module._relink()
        self.module.eval()

    def ema_args(self):
        """The filled fpd_ema_t: parameter arena, running-statistics arena, num_batches_tracked as the plain copy."""
        t, src = self.model.table, self.model._flat
        a = R.EmaT()
        a.nseg = 2
        for s, n in enumerate(('param', 'rstat')):
            a.seg[s].src, a.seg[s].dst, a.seg[s].n = src[n].data_ptr(), self.flat[n].data_ptr(), t.sizes[n]
        a.warmup, a.decay = int(self.warmup), self.decay
        a.copy_src, a.copy_dst, a.copy_n = src['nbt'].data_ptr(), self.flat['nbt'].data_ptr(), t.sizes['nbt']
        a.updates_dev = self.updates_dev.data_ptr()
        return a

    @torch.no_grad()
    def update(self):
        if not self.flat['param'].is_cuda:
            raise R.FpdError('ModelEma.update needs the model on a CUDA (ROCm) device; there is no CPU path')
        R.check(R.lib().fpd_ema(self.ema_args(), R.current_stream()), 'fpd_ema')

    @torch.no_grad()
    def set(self, model=None):
        """Start the average again from the model's current state: arenas copied, counter zero."""
        m = self.model if model is None else (model.module if hasattr(model, 'module') else model)
        for n in self.flat:
            self.flat[n].copy_(m._flat[n])
        self.updates_dev.zero_()

    @property
    def updates(self):
        return int(self.updates_dev.item())

    def state_dict(self):
        return {'state_dict': {k: v.clone() for k, v in self.module.state_dict().items()}, 'updates': self.updates,
                'decay': self.decay, 'warmup': self.warmup}

    def load_state_dict(self, sd):
        inner = {(k[7:] if k.startswith('module.') else k): v for k, v in sd['state_dict'].items()}
        self.module.load_state_dict(inner)
        self.updates_dev.fill_(int(sd.get('updates', 0)))
        if 'decay' in sd:
            if not 0.0 <= float(sd['decay']) < 1.0:
                raise ValueError('Invalid EMA decay in the state: %r' % (sd['decay'],))
            self.decay = float(sd['decay'])
        if 'warmup' in sd:
            self.warmup = bool(sd['warmup'])


class GradClipper:
    """torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) over the model's flat gradient arena as ONE fpd_grad_clip
    call (csrc/grad_clip.hip: float64 sum of squares, coefficient, in-place scale; three launches, no host wait) -- by
    clip() between loss.backward() and optimizer.step() on the module-API path, or as the first plan op of the fused step's
    optimizer range (FusedFPDStep(clip=)).  max_norm = inf measures the norm and scales nothing.  The clipper owns the
    scratch, the device pair (norm, coef) of the last call and three device counters (calls, clipped, non-finite norm).
    Create it after .to(device), like the optimizer."""

    def __init__(self, model, max_norm):
        max_norm = float(max_norm)
        if not max_norm > 0.0:                   # refuses a NaN too
            raise ValueError('Invalid max_norm: %r (expected > 0; inf measures without clipping)' % (max_norm,))
        self.model = model.module if hasattr(model, 'module') else model
        if not hasattr(self.model, '_flat') or not hasattr(self.model, 'table'):
            raise R.FpdError('GradClipper: %s is not a HIP-backed model (lib.models)' % type(self.model).__name__)
        self.max_norm = max_norm
        dev = self.model._flat['param'].device
        nbytes = R.lib().fpd_grad_clip_scratch_bytes(self.model.table.sizes['param'])
        if nbytes < 0:
            R.check(int(nbytes), 'fpd_grad_clip_scratch_bytes')
        self.partial = torch.zeros(nbytes // 8, dtype=torch.float64, device=dev)
        self.out = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)
        self.counters = torch.zeros(3, dtype=torch.int64, device=dev)

    def clip_args(self):
        """The filled fpd_grad_clip_t over the gradient arena of the model's device state."""
        st = self.model.device_state()
        a = R.GradClipT()
        a.n, a.grad, a.max_norm = st.table.sizes['param'], st.A.tensor('grad').data_ptr(), self.max_norm
        a.partial, a.partial_bytes = self.partial.data_ptr(), self.partial.numel() * 8
        a.out, a.counters = self.out.data_ptr(), self.counters.data_ptr()
        return a

    @torch.no_grad()
    def clip(self):
        """Clip now, on the current stream; returns the device tensor of the norm (no synchronisation)."""
        R.check(R.lib().fpd_grad_clip(self.clip_args(), R.current_stream()), 'fpd_grad_clip')
        return self.out[0]

    __call__ = clip

    def norm(self):
        """Gradient norm of the last call, before clipping -- synchronises."""
        return float(self.out[0].item())

    def coef(self):
        """The factor the last call scaled the gradient by (1: not clipped) -- synchronises."""
        return float(self.out[1].item())

    def stats(self):
        """{'calls', 'clipped', 'nonfinite'} since creation -- synchronises."""
        c = self.counters.tolist()
        return {'calls': c[0], 'clipped': c[1], 'nonfinite': c[2]}


def get_grad_clipper(cfg, model):
    """TRAIN.CLIP_GRAD_NORM -> a GradClipper of `model`: 0 (the default) = none, .inf = measure and log only."""
    v = cfg.TRAIN.CLIP_GRAD_NORM
    if isinstance(v, str) and v.lower() in ('.inf', '+.inf'):     # YAML's spelling, as a KEY VALUE pair of the command line
        v = 'inf'
    max_norm = float(v)
    if max_norm == 0.0:
        return None
    if not max_norm > 0.0:
        raise ValueError('TRAIN.CLIP_GRAD_NORM must be 0 (off), positive or .inf (measure only), got %r' % (cfg.TRAIN.CLIP_GRAD_NORM,))
    return GradClipper(model, max_norm)


def get_accum_steps(cfg):
    """TRAIN.ACCUM_STEPS -> the accum= of the fused step: batches per optimizer update, 1 (the default) = every batch."""
    v = cfg.TRAIN.ACCUM_STEPS
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError('TRAIN.ACCUM_STEPS must be an integer >= 1 (batches per optimizer update), got %r' % (v,))
    return v


def multistep_lr(base_lr, milestones, gamma, epoch):
    """Learning rate the reference trains epoch `epoch` with (tools/fpd_train.py:236-239,253: MultiStepLR built with
    last_epoch = -1 and stepped at the START of every epoch, so epoch e runs at the scheduler's value for e + 1, i.e.
    a milestone m takes effect in epoch m - 1).  Closed form, so a resumed run continues exactly where an
    uninterrupted one would be (torch's chainable scheduler form re-applies a milestone that falls on the resume epoch
    when it is handed an already-decayed lr; the reference under torch 1.0 additionally skips one epoch on resume --
    neither artefact is reproduced)."""
    return base_lr * gamma ** sum(1 for m in milestones if m <= epoch + 1)


def _cfg_flag(cfg, name):
    """TRAIN.<name> as a bool; a config object without the key (callers that build only the keys they read) means false."""
    try:
        v = getattr(cfg.TRAIN, name)
    except (AttributeError, KeyError):
        return False
    if isinstance(v, str) and v.lower() in ('true', 'false'):     # YAML's spelling, as a KEY VALUE pair of the command line
        v = v.lower() == 'true'
    if not isinstance(v, bool):
        raise ValueError('TRAIN.%s must be true or false, got %r' % (name, v))
    return v


def get_optimizer(cfg, model):
    """utils.py:59-75, plus what the reference does not offer: TRAIN.OPTIMIZER adamw (decoupled TRAIN.WD, TRAIN.AMSGRAD,
    TRAIN.NO_DECAY_NORM_BIAS), and adam with TRAIN.AMSGRAD = torch.optim.Adam(amsgrad=True).  Plain adam ignores TRAIN.WD, as the
    reference does."""
    amsgrad = _cfg_flag(cfg, 'AMSGRAD')
    if cfg.TRAIN.OPTIMIZER == 'adam':
        if amsgrad:
            return FusedAdamW(model, lr=cfg.TRAIN.LR, weight_decay=0, amsgrad=True)
        return FusedAdam(model, lr=cfg.TRAIN.LR)
    if cfg.TRAIN.OPTIMIZER == 'adamw':
        return FusedAdamW(model, lr=cfg.TRAIN.LR, weight_decay=cfg.TRAIN.WD, amsgrad=amsgrad,
                          no_decay_norm_bias=_cfg_flag(cfg, 'NO_DECAY_NORM_BIAS'))
    if cfg.TRAIN.OPTIMIZER == 'sgd':
        return FusedSGD(model, lr=cfg.TRAIN.LR, momentum=cfg.TRAIN.MOMENTUM, weight_decay=cfg.TRAIN.WD,
                        nesterov=cfg.TRAIN.NESTEROV)
    raise ValueError('unknown optimizer %r' % cfg.TRAIN.OPTIMIZER)


def get_model_summary(model, *input_tensors, item_length=26, verbose=False):
    """utils.py:86-202: per-layer table (name, input size, output size, parameters, multiply-adds) collected by forward
    hooks on every non-container module.  The reference obtains it from a CPU dry-run; the HIP-backed models execute as
    one fused plan, so the hooks are fired by `model.shape_forward(input_shape)` instead -- the same modules in the same
    order with shape-only (meta) tensors, which is everything the hooks read.  Same text as the reference's."""
    import os as _os
    import torch.nn as nn
    summary, hooks, instances = [], [], {}

    def hook(module, inp, output):
        cls = type(module).__name__
        instances[cls] = instances.get(cls, 0) + 1
        params = 0
        if 'Conv' in cls or 'BatchNorm' in cls or 'Linear' in cls:
            params = sum(p.numel() for p in module.parameters())
        flops = 'Not Available'
        if 'Conv' in cls and hasattr(module, 'weight'):
            flops = int(module.weight.numel())
            for d in list(output.size())[2:]:
                flops *= int(d)
        elif isinstance(module, nn.Linear):
            flops = int(output.numel()) * int(inp[0].size(1))
        out0 = output[0] if isinstance(output, list) else output
        summary.append(('%s_%d' % (cls, instances[cls]), list(inp[0].size()), list(out0.size()), params, flops))

    target = model.module if hasattr(model, 'module') and hasattr(model.module, 'shape_forward') else model
    def add_hooks(m):                       # utils.py:147-152 via nn.Module.apply: a module shared by several parents
        if not isinstance(m, (nn.ModuleList, nn.Sequential)) and m is not target:      # (the model's ReLU) is visited, and
            hooks.append(m.register_forward_hook(hook))                                # hooked, once per parent
    target.apply(add_hooks)
    target.eval()
    try:
        target.shape_forward(tuple(input_tensors[0].shape))
    finally:
        for h in hooks:
            h.remove()
    sp, nl = item_length, _os.linesep
    rule = '-' * sp * 5 + nl
    details = ''
    if verbose:
        heads = ('Name', 'Input Size', 'Output Size', 'Parameters', 'Multiply Adds (Flops)')
        details = 'Model Summary' + nl + ''.join(h + ' ' * (sp - len(h)) for h in heads) + nl + rule
    params_sum = flops_sum = 0
    for row in summary:
        params_sum += row[3]
        if row[4] != 'Not Available':
            flops_sum += row[4]
        if verbose:
            details += ''.join(str(c) + ' ' * (sp - len(str(c))) for c in row) + nl + rule
    details += nl + 'Total Parameters: {:,}'.format(params_sum) + nl + rule
    details += 'Total Multiply Adds (For Convolution and Linear Layers only): {:,} GFLOPs'.format(flops_sum / (1024 ** 3)) + nl + rule
    details += 'Number of Layers' + nl
    for cls in instances:
        details += '{} : {} layers   '.format(cls, instances[cls])
    return details


def save_checkpoint(states, is_best, output_dir, filename='checkpoint.pth'):
    """utils.py:78-83."""
    torch.save(states, os.path.join(output_dir, filename))
    if is_best and 'state_dict' in states:
        torch.save(states['best_state_dict'], os.path.join(output_dir, 'model_best.pth'))


def load_checkpoint(checkpoint, model, strict=True, model_info=''):
    """utils.py:204-258: accepts a raw state_dict, a DataParallel state_dict ('module.' prefix) or a wrapped dict."""
    sd = torch.load(checkpoint, map_location='cpu') if isinstance(checkpoint, str) else checkpoint
    for key in ('best_state_dict', 'state_dict'):
        if isinstance(sd, dict) and key in sd and isinstance(sd[key], dict):
            sd = sd[key]
            break
    sd = {(k[7:] if k.startswith('module.') else k): v for k, v in sd.items()}
    target = model.module if hasattr(model, 'module') else model
    return target.load_state_dict(sd, strict=strict)
