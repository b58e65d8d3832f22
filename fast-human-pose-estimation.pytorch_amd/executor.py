"""Device-side realisation of graph.py: arenas in HBM, lowering of the op list to the C ABI, native
execution plans (one C call or one hipGraph replay per phase), and the fused FPD train step.

PyTorch is used here only as the HBM allocator, stream provider and RCCL front end
(torch.distributed); every kernel that touches the data is in csrc/ (libfpd_amd.so).
"""
import ctypes as C
import os
from collections import namedtuple

import torch

from . import graph as G
from . import runtime as R
from .lib.utils.utils import fill_adam_args
from .schedule import PhaseSchedule

_EW = {'bnrelu_fwd': R.EW_BNRELU_FWD, 'bnrelu_bwd_r': R.EW_BNRELU_BWD_R, 'bn_bwd_apply': R.EW_BN_BWD_APPLY,
       'maxpool_fwd': R.EW_MAXPOOL_FWD, 'maxpool_bwd': R.EW_MAXPOOL_BWD, 'upadd_fwd': R.EW_UPADD_FWD,
       'sumpool': R.EW_SUMPOOL, 'add': R.EW_ADD, 'relu_mask': R.EW_RELU_MASK, 'dilate2': R.EW_DILATE2}
_ARENA_DTYPE = {'param': torch.float32, 'grad': torch.float32, 'rstat': torch.float32, 'nbt': torch.int64,
                'stats': torch.int64, 'losses': torch.float64, 'image': torch.float32, 'target': torch.float32,
                'weight': torch.float32, 'adam_m': torch.float32, 'adam_v': torch.float32, 'fold': torch.float32,
                'w8': torch.uint8, 'w8s': torch.float32, 'ohkm_scratch': torch.float64, 'ohkm_masks': torch.int32,
                'kl_scratch': torch.float64}


def act_torch_dtype(dtype):
    return torch.bfloat16 if dtype == R.BF16 else torch.float32


_STAT_HI, _STAT_LO = float(2 ** 20), float(2 ** 60)      # include/fpd_amd.h fpd_stat_t: value = hi * 2^-20 + lo * 2^-60


class Arenas:
    """name -> flat device tensor.  Lookups fall through to `parent` (model-level arenas).

    The 'stats' arena holds the exact statistics of include/fpd_amd.h (fpd_stat_t): the IR sizes a buffer over C channels
    as [R][2][C] logical values (what the CPU interpreter keeps as doubles); on the device every logical value is TWO
    64-bit integer limbs, laid out [R][2 sums][2 limbs][C], so the arena has two words per IR element."""

    def __init__(self, device, dtype, parent=None):
        self.device, self.dtype, self.parent = device, dtype, parent
        self.t = {}

    def alloc(self, name, n):
        dt = _ARENA_DTYPE.get(name, act_torch_dtype(self.dtype))
        n = max(int(n), 4) * (2 if name == 'stats' else 1)
        self.t[name] = torch.zeros(n, dtype=dt, device=self.device)
        return self.t[name]

    def stats_read(self, buf):
        """[R][2][C] float64: the value of every (replica, sum, channel) of a statistics buffer (a copy)."""
        raw = self.view(buf)
        return raw[:, :, 0, :].double() / _STAT_HI + raw[:, :, 1, :].double() / _STAT_LO

    def stats_write(self, buf, values):
        """Store [R][2][C] float64 values into a statistics buffer (the split a kernel's contribution goes through)."""
        v = values.to(self.device, torch.float64).reshape(buf.shape)
        hi = torch.round(v * _STAT_HI)
        lo = torch.round((v - hi / _STAT_HI) * _STAT_LO)
        self.view(buf).copy_(torch.stack([hi.to(torch.int64), lo.to(torch.int64)], 2))

    def tensor(self, name):
        if name in self.t:
            return self.t[name]
        if self.parent is not None:
            return self.parent.tensor(name)
        raise KeyError(name)

    def ptr(self, buf):
        if buf is None:
            return None
        t = self.tensor(buf.arena)
        return t.data_ptr() + buf.off * t.element_size() * (2 if buf.arena == 'stats' else 1)

    def view(self, buf):
        if buf.arena == 'stats':                   # raw limbs [R][2 sums][2 limbs][C]
            r, two, c = buf.shape
            return self.tensor('stats')[2 * buf.off:2 * (buf.off + buf.numel)].view(r, two, 2, c)
        return self.tensor(buf.arena)[buf.off:buf.off + buf.numel].view(buf.shape)


def _abuf(a):
    return None if a is None else (a.buf if isinstance(a, G.Act) else a)


def _nop():
    """What an op lowers to when it launches nothing (graph.Op.absorbed(), a fused weight gradient, a marker)."""
    return R.OP_NOP, R.MemsetT()


def _readers_of(readers, t, exclude=(), by_buf=True):
    """(position in `readers`, member op) of every launch member that lists tensor `t` among its acts_in(), the ops in
    `exclude` left out.  by_buf=True compares the planned Buf, which also catches a tensor aliased into another Act;
    by_buf=False compares the Act itself -- the only key there is before plan_memory, while every buf is still None."""
    key = _abuf if by_buf else (lambda a: a)
    y = key(t)
    for j, top in enumerate(readers):
        for o in (top.members() if top is not None else ()):
            if not any(o is e for e in exclude) and any(key(a) is y for a in o.acts_in()):
                yield j, o


# One weight gradient's slabs: `s` is the struct finish_partials patches (the very object the plan copies, for a pair a
# view INTO the pair struct), n slabs of `stride` floats from float `off` of the workspace, each dw (numel) + nbias bias sums.
Slabs = namedtuple('Slabs', 's dw numel stride n off dbias nbias')


# FPD_WHATIF=token[,token...]: TIMING-ONLY experiments (results are wrong when set): the named class of ops is lowered to
# no-ops, which shows what that class costs inside the pipelined step (experiments/r03/whatif.sh).  Student graph:
# nowgrad / nowgrad_small / nowgrad_big (weight gradients, by map height <= 16 / >= 64), noapply (BN-backward applies),
# nobigconv (convolutions on >= 64x64 maps), nobig / nomid / nosmall (every op on >= 64 / 32 / <= 16 high maps, weight
# gradients excepted), noew.  Teacher graph: t_all, t_big, t_mid, t_small; t_bneck_big / t_head / t_plain_big (the >= 64-high ops by kind).
_WHATIF = frozenset(t for t in os.environ.get('FPD_WHATIF', '').split(',') if t)
if _WHATIF:
    import sys
    sys.stderr.write('[fpd_amd] WARNING: FPD_WHATIF=%s is set: op classes are dropped from the plans -- TIMING ONLY, every result '
                     '(maps, losses, gradients, parameters) of this process is WRONG\n' % ','.join(sorted(_WHATIF)))


def _whatif_drop(op, train):
    k = op.kind
    if k in ('conv2', 'bneck2', 'ew2'):
        sub = op.a
        k = sub.kind
    else:
        sub = op
    dims = getattr(sub, 'dims', None)
    h = dims[1] if dims else 0
    if not train:
        if k not in ('conv', 'bneck', 'head', 'ew', 'stem_fwd'):
            return False
        # round 5: the teacher's >= 64-high ops by kind -- fused Bottlenecks (persistent, capped grid), fused heads, and the rest
        # (stem, layer1 / layer2 convolutions, max-pool: plain full-grid launches)
        if h >= 64 and (('t_bneck_big' in _WHATIF and k == 'bneck') or ('t_head' in _WHATIF and k == 'head') or
                        ('t_plain_big' in _WHATIF and k in ('conv', 'ew', 'stem_fwd'))):
            return True
        return ('t_all' in _WHATIF or ('t_big' in _WHATIF and h >= 64) or ('t_mid' in _WHATIF and h == 32) or
                ('t_small' in _WHATIF and h <= 16))
    if k in ('wgrad', 'stem_wgrad', 'wreduce'):
        return ('nowgrad' in _WHATIF or ('nowgrad_small' in _WHATIF and k == 'wgrad' and h <= 16) or
                ('nowgrad_big' in _WHATIF and k == 'wgrad' and h >= 64))
    if k not in ('conv', 'ew', 'stem_fwd'):
        return False
    if k == 'ew' and ('noew' in _WHATIF or ('noapply' in _WHATIF and sub.op == 'bn_bwd_apply')):
        return True
    if k == 'conv' and 'nobigconv' in _WHATIF and h >= 64:
        return True
    if k == 'conv' and h >= 32 and (('no3x3big' in _WHATIF and dims[5] == 3) or ('no1x1big' in _WHATIF and dims[5] == 1)):
        return True                                        # round 6: the >= 32-high convolutions by filter size
    return ('nobig' in _WHATIF and h >= 64) or ('nomid' in _WHATIF and h == 32) or ('nosmall' in _WHATIF and h <= 16)


class Lowering:
    """IR op -> (native op code, ctypes struct)."""

    def __init__(self, arenas, dtype):
        self.A, self.dtype = arenas, dtype
        self.keep = []          # device tables that must outlive the plan
        self.use_partials = False
        self.partials, self.partial_elems = {}, 0      # id(IR wgrad op) -> slab record
        self.fused = set()                             # id(IR wgrad op) computed inside its data-gradient launch (conv_pp)
        self.reduces = []                              # (IR wreduce op, its TableT) filled in by finish_partials()

    def bn(self, bn):
        s = R.BnT()
        if bn is None:
            s.mode = R.BN_NONE
            return s
        s.mode = R.BN_TRAIN if bn.mode == 'train' else R.BN_EVAL
        s.relu = 1 if bn.relu else 0
        s.eps = G.BN_EPS
        s.stats = self.A.ptr(bn.stats) if bn.mode == 'train' else None
        s.gamma, s.beta = self.A.ptr(bn.gamma), self.A.ptr(bn.beta)
        s.running_mean, s.running_var = self.A.ptr(bn.rmean), self.A.ptr(bn.rvar)
        return s

    def conv(self, op, plain=False):
        """plain=True: the convolution as the graph states it, every decision ignored (the planners and the pair launches start there)."""
        if not plain and op.absorbed():        # formed inside the launch of the conv3 it is the residual of (plan_skips)
            return _nop()
        s = R.ConvT()
        (s.N, s.H, s.W, s.C, s.K, s.R, s.S, s.stride, s.pad, s.P, s.Q) = op.dims
        s.dtype = self.dtype
        s.epi = R.EPI_BNRELU_BWD if op.epi == 'bnrelu_bwd' else R.EPI_PLAIN
        p = self.A.ptr
        s.x, s.w, s.bias, s.residual, s.y = p(_abuf(op.x)), p(op.w), p(op.bias), p(_abuf(op.residual)), p(_abuf(op.y))
        s.out_stats = p(op.out_stats)
        s.bn = self.bn(op.bn)
        s.epi_x, s.epi_bn, s.epi_stats = p(_abuf(op.epi_x)), self.bn(op.epi_bn), p(op.epi_stats)
        if plain:
            return R.OP_CONV, s
        if op.skip_active:
            self._fill_skip(op, s)
        if op.fused_wgrad is not None and self.use_partials:
            n = R.lib().fpd_conv_fused_wgrad_partials(C.byref(s))
            if n > 0:
                self._fuse_wgrad(op, s, n)
        self._fill_fold(op, s)
        if op.w8 is not None:
            f = R.ConvF8T()
            f.c, f.w8, f.w8_scale = s, p(op.w8), p(op.w8s)
            return R.OP_CONV_F8, f
        return R.OP_CONV, s

    def plan_folds(self, ops):
        """Decide, BEFORE the list is lowered, which BN-backward applies are evaluated by the data gradient that consumes
        them (graph: conv.fold_apply; include/fpd_amd.h: fpd_conv_t.fold_x): where the library serves the launch (pair)
        that way the apply is marked `folded` (lowered as a no-op) and the convolution `fold_active`."""
        if os.environ.get('FPD_FOLD_APPLY', '1') == '0':
            return
        l = R.lib()
        for i, op in enumerate(ops):
            if op is None or op.kind not in ('conv', 'conv2'):
                continue
            cands = [m for m in op.members() if m.fold_apply is not None and not m.fold_apply.folded]
            if not cands or any(m.w8 is not None for m in op.members()):
                continue
            # Who else reads an apply's result?  Its own convolution's weight gradient is served from the launch's operand image
            # when that is fused too; ANY other reader (a tensor aliased into a residual-path gradient, an op on another lane)
            # needs the evaluated operand in memory: the launch then writes it out (fold_out).  A reader that comes BEFORE the
            # convolution in the list would read it before it exists: no fold.
            early = False
            for m in cands:
                at = [j for j, _ in _readers_of(ops, m.fold_apply.y, exclude=(m, m.fold_apply, m.fold_wgrad))]
                m.fold_other_readers = bool(at)
                early = early or any(j < i for j in at)
            if early:
                continue
            if op.kind == 'conv2':
                ps = R.ConvPairT()
                ps.a, ps.b = self.conv(op.a, plain=True)[1], self.conv(op.b, plain=True)[1]
                ok = l.fpd_conv_pair_fold_supported(C.byref(ps)) == 1
            else:
                ok = l.fpd_conv_fold_supported(C.byref(self.conv(op, plain=True)[1])) == 1
            if ok:
                for m in cands:
                    m.fold_active = True
                    m.fold_apply.folded = True

    def plan_ew_merge(self, ops):
        """Decide, AFTER memory planning and before the backward list is lowered, which BN-backward applies that carry a residual
        `add` are evaluated inside the pool-backward op that reads them first (include/fpd_amd.h: fpd_ew_merge_t):
          pattern 1  an apply pair (or a lone half-resolution apply) directly in front of a 'maxpool_bwd' on lane 0 whose dy / add
                     / x are the pair's b.y / a.y / a.x, and nothing else reads a.y or b.y;
          pattern 2  an apply directly in front of the 'sumpool' whose x is its result.
        The absorbed ops are marked `ewm_absorbed` (lowered as no-ops); the pool op gets `ewm_kind` / `ewm_full` / `ewm_half`
        and is lowered, at its own position, as one FPD_OP_EW_MERGE.  The launch reads the applies' inputs (and, pattern 2, writes
        the apply's result) later than the memory plan assumed, so a group is taken only if, on PHYSICAL arena intervals, no
        output of the launch overlaps one of its inputs and no op between the absorbed op and the launch touches what moved."""
        if os.environ.get('FPD_EW_MERGE', '1') == '0':
            return
        l = R.lib()
        iv = lambda b: (b.arena, b.off, b.off + b.numel)
        hit = lambda p, q: p[0] == q[0] and p[1] < q[2] and q[1] < p[2]
        is_apply = lambda m: m.kind == 'ew' and m.op == 'bn_bwd_apply' and not m.folded and not m.ewm_absorbed
        lane0 = [i for i, op in enumerate(ops) if op is not None and (op.lane or 0) == 0]
        for k in range(1, len(lane0)):
            i, j = lane0[k - 1], lane0[k]
            prev, op = ops[i], ops[j]
            if op.kind != 'ew' or op.op not in ('maxpool_bwd', 'sumpool') or op.ewm_kind is not None:
                continue
            full = half = None
            if op.op == 'maxpool_bwd':
                cands = [m for m in prev.members() if is_apply(m)] if prev.kind in ('ew', 'ew2') else []
                if len(cands) != len(prev.members()):
                    continue
                half = next((m for m in cands if _abuf(m.y) is _abuf(op.dy)), None)
                full = next((m for m in cands if m is not half), None)
                n, h, w, c = op.dims
                if half is None or tuple(half.dims) != (n, h // 2, w // 2, c):
                    continue
                if full is not None and not (_abuf(op.add) is _abuf(full.y) and _abuf(op.x) is _abuf(full.x) and tuple(full.dims) == tuple(op.dims)):
                    continue
                if any(any(_readers_of(ops, m.y, exclude=(op,))) for m in cands):      # their results are never written: nobody else may read them
                    continue
            else:
                if prev.kind != 'ew' or not is_apply(prev) or _abuf(prev.y) is not _abuf(op.x) or tuple(prev.dims) != tuple(op.dims):
                    continue
                full = prev
                # its result is written at the pool op's position now: a reader in between would see it too early
                if any(i < at < j for at, _ in _readers_of(ops, full.y)):
                    continue
            group = [m for m in (full, half) if m is not None]
            if not self._ew_merge_intervals_ok(op, full, half, ops[i + 1:j], iv, hit):
                continue
            op.ewm_kind, op.ewm_full, op.ewm_half = op.op, full, half
            if l.fpd_ew_merge_supported(C.byref(self.ew_merge(op)[1])) == 1:
                for m in group:
                    m.ewm_absorbed = True
            else:
                op.ewm_kind = op.ewm_full = op.ewm_half = None

    @staticmethod
    def _ew_merge_intervals_ok(op, full, half, between, iv, hit):
        """The aliasing rule of plan_ew_merge on physical intervals (arena, first element, end): the fused launch's outputs overlap
        none of its inputs (nor each other), and no op issued between the absorbed op(s) and the launch writes what the applies
        read or touches what they write -- those accesses now happen at the launch."""
        group = [m for m in (full, half) if m is not None]
        pool_bwd = op.op == 'maxpool_bwd'
        moved_rd, moved_wr = [], []
        for m in group:
            r, w = m.accesses()
            moved_rd += r + [m.bstats]                                        # (listed under the writes: produced OR consumed)
            moved_wr += [b for b in w if b is not m.bstats and not (pool_bwd and b is _abuf(m.y))]     # pattern 1: the result is never written
        ins = moved_rd + [_abuf(t) for t in ((op.x, op.add if full is None else None) if pool_bwd else (op.add,)) if t is not None]
        outs = moved_wr + [_abuf(op.y)]
        if any(hit(iv(o), iv(b)) for o in outs for b in ins):
            return False
        if any(hit(iv(a), iv(b)) for x, a in enumerate(outs) for b in outs[x + 1:]):
            return False
        for top in between:
            if top is None:
                continue
            acc = top.accesses()
            if acc is None:
                return False
            r, w = acc
            if any(hit(iv(a), iv(b)) for a in w for b in moved_rd + moved_wr) or any(hit(iv(a), iv(b)) for a in r for b in moved_wr):
                return False
        return True

    def ew_merge(self, op):
        """fpd_ew_merge_t of a pool-backward op that evaluates its apply(s) itself (plan_ew_merge decided)."""
        s = R.EwMergeT()
        s.kind = R.EWM_MAXPOOL_BWD if op.ewm_kind == 'maxpool_bwd' else R.EWM_SUMPOOL
        if op.ewm_full is not None:
            s.has_full, s.full = 1, self.ew(op.ewm_full, plain=True)[1]
        if op.ewm_half is not None:
            s.half = self.ew(op.ewm_half, plain=True)[1]
        s.pool = self.ew(op, plain=True)[1]
        return R.OP_EW_MERGE, s

    def _fill_skip(self, op, s):
        """Second 1x1 source of a conv3 that forms its Bottleneck's downsample convolution itself (fpd_conv_t.x2)."""
        sc, p = op.skip_conv, self.A.ptr
        assert _abuf(sc.y) is _abuf(op.residual) and sc.bn is None, 'skip: the downsample convolution must produce exactly this residual'
        s.x2, s.w2, s.bias2, s.C2 = p(_abuf(sc.x)), p(sc.w), p(sc.bias), sc.dims[3]
        s.residual = None

    def plan_skips(self, ops, readers=None):
        """Decide, BEFORE the forward list is lowered, which downsample convolutions (graph: conv3.skip_conv) are formed inside
        the conv3 launch they are the residual of (include/fpd_amd.h: fpd_conv_t.x2): the skip tensor has no other reader
        (among `readers`, default `ops`), both ops run on one lane, neither is an fp8 convolution, and the library serves the
        launch as it will be made.  The downsample op is then lowered as a no-op (`skip_fused`), conv3 is `skip_active`."""
        if os.environ.get('FPD_FUSE_SKIP', '1') == '0':
            return
        l = R.lib()
        readers = ops if readers is None else readers
        for op in ops:
            sc = op.skip_conv if op is not None and op.kind == 'conv' else None
            if sc is None or not any(o is sc for o in ops) or (op.lane or 0) != (sc.lane or 0):
                continue
            if op.w8 is not None or sc.w8 is not None or sc.bn is not None:
                continue
            if _abuf(sc.y) is not _abuf(op.residual) or sc.out_stats is not None:
                continue
            if any(_readers_of(readers, sc.y, exclude=(op,))):
                continue
            s = self.conv(op, plain=True)[1]
            self._fill_skip(op, s)
            if l.fpd_conv_skip_supported(C.byref(s)) == 1:
                op.skip_active = True
                sc.skip_fused = True

    def plan_stem_act(self, ops, readers=None):
        """The same for a frozen stem's BN + ReLU (graph: stem_fwd.act_ew; fpd_stem_t.act): the elementwise op becomes a no-op and
        the stem writes the activation, where the BN is in eval mode, the stem output has no other reader and the library
        serves the launch."""
        if os.environ.get('FPD_STEM_ACT', '1') == '0':
            return
        readers = ops if readers is None else readers
        for op in ops:
            ae = op.act_ew if op is not None and op.kind == 'stem_fwd' else None
            if ae is None or not any(o is ae for o in ops) or (op.lane or 0) != (ae.lane or 0):
                continue
            if ae.op != 'bnrelu_fwd' or ae.bn is None or ae.bn.mode != 'eval' or _abuf(ae.x) is not _abuf(op.y):
                continue
            if op.out_stats is not None or ae.out_stats is not None:
                continue
            if any(_readers_of(readers, op.y, exclude=(ae,))):
                continue
            op.act_active = ae.stem_fused = R.lib().fpd_stem_act_supported(C.byref(self.stem(op, act=True)[1])) == 1

    @staticmethod
    def plan_upadd(ops, readers=None, dtype=R.BF16):
        """Decide, BEFORE memory is planned, which up-adds of a frozen graph are formed on load by the fused Bottleneck that reads
        them (include/fpd_amd.h: fpd_bneck_t.x2): the up-add produces no statistics, its result has exactly one reader (among
        `readers`, default `ops`) and that reader is a single fused Bottleneck on the same lane (not a member of a 'bneck2'), the
        knob FPD_BNECK_UPADD is on and the library serves the dimensions.  The Bottleneck then names both sources as its inputs
        (`x`, `x2`; `upadd_op` keeps the relation), the up-add is `upadd_absorbed`: it accesses nothing, is lowered as a no-op and
        its result is never allocated.  A train-mode graph has no fused Bottlenecks (and its up-adds feed statistics): none
        qualifies.  Returns the number absorbed."""
        if os.environ.get('FPD_BNECK_UPADD', '1') == '0':
            return 0
        readers = ops if readers is None else readers
        n = 0
        for op in ops:
            if op is None or op.kind != 'bneck' or op.x2 is not None:
                continue
            ua = getattr(op.x, 'producer', None)
            if ua is None or ua.kind != 'ew' or ua.op != 'upadd_fwd' or ua.out_stats is not None or op.x.stats is not None:
                continue
            if ua.y is not op.x or op.x.persistent or not any(o is ua for o in ops) or (op.lane or 0) != (ua.lane or 0):
                continue
            if [o for _, o in _readers_of(readers, op.x, by_buf=False)] != [op]:      # (by Act: no tensor has a buf yet)
                continue
            s = R.BneckT()
            (s.N, s.H, s.W, s.C, s.P), s.dtype = op.dims, dtype
            if R.lib().fpd_bneck_upadd_supported(C.byref(s)) != 1:
                continue
            op.upadd_op, op.x, op.x2 = ua, ua.x, ua.x2
            ua.upadd_absorbed = True
            n += 1
        return n

    def _fill_fold(self, op, s):
        """Fold fields of a data gradient that evaluates its BN-backward apply itself (plan_folds decided)."""
        if not op.fold_active:
            return
        ap, p = op.fold_apply, self.A.ptr
        assert ap.add is None and _abuf(ap.y) is _abuf(op.x), 'fold: the apply must produce exactly this operand'
        s.x = p(_abuf(ap.dy))                               # the masked gradient; the operand proper is evaluated in-kernel
        s.fold_x, s.fold_bn, s.fold_stats = p(_abuf(ap.x)), self.bn(ap.bn), p(ap.bstats)
        s.fold_dgamma, s.fold_dbeta = p(ap.dgamma), p(ap.dbeta)
        # its other consumer -- the convolution's weight gradient -- reads the evaluated operand unless it is formed right here
        skip = op.fused_active and not op.fold_other_readers
        s.fold_out = None if skip else p(_abuf(ap.y))

    def _register_slabs(self, wg, s, n, nbias):
        """The launch of struct `s` writes weight gradient `wg` (an IR 'wgrad' / 'stem_wgrad' op) as `n` slabs of its own, no
        device-scope atomics: finish_partials() places them and patches `s`, the bucket's 'wreduce' sums them.  With n == 0, and in
        every struct never registered, the slab fields stay null as ctypes made them: the launch sums into dw itself."""
        if n > 0:
            numel = wg.dw.numel
            stride = (numel + nbias + 63) // 64 * 64        # weight slab + bias partials
            self.partials[id(wg)] = Slabs(s, wg.dw, numel, stride, n, self.partial_elems, wg.dbias, nbias)
            self.partial_elems += n * stride

    def _fuse_wgrad(self, op, s, n):
        """The data-gradient launch `op` (struct `s`, a ConvT -- possibly a field of a pair struct) also forms the weight
        gradient of `op.fused_wgrad` into `n` slabs: register them like a weight-gradient kernel's and turn the separate
        'wgrad' op into a no-op."""
        fw = op.fused_wgrad
        assert fw.dw.numel == s.C * s.K, (fw.dw.numel, s.C, s.K)     # [Kf][1][1][Cf] = [s.C][s.K]
        self._register_slabs(fw, s, n, s.C)
        s.wg_bias = 1 if fw.dbias is not None else 0
        s.wg_count = n                                      # the launch refuses a geometry that writes another number of slabs
        self.fused.add(id(fw))
        op.fused_active = True

    def wquant(self, entries):
        """[(master weight Buf, e4m3 Buf, scale Buf)] -> one table-driven launch (fpd_weight_quant_f8)."""
        ents = []
        for w, q, sc in entries:
            e = R.WquantEntryT()
            e.w, e.w8, e.scale = self.A.ptr(w), self.A.ptr(q), self.A.ptr(sc)
            e.K, e.RSC = w.shape[0], w.numel // w.shape[0]
            ents.append(e)
        s = R.TableT()
        s.table, s.n, s.dtype, s.max_elems = self._table(ents, R.WquantEntryT), len(ents), self.dtype, 0
        return R.OP_WQUANT, s

    def bneck(self, op):
        s = R.BneckT()
        (s.N, s.H, s.W, s.C, s.P) = op.dims
        s.dtype = self.dtype
        p = self.A.ptr
        s.x, s.y = p(_abuf(op.x)), p(_abuf(op.y))
        s.w1, s.b1, s.w2, s.b2, s.w3, s.b3 = p(op.w1), p(op.b1), p(op.w2), p(op.b2), p(op.w3), p(op.b3)
        s.bn1, s.bn2, s.bn3 = self.bn(op.bn1), self.bn(op.bn2), self.bn(op.bn3)
        s.folded = p(op.folded)                            # (the fold table's Buf, or None)
        if op.x2 is not None:                              # up-add on load (plan_upadd): y overlaps neither source in the arena
            yb = _abuf(op.y)
            for t in (_abuf(op.x), _abuf(op.x2)):
                assert t.arena != yb.arena or t.off + t.numel <= yb.off or yb.off + yb.numel <= t.off, 'bneck: y overlaps a source of its up-add'
            s.x2 = p(_abuf(op.x2))
        return R.OP_BNECK, s

    def head(self, op):
        s = R.HeadT()
        (s.N, s.H, s.W, s.C, s.J) = op.dims
        s.dtype = self.dtype
        p = self.A.ptr
        s.y0, s.x, s.score, s.next = p(_abuf(op.y0)), p(_abuf(op.x)), p(_abuf(op.score)), p(_abuf(op.next))
        s.w_fc, s.b_fc, s.w_score, s.b_score = p(op.w_fc), p(op.b_fc), p(op.w_score), p(op.b_score)
        s.w_fc2, s.b_fc2, s.w_score2, s.b_score2 = p(op.w_fc2), p(op.b_fc2), p(op.w_score2), p(op.b_score2)
        s.bn = self.bn(op.bn)
        s.folded = p(op.folded)
        return R.OP_HEAD, s

    def wgrad(self, op):
        if id(op) in self.fused:                           # formed by the data-gradient launch (fpd_conv_t.wg_partial)
            return _nop()
        s = R.WgradT()
        (s.N, s.H, s.W, s.C, s.K, s.R, s.S, s.stride, s.pad, s.P, s.Q) = op.dims
        s.dtype = self.dtype
        p = self.A.ptr
        s.x, s.dy, s.dw, s.dbias = p(_abuf(op.x)), p(_abuf(op.dy)), p(op.dw), p(op.dbias)
        s.bn = self.bn(op.bn)
        if self.use_partials:
            # two-stage reduction instead of device-scope atomics: ask the library how many slabs this launch writes
            self._register_slabs(op, s, R.lib().fpd_wgrad_num_partials(C.byref(s)), s.K)
        return R.OP_WGRAD, s

    def wreduce(self, op):
        """Second stage of the weight-gradient reduction for the convolutions of ONE gradient bucket (op.wgrads, all
        lowered before this op): dw += sum of slabs, one launch.  The table is filled in by finish_partials()."""
        if not any(id(w) in self.partials for w in op.wgrads):
            return _nop()
        t = R.TableT()
        self.reduces.append((op, t))
        return R.OP_WREDUCE, t

    def finish_partials(self):
        """Allocate the slab workspace, patch the recorded wgrad structs and fill the reduce tables (call after every
        backward op has been lowered and BEFORE the structs are copied into the plan)."""
        if not self.partials:
            return
        ws = torch.empty(self.partial_elems, dtype=torch.float32, device=self.A.device)
        self.keep.append(ws)
        for wg, r in self.partials.items():
            if wg in self.fused:                          # formed by a data-gradient launch: r.s is its ConvT
                r.s.wg_partial, r.s.wg_stride = ws.data_ptr() + 4 * r.off, r.stride
            else:
                r.s.partial, r.s.partial_stride = ws.data_ptr() + 4 * r.off, r.stride
        for op, t in self.reduces:
            ents, mx = [], 0
            for w in op.wgrads:
                r = self.partials.get(id(w))
                if r is None:
                    continue
                for at, dst, count in ((r.off, r.dw, r.numel), (r.off + r.numel, r.dbias, r.nbias)):      # a slab: weights, then bias sums
                    if dst is not None:
                        e = R.WreduceEntryT()
                        e.partial, e.dw, e.n, e.stride, e.count = ws.data_ptr() + 4 * at, self.A.ptr(dst), count, r.stride, r.n
                        ents.append(e)
                mx = max(mx, r.numel)
            t.table, t.n, t.dtype, t.max_elems = self._table(ents, R.WreduceEntryT), len(ents), self.dtype, mx

    def stem(self, op, act=None):
        """act: whether a 'stem_fwd' applies its `act_ew`; None = as decided (`act_active`), True = plan_stem_act's candidate."""
        s = R.StemT()
        (s.N, s.H, s.W, s.K, s.P, s.Q) = op.dims
        s.dtype = self.dtype
        p = self.A.ptr
        s.x = p(op.image)
        if op.kind == 'stem_fwd':
            s.w, s.bias, s.y, s.out_stats = p(op.w), p(op.bias), p(_abuf(op.y)), p(op.out_stats)
            if op.act_active if act is None else act:      # bn1 + ReLU in the epilogue: the stem writes the activation
                s.act, s.y = self.bn(op.act_ew.bn), p(_abuf(op.act_ew.y))
            return R.OP_STEM_FWD, s
        s.dy, s.dw, s.dbias = p(_abuf(op.dy)), p(op.dw), p(op.dbias)
        if self.use_partials:                  # same two-stage reduction as the other weight gradients (no atomics)
            self._register_slabs(op, s, R.lib().fpd_stem_wgrad_num_partials(C.byref(s)), s.K)
        return R.OP_STEM_WGRAD, s

    def ew(self, op, plain=False):
        """plain=True: the op's own struct as a member of an OP_EW_MERGE -- plan_ew_merge's decisions are ignored, the others are not."""
        if op.absorbed(merged=not plain):
            return _nop()
        if not plain and op.ewm_kind is not None:
            return self.ew_merge(op)
        s = R.EwT()
        s.op, s.dtype = _EW[op.op], self.dtype
        (s.N, s.H, s.W, s.C) = op.dims
        p = self.A.ptr
        s.x, s.x2, s.dy, s.add, s.y = p(_abuf(op.x)), p(_abuf(op.x2)), p(_abuf(op.dy)), p(_abuf(op.add)), p(_abuf(op.y))
        s.out_stats, s.bstats, s.dgamma, s.dbeta = p(op.out_stats), p(op.bstats), p(op.dgamma), p(op.dbeta)
        s.bn = self.bn(op.bn)
        return R.OP_EW, s

    def _table(self, entries, cls):
        arr = (cls * len(entries))(*entries)
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.A.device)
        self.keep.append(raw)
        return raw.data_ptr()

    def bnupd(self, op):
        ents = []
        for bn in op.bns:
            e = R.BnupdEntryT()
            e.stats, e.running_mean, e.running_var = self.A.ptr(bn.stats), self.A.ptr(bn.rmean), self.A.ptr(bn.rvar)
            e.num_batches_tracked = self.A.ptr(bn.nbt)
            e.count, e.momentum, e.C = float(bn.count), G.BN_MOMENTUM, bn.C
            ents.append(e)
        s = R.TableT()
        s.table, s.n, s.dtype, s.max_elems = self._table(ents, R.BnupdEntryT), len(ents), self.dtype, 0
        return R.OP_BNUPD, s

    def wprep(self, entries):
        ents, mx = [], 0
        for w, wf, wb in entries:
            e = R.WprepEntryT()
            e.w, e.w_fwd, e.w_bwd = self.A.ptr(w), self.A.ptr(wf), self.A.ptr(wb)
            (e.K, e.R, e.S, e.C) = w.shape
            mx = max(mx, w.numel)
            ents.append(e)
        s = R.TableT()
        s.table, s.n, s.dtype, s.max_elems = self._table(ents, R.WprepEntryT), len(ents), self.dtype, mx
        return R.OP_WPREP, s

    def memset(self, arena_name, off=0, n=None):
        t = self.A.tensor(arena_name)
        n = t.numel() - off if n is None else n
        s = R.MemsetT()
        s.ptr, s.bytes = t.data_ptr() + off * t.element_size(), n * t.element_size()
        return R.OP_MEMSET, s

    def op(self, op):
        if _WHATIF and _whatif_drop(op, getattr(self, 'train', True)):
            return _nop()
        if op.kind == 'conv2':
            s = R.ConvPairT()
            s.a, s.b = self.conv(op.a, plain=True)[1], self.conv(op.b, plain=True)[1]
            if self.use_partials and op.a.fused_wgrad is not None and op.b.fused_wgrad is not None:
                na, nb = C.c_int32(0), C.c_int32(0)
                R.check(R.lib().fpd_conv_pair_fused_wgrad_partials(C.byref(s), C.byref(na), C.byref(nb)), 'fpd_conv_pair_fused_wgrad_partials')
                if na.value > 0 and nb.value > 0:          # s.a / s.b are views INTO the pair struct: patched in place later
                    self._fuse_wgrad(op.a, s.a, na.value)
                    self._fuse_wgrad(op.b, s.b, nb.value)
            self._fill_fold(op.a, s.a)
            self._fill_fold(op.b, s.b)
            return R.OP_CONV_PAIR, s
        if op.kind == 'ew2':
            live = [m for m in op.members() if not m.absorbed()]
            if len(live) < 2:                              # absorbed members leave the pair: a folded apply's partner goes out
                return self.ew(live[0]) if live else _nop()      # alone, a pair inside the pool backward behind it not at all
            s = R.EwPairT()
            s.a, s.b = self.ew(op.a)[1], self.ew(op.b)[1]
            return R.OP_EW_PAIR, s
        if op.kind == 'bneck2':
            s = R.BneckPairT()
            s.a, s.b = self.bneck(op.a)[1], self.bneck(op.b)[1]
            return R.OP_BNECK_PAIR, s
        if op.kind == 'head_fold':
            return R.OP_HEAD_FOLD, self.head(op.target)[1]
        if op.kind == 'bneck_fold':
            return R.OP_BNECK_FOLD, self.bneck(op.target)[1]
        if op.kind == 'affsum':
            s = R.AffsumT()
            (s.N, s.H, s.W, s.C) = op.dims
            s.dtype, s.relu, s.nterms = self.dtype, 1 if op.relu else 0, len(op.terms)
            assert len(op.terms) <= R.AFFSUM_MAX and op.out_stats is None
            for j, (t, bn, up) in enumerate(op.terms):
                s.t[j].x, s.t[j].bn, s.t[j].up = self.A.ptr(_abuf(t)), self.bn(bn), up
            s.y = self.A.ptr(_abuf(op.y))
            return R.OP_AFFSUM, s
        if op.kind == 'nchw2nhwc':
            s = R.LayoutT()
            (s.N, s.C, s.H, s.W) = op.dims
            s.src, s.dst, s.dtype = self.A.ptr(op.image), self.A.ptr(_abuf(op.y)), self.dtype
            return R.OP_NCHW2NHWC, s
        if op.kind == 'grad_ready':
            return _nop()
        return {'conv': self.conv, 'bneck': self.bneck, 'head': self.head, 'wgrad': self.wgrad, 'wreduce': self.wreduce, 'stem_fwd': self.stem,
                'stem_wgrad': self.stem, 'ew': self.ew, 'bnupd': self.bnupd}[op.kind](op)


class ModelState:
    """Flat HBM arenas of one model's state_dict (see graph.ParamTable)."""

    def __init__(self, table, device, dtype):
        self.table, self.device, self.dtype = table, device, dtype
        self.A = Arenas(device, dtype)
        for name in ('param', 'rstat', 'nbt'):
            self.A.alloc(name, table.sizes[name])
        self.A.alloc('grad', table.sizes['param'])


class GraphInstance:
    """One HourglassGraph realised on the device: activation/statistics/working-weight arenas + native plan.

    Plan ranges (self.rng): 'prep' (zero statistics, refresh working weight copies), 'fwd', and for training
    graphs 'bwd' (zero parameter gradients, backward ops).  `extra_ops` (e.g. the fused loss) can be spliced
    between fwd and bwd by the trainer before finalize()."""

    def __init__(self, state, cfg, batch, height, width, train, image=None, share_weights_with=None):
        self.state, self.train = state, train
        self._wlp_owner = share_weights_with       # another instance of the same model whose working weights we read
        self.dtype = state.dtype
        env = os.environ.get
        if cfg.get('arch') == 'hrnet':
            self.g = G.HRNetGraph(state.table, cfg['extra'], cfg['J'], batch, height, width, train,
                                  wlp_is_master=(self.dtype == R.F32),
                                  wgrad_batch=int(env('FPD_WGRAD_BATCH')) if env('FPD_WGRAD_BATCH') else None,
                                  fp8=bool(cfg.get('fp8', False)))
        else:
            self.g = G.HourglassGraph(state.table, cfg['F'], cfg['S'], cfg['J'], batch, height, width, train,
                                      num_blocks=cfg.get('num_blocks', 1), wlp_is_master=(self.dtype == R.F32),
                                      fuse_bneck=(self.dtype == R.BF16 and not train and env('FPD_FUSE_BNECK', '1') != '0'),
                                      pair_branches=env('FPD_PAIR', '1') != '0', fuse_head=env('FPD_FUSE_HEAD', '1') != '0',
                                      fuse_skip=(self.dtype == R.BF16 and env('FPD_FUSE_SKIP', '1') != '0'),
                                      fuse_stem_act=(self.dtype == R.BF16 and env('FPD_STEM_ACT', '1') != '0'),
                                      wgrad_batch=int(env('FPD_WGRAD_BATCH')) if env('FPD_WGRAD_BATCH') else None)
        self.A = Arenas(state.device, self.dtype, parent=state.A)
        self.low = Lowering(self.A, self.dtype)
        self.low.train = train
        self.plan = R.Plan()
        self.rng = {}
        self.graphs = {}
        self._image_ext = image
        self._finalized = False
        self.mid_ops = []          # IR ops between fwd and bwd (loss)
        self.mid_native = []       # callables adding native ops for the mid section

    def _schedule(self, name, ir_ops):
        """Multi-lane schedule of plan range `name`; ir_ops[k] is the IR op behind plan op begin+k (None = barrier)."""
        b, e = self.rng[name]
        assert e - b == len(ir_ops), (name, b, e, len(ir_ops))
        if not self.lanes_enabled or not any(o is not None and o.lane for o in ir_ops):
            return
        sch = PhaseSchedule([((o.lane or 0), o.accesses()) if o is not None else (0, None) for o in ir_ops], self.g.n_lanes)
        for k in range(len(ir_ops)):
            if sch.lanes[k] or sch.waits[k]:
                self.plan.set_schedule(b + k, sch.lanes[k], [b + w for w in sch.waits[k]])
        self.schedules[name] = sch

    def finalize(self):
        g = self.g
        ops = g.fwd + self.mid_ops + g.bwd
        self.lanes_enabled = os.environ.get('FPD_LANES', '1') != '0'
        self.schedules = {}
        # several lanes in flight: do not hand a released block to the very next tensor (false WAR dependencies)
        # (a frozen graph has a single lane: immediate reuse keeps its working set small)
        delay = int(os.environ.get('FPD_REUSE_DELAY', '400')) if self.lanes_enabled else 0
        if not self.train:
            delay = 0
        if not self.train and self.dtype == R.BF16:
            self.low.plan_upadd(g.fwd, readers=ops, dtype=self.dtype)      # before planning: lifetimes are right by construction
        act = G.plan_memory(ops, reuse_delay=delay)
        self.act_elems = act
        self.A.alloc('act', act)
        self.A.alloc('stats', g.stats_size)
        if self._wlp_owner is not None:            # same ParamTable / same graph -> same layout of the working-weight arena
            o = self._wlp_owner                    # and of the folded BN tables, both written by the owner's 'prep' phase
            assert o.g.wlp_size == g.wlp_size and o.g.fold_size == g.fold_size and not self.train
            self.A.t['wlp'] = o.A.t['wlp']
            self.A.t['fold'] = o.A.t['fold']
        else:
            self.A.alloc('wlp', g.wlp_size)
            self.A.alloc('fold', g.fold_size)
        if self._image_ext is not None:
            self.A.t['image'] = self._image_ext
        else:
            self.A.alloc('image', g.N * 3 * g.H * g.W)
        p = self.plan
        b = len(p)
        p.add(*self.low.memset('stats'))
        entries = []
        for k in self.state.table.conv_keys():
            if k in g.MASTER_ONLY:
                continue
            wf, wb = g.wfwd.get(k), g.wbwd.get(k)
            if wf is not None or wb is not None:
                entries.append((self.state.table[k], wf, wb))
        if entries:
            p.add(*self.low.wprep(entries))
        w8 = getattr(g, 'w8', None)
        if w8:                                     # e4m3 copies + scales of the convolutions that run on the fp8 matrix pipe
            self.A.alloc('w8', g.w8_size)
            self.A.alloc('w8s', g.w8s_size)
            p.add(*self.low.wquant([(self.state.table[k], q, sc) for k, (q, sc) in w8.items()]))
        for op in g.fwd:                           # frozen fused Bottlenecks: fold BN + biases into tables once
            for sub in op.members():
                if sub.kind in ('bneck', 'head') and sub.folded is not None:
                    p.add(*self.low.op(G.Op(sub.kind + '_fold', target=sub)))
        self.rng['prep'] = (b, len(p))
        b = len(p)
        self.op_index = {}                         # id(IR op) -> plan op (bench.py times single recorded ops through it)
        self.low.plan_skips(g.fwd, readers=ops)
        self.low.plan_stem_act(g.fwd, readers=ops)
        for op in g.fwd:
            self.op_index[id(op)] = p.add(*self.low.op(op))
        self.rng['fwd'] = (b, len(p))
        self._schedule('fwd', list(g.fwd))
        b = len(p)
        for fn in self.mid_native:
            fn(p)
        self.rng['mid'] = (b, len(p))
        if self.train:
            b = len(p)
            p.add(*self.low.memset('grad'))
            self.low.use_partials = True
            bwd_ir = [op for op in g.bwd if op.kind != 'seed']
            self.low.plan_folds(bwd_ir)
            if not isinstance(g, G.HRNetGraph):       # (hourglass only: the HRNet backward has no such groups worth a launch)
                self.low.plan_ew_merge(bwd_ir)
            lowered = [self.low.op(op) for op in bwd_ir]
            self.low.finish_partials()                # patches the wgrad structs / fills the per-bucket reduce tables
            self.bucket_ops = {}                      # gradient bucket -> plan op after which its grad slice is final
            for ir, (code, st) in zip(bwd_ir, lowered):
                k = self.op_index[id(ir)] = p.add(code, st)
                if ir.kind == 'grad_ready':
                    self.bucket_ops[ir.bucket] = k
                    p.mark_event(k)
            self.rng['bwd'] = (b, len(p))
            self._schedule('bwd', [None] + bwd_ir)
        self._finalized = True
        return self

    def run(self, name, stream=None):
        gid = self.graphs.get(name)
        if gid is not None:
            self.plan.replay(gid, stream)
            return
        b, e = self.rng[name]
        self.plan.run(b, e, stream)

    def capture(self, names, cap_stream):
        """Capture plan ranges into hipGraphs (one per name) on `cap_stream` (a non-default stream; the ranges must
        already have run eagerly once so one-time kernel attributes are set).  run(name) then replays the graph:
        the ~1 700 launches of a step stop costing host time one by one."""
        torch.cuda.synchronize()
        with torch.cuda.stream(cap_stream):
            for n in names:
                b, e = self.rng[n]
                self.graphs[n] = self.plan.capture(b, e, C.c_void_p(cap_stream.cuda_stream))
        torch.cuda.synchronize()

    def image(self):
        return self.A.tensor('image').view(self.g.N, 3, self.g.H, self.g.W)

    def calibrate_running_stats(self):
        """After one train-mode forward: overwrite every BN's running estimates with this batch's statistics
        (unbiased variance).  Used to give random-init synthetic teachers sane eval-mode statistics
        (SURVEY.md section 8(d)); not part of the train step."""
        assert self.train
        torch.cuda.synchronize()
        for bn in self.g.bns:
            st = self.A.stats_read(bn.stats).sum(0)
            mean = st[0] / bn.count
            var = (st[1] / bn.count - mean * mean).clamp_min(0) * (bn.count / max(bn.count - 1, 1))
            self.A.view(bn.rmean).copy_(mean.float())
            self.A.view(bn.rvar).copy_(var.float())

    def output_view(self, i):
        return self.A.view(self.g.outputs[i].buf)          # NHWC in act dtype

    def out_grad_view(self, i):
        return self.A.view(self.g.out_grads[i].buf)


class FusedFPDStep:
    """The fused FPD iteration (lib/core/function.py:119-147 of the reference) on one GPU:
         teacher forward (eval BN) -> student forward (train BN) -> fused pose+KD loss fwd/bwd
         -> student backward -> [RCCL all-reduce of the flat gradient] -> the flat optimizer update: Adam with the step's own
         moments, or the op that the optimizer given as adam= (a lib.utils.utils.FusedAdam or FusedAdamW) or sgd= (a FusedSGD)
         plans itself (plan_op)
         [-> ema=: the weight average of a lib.utils.utils.ModelEma, one more launch in the optimizer's range].
    clip=: a lib.utils.utils.GradClipper of the student clips the (reduced) gradient to a global L2 norm at the head of the
    optimizer's range.
    accum=k > 1: one optimizer update per window of k student_step calls (micro-batches), see _add_accum.
    No host synchronisation inside; losses are read back only when asked for."""

    def __init__(self, student_state, student_cfg, teacher_state, teacher_cfg, batch, height, width, alpha,
                 lr=2.5e-4, betas=(0.9, 0.999), eps=1e-8, world_size=1, adam=None, teacher_chunks=None,
                 use_target_weight=(True, True), ohkm=None, sgd=None, kl=None, ema=None,
                 clip=None, accum=None):
        dev = student_state.device
        if accum is None:
            accum = 1
        if isinstance(accum, bool) or not isinstance(accum, int) or not 1 <= accum <= 1024:
            raise R.FpdError('FusedFPDStep: accum=%r: an integer in [1, 1024] (micro-batches per optimizer update)' % (accum,))
        self.accum = accum
        if adam is not None and sgd is not None:
            raise R.FpdError('FusedFPDStep: adam= and sgd= are mutually exclusive')
        # JointsMSELoss(use_target_weight) of the pose / distillation criterion (tools/fpd_train.py:145-147,177-179):
        # False = that term ignores the loader's target_weight (loss.py:30-37), i.e. a weight buffer of ones
        self.use_w = (bool(use_target_weight[0]), bool(use_target_weight[1]))
        self.dtype = student_state.dtype
        self.alpha, self.world_size = alpha, world_size
        self.B, self.J = batch, student_cfg['J']
        # JointsOHKMMSELoss(topk) of the pose / distillation criterion: (k_pose or None, k_kd or None); None (the default) is the
        # JointsMSELoss pair and the plan of before; a None inside the pair is a JointsMSELoss term = every joint kept
        self.ohkm = None
        if ohkm is not None:
            self.ohkm = tuple(self.J if k is None else int(k) for k in ohkm)
            if len(self.ohkm) != 2 or not all(1 <= k <= self.J for k in self.ohkm):
                raise R.FpdError('FusedFPDStep: ohkm=%r: topk must lie in [1, J=%d]' % (ohkm, self.J))
        # JointsKLDLoss(temperature) of the pose / distillation criterion: (T_pose or None, T_kd or None); None (the default) is
        # the plan of before; a None inside the pair is a JointsMSELoss term
        self.kl = None
        if kl is not None:
            if ohkm is not None:
                raise R.FpdError('FusedFPDStep: kl= and ohkm= are mutually exclusive (no kernel pairs a KL term with hard-keypoint mining)')
            self.kl = tuple(None if t is None else float(t) for t in kl)
            if len(self.kl) != 2 or self.kl == (None, None):
                raise R.FpdError('FusedFPDStep: kl=%r: a pair of temperatures, at least one of them not None' % (kl,))
            if not all(t is None or (0.0 < t < float('inf')) for t in self.kl):
                raise R.FpdError('FusedFPDStep: kl=%r: a temperature must be positive' % (kl,))
        # teacher first: it owns the image buffer; its last-stack map is read in place by the loss kernel
        self.teacher = None
        self.teachers = []
        self.tmap = [None, None]
        if teacher_state is not None:
            assert teacher_state.dtype == self.dtype
            # The frozen teacher normalises with running statistics, so its samples are independent: the batch CAN be cut
            # into chunks that run as separate op chains on separate streams (constructor argument teacher_chunks).
            # Measured on MI355X (r01): 1 chunk 15.0 ms/step, 2 chunks 15.0, 4 chunks 17.7 -- beyond three concurrent
            # streams (teacher, student chain, weight-gradient lane) the step gets slower, so the default is 1.
            if teacher_chunks is None:
                teacher_chunks = 1
            while batch % teacher_chunks:
                teacher_chunks -= 1
            cb = batch // teacher_chunks
            self.teacher = GraphInstance(teacher_state, teacher_cfg, cb, height, width, train=False).finalize()
            self.teachers = [self.teacher] + [
                GraphInstance(teacher_state, teacher_cfg, cb, height, width, train=False,
                              share_weights_with=self.teacher).finalize() for _ in range(1, teacher_chunks)]
            self.teacher.run('prep')           # frozen weights: working copies are prepared once, shared by the chunks
            nt = self.teacher.g.outputs[-1].numel * teacher_chunks
            # the teacher runs one batch ahead on its own streams: its last-stack map is staged in two slots
            self.tmap = [torch.zeros(nt, dtype=act_torch_dtype(self.dtype), device=dev) for _ in range(2)]
            self.t_streams = [torch.cuda.Stream(device=dev) for _ in range(teacher_chunks)]
            self.t_stream = self.t_streams[0]
            self.ev_t = [torch.cuda.Event(), torch.cuda.Event()]
            self.ev_chunk = [torch.cuda.Event() for _ in range(teacher_chunks)]
        self._k_t = self._k_s = 0
        # 'loss' (default): the student step waits for the teacher's map in front of the fused loss; 'start': before its forward
        self._late_teacher_wait = True         # (round 3: 10.62 -> 10.51 ms; the FPD_TEACHER_WAIT=start spelling of the old order is gone)
        self.student = GraphInstance(student_state, student_cfg, batch, height, width, train=True)
        g = self.student.g
        self.hh, self.hw = g.outputs[0].shape[1:3]
        A = self.student.A
        A.alloc('target', self.B * self.J * self.hh * self.hw)
        A.alloc('weight', self.B * self.J)
        if self.use_w[0] != self.use_w[1]:
            A.t['weight_kd'] = torch.ones(self.B * self.J, dtype=torch.float32, device=dev)
        if not self.use_w[0]:
            A.tensor('weight').fill_(1.0)
        A.alloc('losses', 4)
        if self.ohkm is not None:
            self._alloc_loss_scratch('ohkm')
            A.alloc('ohkm_masks', len(g.outputs) * 2 * self.B)
        if self.kl is not None:
            self._alloc_loss_scratch('kl')
        self.student.mid_ops = [G.Op('loss', extra_in=list(g.outputs), extra_out=list(g.out_grads))]
        self.student.mid_native = [lambda plan: self._add_loss(plan, 0)]
        self.student.finalize()
        b = len(self.student.plan)                 # second loss op reading the other staged teacher map
        self._add_loss(self.student.plan, 1)
        self.student.rng['mid1'] = (b, len(self.student.plan))
        # optimizer state (torch.optim.Adam semantics, lib/utils/utils.py:69-73)
        n = student_state.table.sizes['param']
        self.n_param = n
        self._dist_work = None
        opt = adam if adam is not None else sgd
        if opt is not None:         # a lib.utils.utils.FusedAdam / FusedAdamW / FusedSGD: its state, step and lr are shared (checkpointable),
            g = opt.param_groups[0]     # its hyperparameters recorded as they are NOW (core.function keys its step cache on them)
            self.m, self.v, self.vmax, self.buf = (getattr(opt, k, None) for k in ('m', 'v', 'vmax', 'buf'))
            self.lr_dev, self.step_dev = opt.lr_dev, opt.step_dev
            self.betas, self.eps = g.get('betas'), g.get('eps')
            opcode, a = opt.plan_op(student_state)
        else:                       # Adam with moments of the step's own
            self.m = torch.zeros(n, dtype=torch.float32, device=dev)
            self.v = torch.zeros(n, dtype=torch.float32, device=dev)
            self.vmax = self.buf = None
            self.lr_dev = torch.full((1,), lr, dtype=torch.float32, device=dev)
            self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
            self.betas, self.eps = betas, eps
            opcode, a = R.OP_ADAM, fill_adam_args(R.AdamT(), student_state, self.m, self.v, lr, betas, eps, self.lr_dev, self.step_dev)
        setattr(self, {R.OP_ADAM: '_adam_args', R.OP_ADAMW: '_adamw_args', R.OP_SGD: '_sgd_args'}[opcode], a)
        self._add_optimizer(opcode, a, clip, ema)
        self._add_accum(student_state)

    def _add_optimizer(self, opcode, args, clip, ema):
        """The optimizer range ('adam' by name whatever the optimizer, so that run / capture / phase timing need not know):
        [clip] -> the optimizer op -> [ema]."""
        b = len(self.student.plan)
        self._add_clip(clip, self.student.state)
        self.student.plan.add(opcode, args)
        self._add_ema(ema, self.student.state)
        self.student.rng['adam'] = (b, len(self.student.plan))

    def _add_accum(self, student_state):
        """accum=k > 1: three one-op ranges behind the optimizer's, over the gradient arena and an arena `acc` of the same size --
        'acc0' (acc = grad), 'acc' (acc += grad) and 'accfin' (grad = acc * *scale_dev).  student_step runs 'acc0' or 'acc'
        behind every backward and closes the window behind the k-th: it fills scale_dev with 1/m (stream-ordered, like lr_dev; m
        is the window's length, so that flush() can close a shorter one with the same recorded op), runs 'accfin' and then
        the tail of a k = 1 step (_update) on the gradient arena, which now holds the window's mean.  All-reduce, clip, optimizer and EMA therefore run
        once per window; nothing is recorded INSIDE the optimizer's range.  The loss op carries no 1/k.  k == 1 adds nothing."""
        self._acc_j = 0                 # micro-batches in the open window
        self._acc_allreduce = None      # the hook of the last student_step: flush() takes none
        self.updates = 0                # windows closed = optimizer updates enqueued (or deferred behind an all-reduce)
        if self.accum == 1:
            return
        dev = student_state.device
        n = self.n_param
        self.acc = torch.empty(n, dtype=torch.float32, device=dev)
        self.scale_dev = torch.ones(1, dtype=torch.float32, device=dev)
        plan = self.student.plan
        for name, mode in (('acc0', R.ACCUM_FIRST), ('acc', R.ACCUM_ADD), ('accfin', R.ACCUM_FIN)):
            a = R.GradAccumT()
            a.n, a.mode = n, mode
            a.grad, a.acc = student_state.A.tensor('grad').data_ptr(), self.acc.data_ptr()
            a.scale_dev = self.scale_dev.data_ptr()
            b = len(plan)
            plan.add(R.OP_GRAD_ACCUM, a)
            self.student.rng[name] = (b, len(plan))

    def _add_clip(self, clip, student_state):
        """clip=: one OP_GRAD_CLIP in front of the optimizer op, INSIDE its range -- student_step, the deferred run behind the
        overlapped all-reduce, flush() and a captured graph all replay that range, so each clips exactly once per update and
        after the gradients are averaged (the loss kernel folds 1/world into them: every rank sees the same reduced arena, hence
        the same norm, and no collective is added).  It scales the gradient arena in place, so the optimizer op is unchanged."""
        self.clip = clip
        if clip is None:
            return
        a = clip.clip_args()
        if a.grad != student_state.A.tensor('grad').data_ptr() or a.n != student_state.table.sizes['param']:
            raise R.FpdError('FusedFPDStep: clip= clips the gradient of another model than the student of this step')
        self._clip_args = a
        self.student.plan.add(R.OP_GRAD_CLIP, a)

    def _add_ema(self, ema, student_state):
        """ema=: one OP_EMA behind the optimizer op, INSIDE its range -- whatever replays that range (student_step, the deferred
        run behind the overlapped all-reduce, a captured graph) averages exactly once per update, and nothing else needs to know.
        It reads the arenas the optimizer and the BN update of this step have just written and writes only the ModelEma's own."""
        self.ema = ema
        if ema is None:
            return
        a = ema.ema_args()
        pa = student_state.A
        if a.seg[0].src != pa.tensor('param').data_ptr() or a.seg[1].src != pa.tensor('rstat').data_ptr():
            raise R.FpdError('FusedFPDStep: ema= averages another model than the student of this step')
        self._ema_args = a
        self.student.plan.add(R.OP_EMA, a)

    def enable_metric(self, min_slots=0):
        """Per-iteration PCK of the last student map against the target, on the device (lib.core.evaluate.DeviceAccuracy).
        `min_slots`: the number of iterations the caller may leave between two drain() calls (the ring is sized to at
        least that; an existing smaller ring is drained by the caller first and replaced)."""
        m = getattr(self, 'metric', None)
        if m is None or m.slots < min_slots:
            assert m is None or m.pending() == 0, 'drain() the metric ring before enlarging it'
            from .lib.core.evaluate import DeviceAccuracy
            g, A = self.student.g, self.student.A
            self.metric = DeviceAccuracy(self.B, self.J, self.hh, self.hw, self.dtype, self.student.state.device,
                                         slots=max(4096, int(min_slots))).bind(
                A.ptr(g.outputs[-1].buf), A.tensor('target').data_ptr(), A.tensor('losses').data_ptr())
        return self.metric

    def _fill_loss(self, s, slot):
        """The fpd_loss_t both loss ops share: maps and gradients of every stack, the staged teacher map of `slot`, target, weights."""
        A, g = self.student.A, self.student.g
        s.B, s.J, s.H, s.W, s.S, s.dtype = self.B, self.J, self.hh, self.hw, len(g.outputs), self.dtype
        s.target_nchw, s.alpha = 1, self.alpha
        for i, (o, d) in enumerate(zip(g.outputs, g.out_grads)):
            s.out[i] = A.ptr(o.buf)
            s.dout[i] = A.ptr(d.buf)
        if self.teacher is not None:
            s.teacher = self.tmap[slot].data_ptr()
        else:                                   # plain (non-KD) training: alpha must be 0, kd term reads the student map
            s.teacher = A.ptr(g.outputs[-1].buf)
        s.target, s.weight = A.tensor('target').data_ptr(), A.tensor('weight').data_ptr()
        s.weight_kd = A.tensor('weight_kd').data_ptr() if 'weight_kd' in A.t else None
        s.losses = A.tensor('losses').data_ptr()
        s.grad_scale = 1.0 / self.world_size

    def _alloc_loss_scratch(self, kind):
        """The arena '<kind>_scratch' of fp64 partial sums that fpd_loss_<kind>_scratch_bytes() asks for at this step's shape."""
        d = R.LossT()
        d.B, d.J, d.H, d.W, d.S = self.B, self.J, self.hh, self.hw, len(self.student.g.outputs)
        query = 'fpd_loss_%s_scratch_bytes' % kind
        nbytes = getattr(R.lib(), query)(d)
        if nbytes < 0:
            R.check(int(nbytes), query)
        self.student.A.alloc(kind + '_scratch', nbytes // 8)

    def _add_loss(self, plan, slot):
        """The zeroing of `losses` and the step's loss op: MSE (csrc/loss_adam.hip), with hard-keypoint mining (csrc/loss_ohkm.hip:
        + topk pair, scratch and masks) or with a spatial-softmax KL term (csrc/loss_kl.hip: + flags, temperatures and scratch)."""
        A = self.student.A
        plan.add(*self.student.low.memset('losses'))
        if self.kl is not None:
            op, k, kind = R.OP_LOSS_KL, R.LossKlT(), 'kl'
            tp, tk = self.kl
            k.kl_pose, k.kl_kd = int(tp is not None), int(tk is not None)
            k.temp_pose, k.temp_kd = tp or 1.0, tk or 1.0
        elif self.ohkm is not None:
            op, k, kind = R.OP_LOSS_OHKM, R.LossOhkmT(), 'ohkm'
            k.topk_pose, k.topk_kd = self.ohkm
            k.masks = A.tensor('ohkm_masks').data_ptr()
        else:
            op, k, kind = R.OP_LOSS, R.LossT(), None
        self._fill_loss(k if kind is None else k.base, slot)
        if kind is not None:
            sc = A.tensor(kind + '_scratch')
            k.scratch, k.scratch_bytes = sc.data_ptr(), sc.numel() * sc.element_size()
        plan.add(op, k)

    def ohkm_masks(self):
        """[S][2][B] int32 of the last step: bit j = joint j of (stack, {pose, kd}, sample) was kept -- synchronises."""
        assert self.ohkm is not None
        n = len(self.student.g.outputs) * 2 * self.B
        return self.student.A.tensor('ohkm_masks')[:n].view(-1, 2, self.B).cpu()

    # ---- data ----
    def set_batch(self, inp, target, target_weight):
        """Copy one loader batch (any device) into the student's fixed HBM buffers (async on the current stream)."""
        self.student.image().copy_(inp, non_blocking=True)
        self.student.A.tensor('target').view(target.shape).copy_(target, non_blocking=True)
        if self.use_w[0]:
            self.student.A.tensor('weight').view(target_weight.shape).copy_(target_weight, non_blocking=True)
        elif self.use_w[1]:
            self.student.A.tensor('weight_kd').view(target_weight.shape).copy_(target_weight, non_blocking=True)
        self._last_inp = inp

    # ---- one iteration = teacher_async(batch) + student_step(batch) ----
    def teacher_async(self, inp=None):
        """Frozen-teacher forward of one batch on the teacher stream.  It may be submitted one batch ahead of the
        student step that consumes it: it then overlaps the previous batch's student forward/backward/Adam (it does
        not depend on the student weights).  `inp` None = reuse the image already in the teacher's buffer."""
        if self.teacher is None:
            return
        slot = self._k_t % 2
        cur = torch.cuda.current_stream()
        n = len(self.teachers)
        for k in reversed(range(n)):                    # chunk 0's stream collects the others at the end
            t, T = self.teachers[k], self.t_streams[k]
            T.wait_stream(cur)                          # inputs staged on the caller's stream; slot free (its loss ran)
            with torch.cuda.stream(T):
                cb = t.g.N
                if inp is not None:
                    t.image().copy_(inp[k * cb:(k + 1) * cb], non_blocking=True)
                t.run('fwd')
                o = t.g.outputs[-1].buf
                self.tmap[slot][k * o.numel:(k + 1) * o.numel].copy_(t.A.tensor('act')[o.off:o.off + o.numel])
                if k:
                    self.ev_chunk[k].record(T)
                else:
                    for j in range(1, n):
                        T.wait_event(self.ev_chunk[j])
                    self.ev_t[slot].record(T)
        self._k_t += 1

    def student_step(self, allreduce=None):
        """Student prep/forward, fused loss (against the staged teacher map), backward, [all-reduce], Adam."""
        s = self.student
        slot = self._k_s % 2
        late = self._late_teacher_wait
        if self.teacher is not None:
            assert self._k_t > self._k_s, 'teacher_async() must be submitted before student_step()'
            if not late:
                torch.cuda.current_stream().wait_event(self.ev_t[slot])
        if self._dist_work is not None:        # previous step's gradient exchange overlapped this step's teacher forward
            self._dist_work()
            self._dist_work = None
            s.run('adam')
        s.run('prep')
        s.run('fwd')
        if self.teacher is not None and late:  # only the fused loss reads the teacher's map: the student's own forward
            torch.cuda.current_stream().wait_event(self.ev_t[slot])      # need not wait for a teacher that is still running
        s.run('mid' if slot == 0 else 'mid1')
        if getattr(self, 'metric', None) is not None:
            self.metric.enqueue()
        s.run('bwd')
        if self.accum > 1:
            s.run('acc0' if self._acc_j == 0 else 'acc')
            self._acc_j += 1
            self._acc_allreduce = allreduce
            if self._acc_j == self.accum:
                self._close_window()
        else:
            self._update(allreduce)
        self._k_s += 1

    def _update(self, allreduce):
        """The tail of an update on the gradient arena: the all-reduce hook with the optimizer's range deferred, or the range."""
        if allreduce is not None:
            self._dist_work = allreduce(self.student.state.A.tensor('grad'), self.grad_buckets())
        else:
            self.student.run('adam')
        self.updates += 1

    def _close_window(self):
        """grad = the mean of the open window's m micro-batch gradients, then the update."""
        m, self._acc_j = self._acc_j, 0
        self.scale_dev.fill_(1.0 / m)
        self.student.run('accfin')
        self._update(self._acc_allreduce)

    def grad_buckets(self):
        """[(first element, end element, wait)] of the flat gradient arena in completion order: `wait(stream)` makes a
        torch stream wait (on the device, no host sync) for the point of the just-enqueued backward where that slice is
        final, so its all-reduce can be issued on another stream while the rest of the backward runs.  One bucket (the
        whole arena, no wait needed: it is issued behind the backward) when the phases are replayed as hipGraphs."""
        s = self.student
        n = self.n_param
        if self.accum > 1:                     # no slice is final before 'accfin', which is issued behind everything
            return [(0, n, None)]
        if s.graphs.get('bwd') is not None or not getattr(s, 'bucket_ops', None):
            return [(0, n, None)]
        table = s.state.table
        out = []
        for b, (lo, hi) in enumerate(table.buckets):
            op = s.bucket_ops.get(b)
            if hi <= lo:
                continue
            assert op is not None, 'gradient bucket %d [%d, %d) has no completion op: it would never be all-reduced' % (b, lo, hi)
            out.append((lo, hi, (lambda stream, op=op: s.plan.wait_op(op, C.c_void_p(stream.cuda_stream)))))
        cover = sorted((lo, hi) for lo, hi, _ in out)
        assert cover and cover[0][0] == 0 and cover[-1][1] == n and all(a[1] == b[0] for a, b in zip(cover, cover[1:])), \
            'gradient buckets %r do not tile the arena [0, %d)' % (cover, n)
        return out

    def enable_graphs(self):
        """Replay every phase as a hipGraph from now on (call after at least one eager step)."""
        cap = torch.cuda.Stream(device=self.student.state.device)
        for t in self.teachers:
            t.capture(['fwd'], cap)
        self.student.capture(['prep', 'fwd', 'mid', 'mid1', 'bwd', 'adam'] + (['acc0', 'acc', 'accfin'] if self.accum > 1 else []), cap)

    def step(self, allreduce=None):
        """Un-pipelined iteration on the batch given to set_batch(): teacher forward, then the student step."""
        self.teacher_async(getattr(self, '_last_inp', None))
        self.student_step(allreduce)

    def run_pipelined(self, n_steps, allreduce=None):
        """n_steps iterations on the staged batch with the teacher one batch ahead (exactly n_steps teacher forwards and
        n_steps student steps are enqueued; the pipeline starts and ends empty)."""
        inp = getattr(self, '_last_inp', None)
        self.teacher_async(inp)
        for i in range(n_steps):
            if i + 1 < n_steps:
                self.teacher_async(None)
            self.student_step(allreduce)
        self.flush()

    def flush(self):
        """Apply a pending (overlapped) optimizer update -- call after the last step().  accum > 1: first close a partial
        window of m < k micro-batches (scale 1/m, the all-reduce hook of the last student_step); the next window starts anew."""
        if self._acc_j > 0:
            self._close_window()
        if self._dist_work is not None:
            self._dist_work()
            self._dist_work = None
            self.student.run('adam')

    def launches_per_step(self):
        """Plan ops (= kernel launches / memsets; no-ops excluded) one iteration enqueues, per phase."""
        def count(inst, name):
            b, e = inst.rng[name]
            return sum(1 for k in range(b, e) if inst.plan.op_type(k) != R.OP_NOP)
        out = {'teacher_fwd': count(self.teacher, 'fwd') * len(self.teachers)} if self.teacher is not None else {}
        for ph in ('prep', 'fwd', 'mid', 'bwd', 'adam'):
            out['student_' + ph] = count(self.student, ph)
        if self.accum > 1:                     # per micro-batch: 'acc0' or 'acc'; 'accfin' and student_adam run once per window
            out['student_acc'] = count(self.student, 'acc')
            out['student_accfin'] = count(self.student, 'accfin')
        out['total'] = sum(out.values())
        return out

    def losses(self):
        """(pose, kd, total) of the last step -- synchronises."""
        l = self.student.A.tensor('losses')[:2].cpu()
        pose, kd = float(l[0]), float(l[1])
        return pose, kd, (1 - self.alpha) * pose + self.alpha * kd

    def set_lr(self, lr):
        self.lr_dev.fill_(lr)


class ValidateStep:
    """One validation batch of core.function.validate as enqueued work only: copy the batch in, the eval-mode forward, the
    forward of the width-flipped batch (TEST.FLIP_TEST), one fpd_val_post launch (flip_back + shift + average, arg-max,
    quarter-pixel shift, the inverse affine map of every sample, the batch's rows of the device-resident all_preds /
    all_boxes), fpd_loss on the merged map and fpd_pck, which appends {avg_acc, cnt, loss, -} to the device log ring.
    Nothing waits for the device; the caller drains `metric` when it prints a line and downloads the results once.

    The step runs the module's own eval-mode GraphInstance (the one `model(x)` runs), so its maps hold the bits `model(x)`
    returns.  'prep' (working weight copies, folded BN tables) runs once per validation in begin(): the weights do not
    change while it lasts.  For the flip test the last map of the first forward is kept as a copy of that one map
    (N*h*w*J elements) rather than in a second instance, which would hold a second activation arena to save one small
    device-to-device copy.

    With `dark` (TEST.DARK: the blur size) fpd_val_post runs without the quarter-pixel shift and one fpd_dark_refine launch
    on the merged map overwrites x and y of the batch's rows of all_preds with the DARK decode (csrc/dark.hip)."""

    def __init__(self, inst):
        from .lib.core.evaluate import DeviceAccuracy
        assert not inst.train
        self.inst = inst
        o = inst.g.outputs[-1]
        self.N, self.H, self.W, self.J = n, h, w, j = o.shape
        if j > R.MAX_JOINTS:
            raise R.FpdError('ValidateStep: at most %d joints, got %d' % (R.MAX_JOINTS, j))
        self.dtype, dev = inst.dtype, inst.A.device
        self.device = dev
        self.out_ptr = inst.A.ptr(o.buf)
        self.map_a = torch.empty((n, h, w, j), dtype=act_torch_dtype(self.dtype), device=dev)
        self.merged = torch.empty((n, h, w, j), dtype=torch.float32, device=dev)
        self.meta = torch.empty(5 * n, dtype=torch.float64, device=dev)        # center [n,2] | scale [n,2] | score [n]
        self.ones = torch.ones((n, j), dtype=torch.float32, device=dev)
        self.losses = torch.zeros(2, dtype=torch.float64, device=dev)
        self.metric = DeviceAccuracy(n, j, h, w, R.F32, dev, slots=64)
        self._image_copy = None
        self._keep = None
        a = self.args = R.ValPostT()
        a.N, a.J, a.H, a.W, a.dtype = n, j, h, w, self.dtype
        a.center, a.scale, a.score = self.meta.data_ptr(), self.meta.data_ptr() + 16 * n, self.meta.data_ptr() + 32 * n
        a.merged = self.merged.data_ptr()
        self.dark, self._taps = 0, {}                  # blur size (0: off); device taps per blur size
        d = self.dark_args = R.DarkT()
        d.N, d.J, d.H, d.W, d.layout = n, j, h, w, R.DARK_NHWC
        d.hm, d.center, d.scale = a.merged, a.center, a.scale
        s = self.loss = R.LossT()
        s.B, s.J, s.H, s.W, s.S, s.dtype, s.target_nchw, s.alpha = n, j, h, w, 1, R.F32, 1, 0.0
        s.out[0] = s.teacher = self.merged.data_ptr()
        s.losses, s.grad_scale = self.losses.data_ptr(), 1.0

    def begin(self, all_preds, all_boxes, flip_pairs=None, shift=False, post_process=False, use_target_weight=True,
              min_slots=1, dark=0):
        """Start a validation: all_preds [rows,J,3] float32 and all_boxes [rows,6] float64 device tensors the batches write
        into; flip_pairs None = no flip test.  Refreshes the working weights (the model may have trained since).  The ring
        holds at least `min_slots` batches between two drains.  dark: blur size of the DARK decoding, which replaces the
        quarter-pixel shift (0: off)."""
        from .lib.core.inference import dark_ksize, dark_taps_device
        from .lib.utils.transforms import channel_sources
        assert all_preds.dtype == torch.float32 and all_preds.is_contiguous() and tuple(all_preds.shape[1:]) == (self.J, 3)
        assert all_boxes.dtype == torch.float64 and all_boxes.is_contiguous() and tuple(all_boxes.shape[1:]) == (6,)
        assert all_preds.shape[0] == all_boxes.shape[0]
        if self.metric.slots < min_slots:
            from .lib.core.evaluate import DeviceAccuracy
            self.metric = DeviceAccuracy(self.N, self.J, self.H, self.W, R.F32, self.device, slots=int(min_slots))
        self.metric.cursor.zero_()                 # an empty ring without asking the device what an earlier run left in it
        self.metric.read = 0
        self.all_preds, self.all_boxes = all_preds, all_boxes
        a = self.args
        a.rows, a.all_preds, a.all_boxes = all_preds.shape[0], all_preds.data_ptr(), all_boxes.data_ptr()
        self.flip = flip_pairs is not None
        self.dark = dark_ksize(dark)
        a.shift, a.post_process = int(bool(shift) and self.flip), int(bool(post_process) and not self.dark)
        if self.dark:
            if self.H * self.W > R.DARK_MAX_HW:
                raise R.FpdError('ValidateStep: DARK decoding holds the map in LDS, H * W <= %d, got %dx%d' % (R.DARK_MAX_HW, self.H, self.W))
            if self.dark not in self._taps:
                self._taps[self.dark] = dark_taps_device(self.dark, self.device)
            d = self.dark_args
            d.ksize, d.taps, d.rows, d.all_preds = self.dark, self._taps[self.dark].data_ptr(), a.rows, a.all_preds
        for k, s in enumerate(channel_sources(self.J, flip_pairs or [])):
            a.src[k] = s
        self.use_w = bool(use_target_weight)
        self.inst.run('prep')

    @staticmethod
    def _host(v):
        import numpy as np
        return v.numpy() if torch.is_tensor(v) else np.asarray(v)

    def run(self, inp, target, target_weight, center, scale, score, row0):
        """Enqueue one batch; its results land in rows row0 .. row0+N-1.  center / scale [N,2] and score [N] are host arrays
        or tensors in the dtype the dataset delivers (a float32 scale keeps numpy's float32 scale * 200)."""
        import numpy as np
        inst, l, st, n = self.inst, R.lib(), R.current_stream(), self.N
        c, s, sc = self._host(center), self._host(scale), self._host(score)
        host = torch.empty(5 * n, dtype=torch.float64, pin_memory=True)     # a fresh block per batch, as the loader stages
        rows = host.numpy()
        rows[0:2 * n] = np.asarray(c).reshape(-1)
        rows[2 * n:4 * n] = np.asarray(s).reshape(-1)
        rows[4 * n:5 * n] = np.asarray(sc).reshape(-1)
        self.meta.copy_(host, non_blocking=True)
        direct = inp.is_cuda and inp.dtype == torch.float32 and inp.is_contiguous()
        inst.image().copy_(inp, non_blocking=True)
        inst.run('fwd')
        a = self.args
        a.box_f32, a.row0 = int(s.dtype == np.float32), int(row0)
        if self.flip:
            self.map_a.copy_(inst.output_view(-1))
            src = inp
            if not direct:
                if self._image_copy is None:
                    self._image_copy = torch.empty_like(inst.image())
                self._image_copy.copy_(inst.image())
                src = self._image_copy
            R.check(l.fpd_flip_w(src.data_ptr(), inst.image().data_ptr(), src.numel() // src.shape[-1], src.shape[-1], st), 'fpd_flip_w')
            inst.run('fwd')
            a.a, a.b = self.map_a.data_ptr(), self.out_ptr
        else:
            a.a, a.b = self.out_ptr, None
        R.check(l.fpd_val_post(a, st), 'fpd_val_post')
        if self.dark:
            d = self.dark_args
            d.box_f32, d.row0 = a.box_f32, a.row0
            R.check(l.fpd_dark_refine(d, st), 'fpd_dark_refine')
        tgt = target.to(self.device, non_blocking=True).float().contiguous()
        wt = (target_weight.to(self.device, non_blocking=True).float().reshape(n, self.J).contiguous() if self.use_w else self.ones)
        self._keep = (inp, tgt, wt)
        self.losses.zero_()
        self.loss.target, self.loss.weight = tgt.data_ptr(), wt.data_ptr()
        R.check(l.fpd_loss(self.loss, st), 'fpd_loss')
        self.metric.bind(self.merged.data_ptr(), tgt.data_ptr(), self.losses.data_ptr()).enqueue()


def validate_step_for(model, batch_shape):
    """One ValidateStep per (model, batch shape), cached on the module like core.function.fused_step_for caches train steps."""
    inst = model.instance(tuple(batch_shape), False)
    cache = model.__dict__.setdefault('_validate_steps', {})
    hit = cache.get(tuple(batch_shape))
    if hit is None or hit.inst is not inst:        # (.cuda() / .to() drop the module's instances: the step goes with them)
        hit = cache[tuple(batch_shape)] = ValidateStep(inst)
    return hit
