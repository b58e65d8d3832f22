"""`core.loss.JointsMSELoss`, `core.loss.JointsOHKMMSELoss` and `core.loss.JointsKLDLoss` with the reference's interface
(/root/reference/lib/core/loss.py:15-39, 42-84), computed by the fused HIP loss kernels (csrc/loss_adam.hip,
csrc/loss_ohkm.hip).

forward(output[B,J,h,w], target[B,J,h,w], target_weight[B,J,1]) -> 0-dim tensor that supports +=, scalar
multiplication, .item() and .backward(), as lib/core/function.py:128-152 needs.  The closed form the kernel
evaluates, 0.5/(B*J*h*w) * sum w^2 (p-g)^2, equals the reference's per-joint loop.  In the fused training
step (core.function.fpd_train -> executor.FusedFPDStep) the same kernel evaluates the pose and the
distillation term of every stack in one pass; this class is the stand-alone (compatibility) entry.

JointsOHKMMSELoss(use_target_weight, topk=8) averages, per sample, the per-joint losses of the `topk` hardest joints
(online hard keypoint mining).  Among joints of equal loss the lower index is kept (torch.topk leaves that open);
topk == J is JointsMSELoss.  The reference's own tools never instantiate the class (their LOSS.USE_OHKM key is read
nowhere); here tools/fpd_train.py does, and core.function.fpd_train / train run it inside the fused step.

JointsKLDLoss(use_target_weight, temperature=1.0) is the soft-label KL divergence between the spatial softmaxes of the
two heat maps (csrc/loss_kl.hip).  For every (sample n, joint j), s the hw values of the output map, r those of the
target (the teacher map in the distillation slot), T the temperature, p = softmax(s/T), q = softmax(r/T):
    L[n,j] = w[n,j] T^2 sum_x q_x ((r_x - s_x)/T - lse(r/T) + lse(s/T)),   loss = 1/(B J) sum L[n,j],
    d loss / d s_x = w[n,j] T (p_x - q_x) / (B J).
The target weight enters ONCE (not squared as in the MSE criteria, which scale both maps); use_target_weight False =
ones.  It equals T*T * (w * F.kl_div(F.log_softmax(s/T, 1), F.softmax(r/T, 1), reduction='none').sum(1)).sum() / (B J)
on the [B*J, hw] rows.  The reference has no such class; its tools/fpd_train.py:175 invites the choice."""
import torch
import torch.nn as nn

from ... import runtime as R


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target, weight, use_w):
        if not output.is_cuda:
            raise R.FpdError('JointsMSELoss needs CUDA (ROCm) tensors; there is no CPU path')
        l, st = R.lib(), R.current_stream()
        b, j, h, w = output.shape
        if j > 32:
            raise R.FpdError('JointsMSELoss: at most 32 joints supported, got %d' % j)
        dev = output.device
        p = torch.empty((b, h, w, j), dtype=torch.float32, device=dev)
        R.check(l.fpd_nchw_to_nhwc(output.detach().float().contiguous().data_ptr(), p.data_ptr(), b, j, h, w, R.F32, st))
        tgt = target.detach().float().contiguous()
        wt = (weight.detach().float().reshape(b, j).contiguous() if use_w
              else torch.ones((b, j), dtype=torch.float32, device=dev))
        losses = torch.zeros(2, dtype=torch.float64, device=dev)
        dp = torch.empty_like(p)
        a = R.LossT()
        a.B, a.J, a.H, a.W, a.S, a.dtype, a.target_nchw, a.alpha = b, j, h, w, 1, R.F32, 1, 0.0
        a.out[0], a.dout[0] = p.data_ptr(), dp.data_ptr()
        a.teacher, a.target, a.weight, a.losses = p.data_ptr(), tgt.data_ptr(), wt.data_ptr(), losses.data_ptr()
        a.grad_scale = 1.0
        R.check(l.fpd_loss(a, st), 'fpd_loss')
        g = torch.empty((b, j, h, w), dtype=torch.float32, device=dev)
        R.check(l.fpd_nhwc_to_nchw(dp.data_ptr(), g.data_ptr(), b, j, h, w, R.F32, st))
        ctx.save_for_backward(g)
        return losses[0].float()

    @staticmethod
    def backward(ctx, gl):
        (g,) = ctx.saved_tensors
        return g * gl, None, None, None


class JointsMSELoss(nn.Module):
    def __init__(self, use_target_weight):
        super().__init__()
        self.use_target_weight = use_target_weight

    def forward(self, output, target, target_weight):
        return _LossFn.apply(output, target, target_weight, bool(self.use_target_weight))


class _OhkmLossFn(torch.autograd.Function):
    """One fpd_loss_ohkm call with S = 1, alpha = 0 and the teacher set to the output (its distillation term is zero)."""

    @staticmethod
    def forward(ctx, output, target, weight, use_w, topk):
        if not output.is_cuda:
            raise R.FpdError('JointsOHKMMSELoss needs CUDA (ROCm) tensors; there is no CPU path')
        l, st = R.lib(), R.current_stream()
        b, j, h, w = output.shape
        dev = output.device
        p = torch.empty((b, h, w, j), dtype=torch.float32, device=dev)
        R.check(l.fpd_nchw_to_nhwc(output.detach().float().contiguous().data_ptr(), p.data_ptr(), b, j, h, w, R.F32, st))
        tgt = target.detach().float().contiguous()
        wt = (weight.detach().float().reshape(b, j).contiguous() if use_w
              else torch.ones((b, j), dtype=torch.float32, device=dev))
        losses = torch.zeros(2, dtype=torch.float64, device=dev)
        dp = torch.empty_like(p)
        k = R.LossOhkmT()
        a = k.base
        a.B, a.J, a.H, a.W, a.S, a.dtype, a.target_nchw, a.alpha = b, j, h, w, 1, R.F32, 1, 0.0
        a.out[0], a.dout[0] = p.data_ptr(), dp.data_ptr()
        a.teacher, a.target, a.weight, a.losses = p.data_ptr(), tgt.data_ptr(), wt.data_ptr(), losses.data_ptr()
        a.grad_scale = 1.0
        k.topk_pose, k.topk_kd = int(topk), j        # (the distillation term is identically zero here)
        nbytes = l.fpd_loss_ohkm_scratch_bytes(a)
        if nbytes < 0:
            R.check(int(nbytes), 'fpd_loss_ohkm_scratch_bytes')
        scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
        masks = torch.zeros((2, b), dtype=torch.int32, device=dev)
        k.scratch, k.scratch_bytes, k.masks = scratch.data_ptr(), scratch.numel() * 8, masks.data_ptr()
        R.check(l.fpd_loss_ohkm(k, st), 'fpd_loss_ohkm')
        g = torch.empty((b, j, h, w), dtype=torch.float32, device=dev)
        R.check(l.fpd_nhwc_to_nchw(dp.data_ptr(), g.data_ptr(), b, j, h, w, R.F32, st))
        ctx.save_for_backward(g)
        kept = masks[0]
        ctx.mark_non_differentiable(kept)
        return losses[0].float(), kept

    @staticmethod
    def backward(ctx, gl, _gm):
        (g,) = ctx.saved_tensors
        return g * gl, None, None, None, None


class JointsOHKMMSELoss(nn.Module):
    def __init__(self, use_target_weight, topk=8):
        super().__init__()
        self.use_target_weight = use_target_weight
        self.topk = topk

    def forward(self, output, target, target_weight):
        loss, self.last_mask = _OhkmLossFn.apply(output, target, target_weight, bool(self.use_target_weight), int(self.topk))
        return loss


class _KlLossFn(torch.autograd.Function):
    """One fpd_loss_kl call with S = 1, alpha = 0, the KL term in the pose slot and an MSE distillation term against the
    output itself (identically zero)."""

    @staticmethod
    def forward(ctx, output, target, weight, use_w, temperature):
        if not output.is_cuda:
            raise R.FpdError('JointsKLDLoss needs CUDA (ROCm) tensors; there is no CPU path')
        l, st = R.lib(), R.current_stream()
        b, j, h, w = output.shape
        dev = output.device
        p = torch.empty((b, h, w, j), dtype=torch.float32, device=dev)
        R.check(l.fpd_nchw_to_nhwc(output.detach().float().contiguous().data_ptr(), p.data_ptr(), b, j, h, w, R.F32, st))
        tgt = target.detach().float().contiguous()
        wt = (weight.detach().float().reshape(b, j).contiguous() if use_w
              else torch.ones((b, j), dtype=torch.float32, device=dev))
        losses = torch.zeros(2, dtype=torch.float64, device=dev)
        dp = torch.empty_like(p)
        k = R.LossKlT()
        a = k.base
        a.B, a.J, a.H, a.W, a.S, a.dtype, a.target_nchw, a.alpha = b, j, h, w, 1, R.F32, 1, 0.0
        a.out[0], a.dout[0] = p.data_ptr(), dp.data_ptr()
        a.teacher, a.target, a.weight, a.losses = p.data_ptr(), tgt.data_ptr(), wt.data_ptr(), losses.data_ptr()
        a.grad_scale = 1.0
        k.kl_pose, k.kl_kd, k.temp_pose, k.temp_kd = 1, 0, float(temperature), 1.0
        nbytes = l.fpd_loss_kl_scratch_bytes(a)
        if nbytes < 0:
            R.check(int(nbytes), 'fpd_loss_kl_scratch_bytes')
        scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
        k.scratch, k.scratch_bytes = scratch.data_ptr(), scratch.numel() * 8
        R.check(l.fpd_loss_kl(k, st), 'fpd_loss_kl')
        g = torch.empty((b, j, h, w), dtype=torch.float32, device=dev)
        R.check(l.fpd_nhwc_to_nchw(dp.data_ptr(), g.data_ptr(), b, j, h, w, R.F32, st))
        ctx.save_for_backward(g)
        return losses[0].float()

    @staticmethod
    def backward(ctx, gl):
        (g,) = ctx.saved_tensors
        return g * gl, None, None, None, None


class JointsKLDLoss(nn.Module):
    def __init__(self, use_target_weight, temperature=1.0):
        super().__init__()
        if not 0.0 < float(temperature) < float('inf'):
            raise ValueError('JointsKLDLoss: temperature must be positive, got %r' % (temperature,))
        self.use_target_weight = use_target_weight
        self.temperature = float(temperature)

    def forward(self, output, target, target_weight):
        return _KlLossFn.apply(output, target, target_weight, bool(self.use_target_weight), self.temperature)
