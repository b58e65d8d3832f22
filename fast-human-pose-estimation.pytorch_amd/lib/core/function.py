"""`core.function.fpd_train` with the reference's signature (/root/reference/lib/core/function.py:99-187), driving
the fused MI355X step (executor.FusedFPDStep): per batch the frozen-teacher forward, the student forward/backward, the
pose + distillation JointsMSELoss of every stack, the data-parallel gradient exchange and Adam run as recorded HIP
plans with no host synchronisation; the teacher runs one batch ahead on its own stream (it does not depend on the
student weights).  Like the reference (function.py:150-155) EVERY iteration feeds the loss and accuracy meters: the
device appends {avg_acc, cnt, pose, kd} of each iteration to a ring (csrc/pck.hip) that is drained -- the only host
synchronisation of the loop -- when a log line is due (PRINT_FREQ) and at the end of the epoch.

Not silently substituted: the fused step implements Adam, AdamW and SGD (lib.utils.utils.FusedAdam / FusedAdamW / FusedSGD) and JointsMSELoss /
JointsOHKMMSELoss / JointsKLDLoss criteria; any other optimizer / criterion object raises instead of being ignored."""
import logging
import os
import time

import torch

from ... import executor as E
from ... import runtime as R
from ..utils.utils import FusedAdam, FusedAdamW, FusedSGD
from .evaluate import accuracy  # noqa: F401  (re-exported like the reference's core.function namespace)
from .loss import JointsKLDLoss, JointsMSELoss, JointsOHKMMSELoss

logger = logging.getLogger(__name__)


class AverageMeter(object):
    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count if self.count != 0 else 0


def _unwrap(m):
    return m.module if hasattr(m, 'module') else m


def _check_supported(optimizer, pose_criterion, kd_pose_criterion):
    """The fused step runs ITS Adam or SGD and ITS JointsMSELoss / JointsOHKMMSELoss: refuse objects it would otherwise
    silently ignore.  Returns the use_target_weight pair and the topk pair (None for a JointsMSELoss criterion; None instead
    of the pair when neither criterion mines).  With a JointsKLDLoss in either slot a third element follows: the temperature
    pair (None for a JointsMSELoss criterion); a KL criterion beside a mining one is refused."""
    if not isinstance(optimizer, (FusedAdam, FusedAdamW, FusedSGD)):
        raise R.FpdError('fpd_train: the fused MI355X step implements Adam, AdamW and SGD only (utils.get_optimizer with '
                         "TRAIN.OPTIMIZER 'adam' -> FusedAdam, 'adamw' -> FusedAdamW, 'sgd' -> FusedSGD); got %s -- its update rule and state "
                         'would be ignored' % type(optimizer).__name__)
    for name, c in (('pose_criterion', pose_criterion), ('kd_pose_criterion', kd_pose_criterion)):
        if not isinstance(c, (JointsMSELoss, JointsOHKMMSELoss, JointsKLDLoss)):
            raise R.FpdError('fpd_train: %s must be a core.loss.JointsMSELoss, core.loss.JointsOHKMMSELoss or core.loss.JointsKLDLoss '
                             '(the fused loss kernels evaluate exactly those criteria), got %s' % (name, type(c).__name__))
    topk = tuple(int(c.topk) if isinstance(c, JointsOHKMMSELoss) else None for c in (pose_criterion, kd_pose_criterion))
    kl = tuple(float(c.temperature) if isinstance(c, JointsKLDLoss) else None for c in (pose_criterion, kd_pose_criterion))
    use_w = (bool(pose_criterion.use_target_weight), bool(kd_pose_criterion.use_target_weight))
    if kl != (None, None):
        if topk != (None, None):
            raise R.FpdError('fpd_train: a JointsKLDLoss criterion cannot be paired with a JointsOHKMMSELoss (no fused kernel '
                             'evaluates that pair); use JointsMSELoss for the other criterion')
        if not all(t is None or 0.0 < t < float('inf') for t in kl):
            raise R.FpdError('fpd_train: JointsKLDLoss temperature must be positive, got %r' % (kl,))
        return use_w, None, kl
    return use_w, None if topk == (None, None) else topk


def fused_step_for(model, tmodel, optimizer, batch_shape, alpha, world_size=1, use_target_weight=(True, True), ohkm=None,
                   kl=None, ema=None, clip=None, accum=None):
    """One FusedFPDStep per (student, teacher, batch shape); shares the optimizer state with the FusedAdam / FusedSGD object.
    tmodel None = plain (non-distillation) training: no teacher graph, alpha must be 0.  ohkm: FusedFPDStep's topk pair;
    kl: its temperature pair.  ema: a utils.ModelEma of the student, averaged inside the step (its decay and warm-up live
    in the recorded plan op, so they are part of the key; the object is compared by identity like the optimizer).
    clip: a utils.GradClipper of the student (its max_norm lives in the recorded plan op, so it is part of the key; the object
    is compared by identity).  accum: FusedFPDStep's micro-batches per update; above 1 it adds plan ranges, so it is part of
    the key (None and 1 are the same step).
    A FusedSGD's (momentum, weight_decay, nesterov) live in the recorded plan op, so they are part of the key; so are a
    FusedAdamW's ('adamw', weight_decay, amsgrad, no_decay_norm_bias) and its betas and eps."""
    s, t = _unwrap(model), (_unwrap(tmodel) if tmodel is not None else None)
    # The cache lives ON the student module (not in a module-level dict keyed by id(): ids are recycled once an object
    # is collected, and a global would keep every plan and its arenas alive for the life of the process).  The teacher
    # and optimizer are compared by identity through the references the entry holds, so they cannot be recycled either.
    cache = s.__dict__.setdefault('_fused_steps', {})
    key = (tuple(batch_shape), float(alpha), world_size, tuple(use_target_weight)) + ((tuple(ohkm),) if ohkm is not None else ())
    if kl is not None:
        key += (('kl',) + tuple(kl),)
    key += getattr(optimizer, 'plan_key', tuple)()      # (an object that is none of the three keys and builds as a plain Adam did)
    if ema is not None:
        key += (('ema', float(ema.decay), bool(ema.warmup)),)
    if clip is not None:
        key += (('clip', float(clip.max_norm)),)
    if accum is not None and accum != 1:
        key += (('accum', accum),)
    hit = cache.get(key)
    if hit is not None and hit[0] is t and hit[1] is optimizer and hit[3] is ema and hit[4] is clip:
        return hit[2]
    n, _, h, w = batch_shape
    assert t is not None or alpha == 0.0
    step = E.FusedFPDStep(s.device_state(), s.cfg_hg, t.device_state() if t is not None else None,
                          t.cfg_hg if t is not None else None, n, h, w, alpha,
                          lr=float(optimizer.param_groups[0]['lr']), world_size=world_size,
                          use_target_weight=use_target_weight, ohkm=ohkm, kl=kl, ema=ema, clip=clip, accum=accum,
                          **{getattr(optimizer, 'keyword', 'adam'): optimizer})
    cache[key] = (t, optimizer, step, ema, clip)
    return step


DEBUG_WRITER_ASYNC = True      # tools/vis_bench.py measures the loops with the writer forced synchronous


def _debug_on(config):
    """DEBUG.DEBUG; a config object without the DEBUG node (callers that build only the keys the loops read) means off."""
    try:
        return bool(config.DEBUG.DEBUG)
    except (AttributeError, KeyError):
        return False


def _debug_writer(config, rank):
    """(utils.vis, writer) of one fpd_train / train / validate call when DEBUG.DEBUG asks rank 0 for debug images, else
    (None, None): with the flag off nothing of utils.vis is imported or touched.  The caller closes the writer before it
    returns, so the files exist by then."""
    if rank != 0 or not _debug_on(config):
        return None, None
    from ..utils import vis
    return vis, (vis.AsyncImageWriter() if DEBUG_WRITER_ASYNC else None)


def _on_device(t, dev):
    return t if t.is_cuda else t.to(dev, non_blocking=True)


def _run_epoch(config, train_loader, model, tmodel, crit, optimizer, epoch, writer_dict, allreduce, world_size, alpha,
               output_dir='', rank=0, ema=None, clip=None, accum=None):
    """The loop shared by fpd_train (function.py:99-187) and train (function.py:28-96; tmodel None, alpha 0)."""
    vis, img_writer = _debug_writer(config, rank)
    try:
        return _run_epoch_body(config, train_loader, model, tmodel, crit, optimizer, epoch, writer_dict, allreduce, world_size,
                               alpha, output_dir, vis, img_writer, ema, clip, accum)
    finally:
        if img_writer is not None:
            img_writer.close()


def _run_epoch_body(config, train_loader, model, tmodel, crit, optimizer, epoch, writer_dict, allreduce, world_size, alpha,
                    output_dir, vis, img_writer, ema=None, clip=None, accum=None):
    """accum > 1: one optimizer update per window of `accum` batches (FusedFPDStep._add_accum).  Both flush() calls below also
    close a partial window, so a window never spans batch shapes or epochs; meters and the `Epoch:` line stay per batch."""
    kd_mode = tmodel is not None
    use_w, ohkm, kl = crit if len(crit) == 3 else tuple(crit) + (None,)
    batch_time, data_time = AverageMeter(), AverageMeter()
    losses, pose_losses, kd_pose_losses, acc = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    model.train()          # function.py:110-111
    if kd_mode:
        tmodel.eval()
    step = metric = None
    end = time.time()
    it = iter(train_loader)
    nxt = next(it, None)
    i = -1
    n_img = 0
    updates = upd0 = 0         # optimizer updates of the steps this epoch has finished with / `step.updates` when it took `step`

    def drain():
        """Feed the meters with every iteration since the last drain (function.py:150-155); synchronises."""
        for avg_acc, cnt, pose, kd in metric.drain(full=True):
            pose_losses.update(pose, n_img); kd_pose_losses.update(kd, n_img)
            losses.update((1 - alpha) * pose + alpha * kd, n_img)
            acc.update(avg_acc, cnt)

    while nxt is not None:
        i += 1
        inp, target, target_weight, meta = nxt
        data_time.update(time.time() - end)
        if step is None or tuple(inp.shape) != tuple(step.student.image().shape):
            if step is not None:                       # batch shape changed (last, smaller batch): finish the old step
                step.flush()
                drain()
                updates += step.updates - upd0
            step = fused_step_for(model, tmodel, optimizer, inp.shape, alpha, world_size, use_w, ohkm, kl, ema, clip, accum)
            upd0 = step.updates
            metric = step.enable_metric(min_slots=config.PRINT_FREQ + 1)   # PCK + losses of every iteration, logged on the device
            metric.drain()
            n_img = inp.size(0)
            step.teacher_async(inp)                    # pipeline prologue: teacher forward of the first batch
        optimizer.sync_lr()
        step.set_batch(inp, target, target_weight)
        nxt = next(it, None)
        if nxt is not None and tuple(nxt[0].shape) == tuple(inp.shape):
            step.teacher_async(nxt[0])                 # teacher runs one batch ahead, overlapping this student step
        step.student_step(allreduce)
        if i % config.PRINT_FREQ == 0:
            if vis is not None:
                # function.py:94-96,185-187, enqueued behind the step: the student's last map is read where the forward left
                # it in the arena (the update does not touch it); the drain below is the wait these launches share
                dev = step.student.image().device
                vis.save_debug_images(config, _on_device(inp, dev), meta, _on_device(target, dev), None,
                                      step.student.output_view(-1).permute(0, 3, 1, 2),
                                      '{}_{}'.format(os.path.join(output_dir, 'train'), i), writer=img_writer)
            drain()                                    # the only host sync of the loop
            batch_time.update(time.time() - end)
            speed = inp.size(0) * world_size / max(batch_time.val, 1e-9)
            if kd_mode:
                msg = 'Epoch: [{0}][{1}/{2}]\t' \
                      'Time {batch_time.val:.3f}s ({batch_time.avg:.3f}s)\t' \
                      'Speed {speed:.1f} samples/s\t' \
                      'Data {data_time.val:.3f}s ({data_time.avg:.3f}s)\t' \
                      'POSE_Loss {pose_loss.val:.5f} ({pose_loss.avg:.5f})\t' \
                      'KD_POSE_Loss {kd_pose_loss.val:.5f} ({kd_pose_loss.avg:.5f})\t' \
                      'Loss {loss.val:.5f} ({loss.avg:.5f})\t' \
                      'Accuracy {acc.val:.3f} ({acc.avg:.3f})'.format(
                          epoch, i, len(train_loader), batch_time=batch_time, speed=speed, data_time=data_time,
                          pose_loss=pose_losses, kd_pose_loss=kd_pose_losses, loss=losses, acc=acc)
            else:
                msg = 'Epoch: [{0}][{1}/{2}]\t' \
                      'Time {batch_time.val:.3f}s ({batch_time.avg:.3f}s)\t' \
                      'Speed {speed:.1f} samples/s\t' \
                      'Data {data_time.val:.3f}s ({data_time.avg:.3f}s)\t' \
                      'Loss {loss.val:.5f} ({loss.avg:.5f})\t' \
                      'Accuracy {acc.val:.3f} ({acc.avg:.3f})'.format(
                          epoch, i, len(train_loader), batch_time=batch_time, speed=speed, data_time=data_time,
                          loss=losses, acc=acc)
            if clip is not None:               # read behind the drain above: the loop's only wait, none is added
                st = clip.stats()
                last_norm = clip.norm()
                msg += '\tGradNorm {last:.4f}  Clipped {clipped}/{calls}'.format(last=last_norm, clipped=st['clipped'], calls=st['calls'])
            if step.accum > 1:
                msg += '\tUpdates {0}'.format(updates + step.updates - upd0)
            logger.info(msg)
            if writer_dict is not None and writer_dict.get('writer') is not None:
                w, gs = writer_dict['writer'], writer_dict['train_global_steps']
                if kd_mode:
                    w.add_scalar('train_pose_loss', pose_losses.val, gs)
                    w.add_scalar('train_kd_pose_loss', kd_pose_losses.val, gs)
                w.add_scalar('train_loss', losses.val, gs)
                w.add_scalar('train_acc', acc.val, gs)
                if clip is not None:
                    w.add_scalar('train_grad_norm', last_norm, gs)
                writer_dict['train_global_steps'] = gs + 1
        else:
            batch_time.update(time.time() - end)
        end = time.time()
    if step is not None:
        step.flush()
        drain()
        updates += step.updates - upd0
    return {'loss': losses.avg, 'pose_loss': pose_losses.avg, 'kd_pose_loss': kd_pose_losses.avg, 'acc': acc.avg,
            'updates': updates,
            'iterations': losses.count // max(n_img, 1) if n_img else 0}


def fpd_train(config, train_loader, model, tmodel, pose_criterion, kd_pose_criterion, optimizer, epoch,
              output_dir, tb_log_dir, writer_dict, allreduce=None, world_size=1, rank=0, ema=None, clip=None, accum=None):
    """function.py:99-187 (same positional signature; allreduce / world_size / rank are the data-parallel extras: only
    rank 0 writes DEBUG images; ema: a utils.ModelEma of the student, updated inside every fused step; clip: a
    utils.GradClipper of the student, applied inside every fused step and reported in the `Epoch:` line; accum: batches per
    optimizer update, TRAIN.ACCUM_STEPS).  Returns the epoch's
    average loss (the reference returns None)."""
    crit = _check_supported(optimizer, pose_criterion, kd_pose_criterion)
    return _run_epoch(config, train_loader, model, tmodel, crit, optimizer, epoch, writer_dict, allreduce, world_size,
                      float(config.KD.ALPHA), output_dir, rank, ema, clip, accum)['loss']


def train(config, train_loader, model, criterion, optimizer, epoch, output_dir, tb_log_dir, writer_dict,
          allreduce=None, world_size=1, rank=0, ema=None, clip=None, accum=None):
    """function.py:28-96: plain (non-distillation) training = the same fused step without a teacher graph (alpha 0)."""
    crit = _check_supported(optimizer, criterion, criterion)
    return _run_epoch(config, train_loader, model, None, crit, optimizer, epoch, writer_dict, allreduce, world_size, 0.0,
                      output_dir, rank, ema, clip, accum)['loss']


def _to_numpy(v):
    import numpy as np
    return v.numpy() if torch.is_tensor(v) else np.asarray(v)


def _image_of(val_dataset, row):
    """Image path of dataset row `row` from the dataset's own records (host data every rank has)."""
    recs = getattr(val_dataset, 'db', None)
    if isinstance(recs, list):
        return recs[row]['image']
    names = getattr(val_dataset, 'all_names', None) or val_dataset.names
    return names[row]


def validate(config, val_loader, val_dataset, model, criterion, output_dir, tb_log_dir, writer_dict=None, gather=None, rank=0):
    """function.py:189-332 with the reference's signature and return value (the dataset's perf indicator); see
    _validate_body.  rank: only rank 0 writes DEBUG images (function.py:286-290), through a writer this call owns."""
    vis, img_writer = _debug_writer(config, rank)
    try:
        return _validate_body(config, val_loader, val_dataset, model, criterion, output_dir, writer_dict, gather, vis, img_writer)
    finally:
        if img_writer is not None:
            img_writer.close()


def _validate_body(config, val_loader, val_dataset, model, criterion, output_dir, writer_dict, gather, vis, img_writer):
    """The body of validate.

    Every batch is enqueued work only (executor.ValidateStep): the eval-mode forward, TEST.FLIP_TEST's second forward on
    the width-flipped batch, and one launch that merges the two maps, takes the arg-max with the TEST.POST_PROCESS
    quarter-pixel shift, computes every sample's inverse affine map and writes the batch's rows of the device-resident
    all_preds [num,J,3] / all_boxes [num,6] (with TEST.DARK one more launch, the DARK decode of the merged map, overwrites
    their x and y, and the quarter-pixel shift is off); JointsMSELoss and the PCK accuracy read the merged map and append to a device
    ring.  The host waits for the device when a `Test:` line is due (PRINT_FREQ) and once after the last batch, when the
    result arrays are downloaded.  A smaller last batch gets a step of its own shape.

    gather (None: this process validates everything its loader yields): a callable taking this rank's
    (all_preds, all_boxes, dataset rows, [sum loss*n, n, sum acc*cnt, cnt]) that returns every rank's four, each
    concatenated in rank order, on rank 0 and None elsewhere (dist.make_gather).  Rank 0 then places the rows, takes the
    image paths of the other ranks' rows from the dataset's own records and calls val_dataset.evaluate; the other ranks
    return the indicator rank 0 broadcasts (gather.broadcast, where the callable has one)."""
    import numpy as np

    from .inference import dark_config
    if type(criterion) is not JointsMSELoss:
        raise R.FpdError('validate: the fused validation step evaluates core.loss.JointsMSELoss, got %s' % type(criterion).__name__)
    net = _unwrap(model)
    if not hasattr(net, 'instance') or not hasattr(net, '_flat'):
        raise R.FpdError('validate: %s is not a HIP-backed model (lib.models)' % type(net).__name__)
    batch_time, losses, acc = AverageMeter(), AverageMeter(), AverageMeter()
    model.eval()
    dev = net._flat['param'].device
    num_samples, J = len(val_dataset), config.MODEL.NUM_JOINTS
    all_preds = torch.zeros((num_samples, J, 3), dtype=torch.float32, device=dev)
    all_boxes = torch.zeros((num_samples, 6), dtype=torch.float64, device=dev)
    flip_pairs = val_dataset.flip_pairs if config.TEST.FLIP_TEST else None
    image_path, filenames, imgnums, rows = [], [], [], []
    idx = 0
    step, n_img = None, {}
    pending = []                    # steps whose ring holds undrained entries, in order of first use

    def drain():
        """Feed the meters with every batch since the last drain; synchronises."""
        for s in pending:
            for avg_acc, cnt, loss, _ in s.metric.drain(full=True):
                losses.update(loss, n_img[id(s)])
                acc.update(avg_acc, cnt)
        del pending[:]

    with torch.no_grad():
        end = time.time()
        for i, (inp, target, target_weight, meta) in enumerate(val_loader):
            shape = tuple(inp.shape)
            if step is None or shape != tuple(step.inst.image().shape):
                step = E.validate_step_for(net, shape)
                if step in pending:                          # a shape that comes back: keep the entries in batch order
                    drain()
                if id(step) not in n_img:
                    step.begin(all_preds, all_boxes, flip_pairs, config.TEST.SHIFT_HEATMAP, config.TEST.POST_PROCESS,
                               criterion.use_target_weight, min_slots=config.PRINT_FREQ + 1, dark=dark_config(config))
                    n_img[id(step)] = shape[0]
            if idx + shape[0] > num_samples:
                raise R.FpdError('validate: the loader yields more than the %d samples of the dataset' % num_samples)
            step.run(inp, target, target_weight, meta['center'], meta['scale'], meta['score'], idx)
            if step not in pending:
                pending.append(step)
            image_path.extend(meta['image'])
            if gather is not None:
                rows.append(_to_numpy(meta['index']).astype(np.int64).reshape(-1))
            idx += shape[0]
            if i % config.PRINT_FREQ == 0:
                if vis is not None:                          # the loader's tensor: the instance's image may hold the flipped batch
                    vis.save_debug_images(config, _on_device(inp, dev), meta, _on_device(target, dev), None,
                                          step.merged.permute(0, 3, 1, 2), '{}_{}'.format(os.path.join(output_dir, 'val'), i),
                                          writer=img_writer)
                drain()                                      # the only host sync of the loop
                batch_time.update(time.time() - end)
                logger.info('Test: [{0}/{1}]\t'
                            'Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
                            'Loss {loss.val:.4f} ({loss.avg:.4f})\t'
                            'Accuracy {acc.val:.3f} ({acc.avg:.3f})'.format(i, len(val_loader), batch_time=batch_time,
                                                                             loss=losses, acc=acc))
            else:
                batch_time.update(time.time() - end)
            end = time.time()
        drain()
        all_preds, all_boxes = all_preds.cpu().numpy(), all_boxes.cpu().numpy()       # the one download
        loss_avg, acc_avg = losses.avg, acc.avg
        if gather is not None:
            rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
            got = gather(all_preds[:idx], all_boxes[:idx], rows, np.array([losses.sum, losses.count, acc.sum, acc.count], np.float64))
            if got is None:                                  # not rank 0: the indicator rank 0 broadcasts
                bc = getattr(gather, 'broadcast', None)
                return bc(None) if bc is not None else None
            g_preds, g_boxes, g_rows, sums = got
            g_rows = np.asarray(g_rows, np.int64)
            all_preds = np.zeros((num_samples, J, 3), dtype=np.float32)
            all_boxes = np.zeros((num_samples, 6))
            all_preds[g_rows], all_boxes[g_rows] = g_preds, g_boxes
            own = dict(zip(rows.tolist(), image_path))
            image_path = [own[r] if r in own else _image_of(val_dataset, r) for r in range(num_samples)]
            sums = np.asarray(sums, np.float64).reshape(-1, 4).sum(0)
            loss_avg = sums[0] / sums[1] if sums[1] else 0
            acc_avg = sums[2] / sums[3] if sums[3] else 0
        name_values, perf_indicator = val_dataset.evaluate(config, all_preds, output_dir, all_boxes, image_path,
                                                           filenames, imgnums)
        for nv in (name_values if isinstance(name_values, list) else [name_values]):
            _print_name_value(nv, config.MODEL.NAME)
        if writer_dict and writer_dict.get('writer') is not None:
            writer, gs = writer_dict['writer'], writer_dict['valid_global_steps']
            writer.add_scalar('valid_loss', loss_avg, gs)
            writer.add_scalar('valid_acc', acc_avg, gs)
            for nv in (name_values if isinstance(name_values, list) else [name_values]):
                writer.add_scalars('valid', dict(nv), gs)
            writer_dict['valid_global_steps'] = gs + 1
    validate.last = {'loss': loss_avg, 'acc': acc_avg, 'all_preds': all_preds, 'all_boxes': all_boxes, 'image_path': image_path}
    if gather is not None and getattr(gather, 'broadcast', None) is not None:
        return gather.broadcast(perf_indicator)
    return perf_indicator


def _validate_per_batch(config, val_loader, val_dataset, model, criterion, output_dir, tb_log_dir, writer_dict=None, rank=0):
    """The per-batch body `validate` had before the fused step, kept as the yardstick of tests/test_val_post_gpu.py and
    tools/validate_bench.py; nothing else calls it.

    Per batch: eval-mode forward (the folded-BN plan: fused frozen Bottlenecks / heads in bf16, the parity kernels in
    fp32), TEST.FLIP_TEST second forward on the width-flipped batch, flip_back + TEST.SHIFT_HEATMAP shift + average
    (one kernel), JointsMSELoss, PCK accuracy (csrc/pck.hip), and get_final_preds (arg-max, TEST.POST_PROCESS
    quarter-pixel shift, affine map to image coordinates: one kernel), with the per-sample matrices from a host loop and
    four host synchronisations: predictions, max values, loss and accuracy cross PCIe every batch."""
    import numpy as np

    from ..utils.transforms import flip_input, flip_merge, get_affine_transform
    from .evaluate import DeviceAccuracy
    from .inference import dark_config, final_preds_device
    batch_time, losses, acc = AverageMeter(), AverageMeter(), AverageMeter()
    model.eval()
    net = _unwrap(model)
    dev = net._flat['param'].device
    num_samples = len(val_dataset)
    all_preds = np.zeros((num_samples, config.MODEL.NUM_JOINTS, 3), dtype=np.float32)
    all_boxes = np.zeros((num_samples, 6))
    image_path, filenames, imgnums = [], [], []
    idx = 0
    metric = None
    with torch.no_grad():
        end = time.time()
        for i, (inp, target, target_weight, meta) in enumerate(val_loader):
            inp = inp.to(dev, non_blocking=True)
            outputs = model(inp)
            output = outputs[-1] if isinstance(outputs, list) else outputs
            if config.TEST.FLIP_TEST:
                outputs_flipped = model(flip_input(inp))
                output_flipped = outputs_flipped[-1] if isinstance(outputs_flipped, list) else outputs_flipped
                output = flip_merge(output, output_flipped, val_dataset.flip_pairs, config.TEST.SHIFT_HEATMAP)
            target = target.to(dev, non_blocking=True)
            target_weight = target_weight.to(dev, non_blocking=True)
            loss = criterion(output, target, target_weight)
            num_images = inp.size(0)
            n, j, h, w = output.shape
            # accuracy(output, target) on the device: NHWC copy of the merged map -> pck kernels -> log ring
            if metric is None or metric.args.B != n:
                metric = DeviceAccuracy(n, j, h, w, R.F32, dev, slots=16)
                nhwc = torch.empty((n, h, w, j), dtype=torch.float32, device=dev)
            R.check(R.lib().fpd_nchw_to_nhwc(output.data_ptr(), nhwc.data_ptr(), n, j, h, w, R.F32, R.current_stream()))
            tgt = target.float().contiguous()
            metric.bind(nhwc.data_ptr(), tgt.data_ptr()).enqueue()
            c, s = _to_numpy(meta['center']), _to_numpy(meta['scale'])
            score = _to_numpy(meta['score'])
            trans = np.stack([get_affine_transform(c[k], s[k], 0, [w, h], inv=1) for k in range(n)])
            _, preds, maxvals = final_preds_device(output, torch.from_numpy(trans).to(dev), config.TEST.POST_PROCESS,
                                                   dark_config(config))
            # the one synchronisation of the iteration: results + the two scalars
            preds, maxvals = preds.cpu().numpy(), maxvals.cpu().numpy()
            losses.update(loss.item(), num_images)
            (avg_acc, cnt), = metric.drain()
            acc.update(avg_acc, cnt)
            batch_time.update(time.time() - end)
            end = time.time()
            all_preds[idx:idx + num_images, :, 0:2] = preds[:, :, 0:2]
            all_preds[idx:idx + num_images, :, 2:3] = maxvals
            all_boxes[idx:idx + num_images, 0:2] = c[:, 0:2]
            all_boxes[idx:idx + num_images, 2:4] = s[:, 0:2]
            all_boxes[idx:idx + num_images, 4] = np.prod(s * 200, 1)
            all_boxes[idx:idx + num_images, 5] = score
            image_path.extend(meta['image'])
            idx += num_images
            if i % config.PRINT_FREQ == 0:
                if rank == 0 and _debug_on(config):          # function.py:286-290 (this yardstick waits every batch anyway)
                    from ..utils.vis import save_debug_images
                    save_debug_images(config, inp, meta, target, None, output, '{}_{}'.format(os.path.join(output_dir, 'val'), i))
                logger.info('Test: [{0}/{1}]\t'
                            'Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
                            'Loss {loss.val:.4f} ({loss.avg:.4f})\t'
                            'Accuracy {acc.val:.3f} ({acc.avg:.3f})'.format(i, len(val_loader), batch_time=batch_time,
                                                                             loss=losses, acc=acc))
        name_values, perf_indicator = val_dataset.evaluate(config, all_preds, output_dir, all_boxes, image_path,
                                                           filenames, imgnums)
        for nv in (name_values if isinstance(name_values, list) else [name_values]):
            _print_name_value(nv, config.MODEL.NAME)
        if writer_dict and writer_dict.get('writer') is not None:
            writer, gs = writer_dict['writer'], writer_dict['valid_global_steps']
            writer.add_scalar('valid_loss', losses.avg, gs)
            writer.add_scalar('valid_acc', acc.avg, gs)
            for nv in (name_values if isinstance(name_values, list) else [name_values]):
                writer.add_scalars('valid', dict(nv), gs)
            writer_dict['valid_global_steps'] = gs + 1
    _validate_per_batch.last = {'loss': losses.avg, 'acc': acc.avg, 'all_preds': all_preds, 'all_boxes': all_boxes,
                                'image_path': image_path}
    return perf_indicator


def _print_name_value(name_value, full_arch_name):
    """function.py:335-353: markdown table of the dataset's metrics."""
    names, values = list(name_value.keys()), list(name_value.values())
    logger.info('| Arch ' + ' '.join('| {}'.format(n) for n in names) + ' |')
    logger.info('|---' * (len(names) + 1) + '|')
    arch = full_arch_name if len(full_arch_name) <= 15 else full_arch_name[:8] + '...'
    logger.info('| ' + arch + ' ' + ' '.join('| {:.3f}'.format(v) for v in values) + ' |')
