#!/usr/bin/env python
"""FPD training entry point with the reference's command line (/root/reference/tools/fpd_train.py:44-83):

    python tools/fpd_train.py --cfg S.yaml --tcfg T.yaml [KEY VALUE ...]
    python -m torch.distributed.run --nproc-per-node 8 tools/fpd_train.py --cfg ... --tcfg ...      (data parallel)

Same flow as the reference's main() (:96-294): config merge, student `models.<NAME>.get_pose_net(cfg, is_train=True)`,
teacher from the cloned config merged with --tcfg, strict teacher-checkpoint load, two JointsMSELoss criteria,
Adam + MultiStepLR, epoch loop -> core.function.fpd_train -> checkpoint.  What differs: one process per GPU with an
RCCL gradient all-reduce instead of nn.DataParallel; the models run on the HIP path; DATASET.DATASET 'synthetic'
(the default) feeds seeded synthetic crops, DATASET.DATASET 'mpii' an MPII directory at DATASET.ROOT, decoded once and
resident on the device (lib/dataset/mpii.py), DATASET.DATASET 'coco' a COCO directory the same way, validated from
ground-truth or detection boxes with OKS NMS on the device and the keypoint AP table (lib/dataset/coco.py), DATASET.DATASET 'synthetic_aug' seeded
scenes that are augmented, cropped and labelled on the device per batch (DATASET.FLIP / SCALE_FACTOR / ROT_FACTOR /
PROB_HALF_BODY / NUM_JOINTS_HALF_BODY, LOSS.USE_DIFFERENT_JOINTS_WEIGHT; lib/dataset/device_dataset.py), and KD.TEACHER 'synthetic' builds a
random teacher with calibrated BN statistics instead of loading a checkpoint.  LOSS.USE_OHKM of the student config makes
the pose criterion a JointsOHKMMSELoss(topk=LOSS.TOPK), LOSS.USE_OHKM of the teacher config the distillation criterion
(make_criterion below); KD.LOSS 'kl' makes the distillation criterion a JointsKLDLoss(KD.TEMPERATURE) (make_kd_criterion);
the reference declares both keys and its tools never read them (its class is never instantiated).  TRAIN.EMA keeps an
exponential moving average of the student (utils.ModelEma, TRAIN.EMA_DECAY / EMA_WARMUP), updated inside the fused step:
the per-epoch validation, model_best.pth and final_state.pth then hold the average; checkpoint.pth keeps the raw weights
(what a resume continues from) and gains ema_state_dict / ema_updates.  TRAIN.CLIP_GRAD_NORM (0 = off, .inf = measure only)
clips the gradient of every update to that global L2 norm inside the fused step (utils.GradClipper) and adds `GradNorm` /
`Clipped` to the `Epoch:` line.  TRAIN.ACCUM_STEPS k > 1 makes one optimizer update per k batches, their gradients averaged
inside the fused step (each batch keeps its own BatchNorm statistics, as a DataParallel replica would); a window never spans
epochs, and the `Epoch:` line gains `Updates`.
"""
import argparse
import logging
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '6' if int(os.environ.get('WORLD_SIZE', '1')) > 1 else '8')      # before torch loads the HIP runtime; see bench.py / DESIGN.md section 4

import torch  # noqa: E402
import torch.utils.data  # noqa: E402

from fpd_amd import dist as fdist, executor as E, synth  # noqa: E402
from fpd_amd.lib import models  # noqa: E402,F401
from fpd_amd.lib.config import cfg, update_config  # noqa: E402
from fpd_amd.lib.core.function import fpd_train, train, validate  # noqa: E402
from fpd_amd.lib.dataset import SyntheticPose, coco, mpii, synthetic_aug  # noqa: E402
from fpd_amd.lib.dataset.device_pipeline import unbiased_targets  # noqa: E402
from fpd_amd.lib.dataset.device_dataset import block_range  # noqa: E402
from fpd_amd.lib.core.loss import JointsKLDLoss, JointsMSELoss, JointsOHKMMSELoss  # noqa: E402
from fpd_amd.lib.utils.utils import (ModelEma, get_accum_steps, get_grad_clipper, get_model_summary, get_optimizer, load_checkpoint,  # noqa: E402
                                     multistep_lr, save_checkpoint)


def parse_args(description='Train keypoints network (FPD)', with_teacher=True):
    p = argparse.ArgumentParser(description=description)
    p.add_argument('--cfg', help='%sexperiment configure file name' % ('student ' if with_teacher else ''), required=True, type=str)
    if with_teacher:
        p.add_argument('--tcfg', help='teacher experiment configure file name', default='', type=str)
    p.add_argument('opts', help='Modify config options using the command-line', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--modelDir', default='', type=str)
    p.add_argument('--logDir', default='', type=str)
    p.add_argument('--dataDir', default='', type=str)
    p.add_argument('--max-iters', type=int, default=0, help='stop every epoch after this many iterations (smoke runs)')
    return p.parse_args()


def get_train_type(train_type, checkpoint):
    """tools/fpd_train.py:85-94."""
    if train_type == 'NORMAL':
        return train_type
    if train_type == 'FPD' and (checkpoint == 'synthetic' or (checkpoint and os.path.exists(checkpoint))):
        return 'FPD'
    if train_type == 'FPD':
        sys.exit('ERROR: teacher checkpoint is not existed.')
    sys.exit('ERROR: please change train type {} to NORMAL or FPD.'.format(train_type))


def make_criterion(c):
    """The criterion config `c` asks for: LOSS.USE_OHKM -> JointsOHKMMSELoss(use_target_weight, topk=LOSS.TOPK), else
    JointsMSELoss(use_target_weight) (:145-147,177-179).  The reference's tools never instantiate its JointsOHKMMSELoss."""
    if c.LOSS.USE_OHKM:
        return JointsOHKMMSELoss(use_target_weight=c.LOSS.USE_TARGET_WEIGHT, topk=c.LOSS.TOPK)
    return JointsMSELoss(use_target_weight=c.LOSS.USE_TARGET_WEIGHT)


def make_kd_criterion(c, tc):
    """The distillation criterion: KD.LOSS 'mse' (the default) -> make_criterion(teacher config) as before; 'kl' ->
    JointsKLDLoss(teacher config's LOSS.USE_TARGET_WEIGHT, KD.TEMPERATURE), the soft-label KL over the spatial softmax of
    the teacher's heat maps (:175 "you can choose or replace pose_loss and kd_pose_loss type").  No fused kernel pairs a
    KL term with hard-keypoint mining, so 'kl' beside LOSS.USE_OHKM of either config ends the run here."""
    kind = str(c.KD.LOSS).lower()
    if kind == 'mse':
        return make_criterion(tc)
    if kind != 'kl':
        sys.exit("ERROR: KD.LOSS %r: choose 'mse' or 'kl'." % (c.KD.LOSS,))
    if tc.LOSS.USE_OHKM or c.LOSS.USE_OHKM:
        sys.exit("ERROR: KD.LOSS 'kl' cannot be combined with LOSS.USE_OHKM (%s config): the fused loss pairs a KL term "
                 'with a plain MSE term only.' % ('teacher' if tc.LOSS.USE_OHKM else 'student'))
    if not float(c.KD.TEMPERATURE) > 0.0:
        sys.exit('ERROR: KD.TEMPERATURE must be positive, got %r.' % (c.KD.TEMPERATURE,))
    return JointsKLDLoss(use_target_weight=tc.LOSS.USE_TARGET_WEIGHT, temperature=float(c.KD.TEMPERATURE))


def run(args, normal=False):
    """The training run both entry points share.  normal: tools/train.py -- plain training whatever KD.TRAIN_TYPE says, no
    teacher config (`args` has no tcfg)."""
    update_config(cfg, args)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    logging.basicConfig(level=logging.INFO if rank == 0 else logging.WARNING, format='%(asctime)-15s %(message)s')
    logger = logging.getLogger()
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
    train_type = 'NORMAL' if normal else get_train_type(cfg.KD.TRAIN_TYPE, cfg.KD.TEACHER)
    out_dir = os.path.join(cfg.OUTPUT_DIR, cfg.DATASET.DATASET, cfg.MODEL.NAME,
                           os.path.basename(args.cfg).split('.')[0])
    os.makedirs(out_dir, exist_ok=True)

    torch.manual_seed(1)
    model = eval('models.' + cfg.MODEL.NAME + '.get_pose_net')(cfg, is_train=True)          # :122-124
    tcfg = cfg.clone()                                                                        # :128-131
    if getattr(args, 'tcfg', ''):
        tcfg.merge_from_file(args.tcfg)
    if rank == 0:                                                                             # :162-167 (shape-only walk)
        logger.info(get_model_summary(model, torch.empty(1, 3, cfg.MODEL.IMAGE_SIZE[1], cfg.MODEL.IMAGE_SIZE[0], device='meta')))
    tmodel = None
    if train_type == 'FPD':
        torch.manual_seed(2)
        tmodel = eval('models.' + tcfg.MODEL.NAME + '.get_pose_net')(tcfg, is_train=False)   # :135-137
        if cfg.KD.TEACHER != 'synthetic':
            load_checkpoint(cfg.KD.TEACHER, tmodel, strict=True, model_info='teacher_' + tcfg.MODEL.NAME)   # :139-141
        tmodel = fdist.DataParallelReplica(tmodel.to(dev))
    if cfg.TRAIN.CHECKPOINT:
        load_checkpoint(cfg.TRAIN.CHECKPOINT, model, strict=True, model_info='student_' + cfg.MODEL.NAME)
    model = fdist.DataParallelReplica(model.to(dev))
    if world > 1:
        fdist.broadcast_state(dist, model.module)
        if tmodel is not None:
            fdist.broadcast_state(dist, tmodel.module)

    pose_criterion = make_criterion(cfg).to(dev)                                             # :145-147,177-179
    kd_pose_criterion = make_criterion(tcfg).to(dev)
    if not normal:                                                                           # KD.LOSS: 'mse' leaves it as it is
        kd_pose_criterion = make_kd_criterion(cfg, tcfg).to(dev)
    if isinstance(kd_pose_criterion, JointsKLDLoss):
        logger.info('=> distillation criterion: spatial-softmax KL, temperature %g', kd_pose_criterion.temperature)
    val_criterion = JointsMSELoss(use_target_weight=cfg.LOSS.USE_TARGET_WEIGHT).to(dev)      # the validation loss stays plain MSE
    if cfg.LOSS.USE_OHKM or tcfg.LOSS.USE_OHKM:
        logger.info('=> hard keypoint mining: pose criterion %s, distillation criterion %s',
                    'topk %d' % cfg.LOSS.TOPK if cfg.LOSS.USE_OHKM else 'MSE', 'topk %d' % tcfg.LOSS.TOPK if tcfg.LOSS.USE_OHKM else 'MSE')

    if cfg.DATASET.DATASET not in ('synthetic', 'synthetic_aug', 'mpii', 'coco'):
        sys.exit('dataset %r is not available here; use DATASET.DATASET synthetic, synthetic_aug, mpii or coco' % cfg.DATASET.DATASET)
    bs = cfg.TRAIN.BATCH_SIZE_PER_GPU
    if unbiased_targets(cfg):                            # read by the device loaders below, train and validation; `synthetic` raises
        logger.info('=> targets: MODEL.TARGET_TYPE gaussian_unbiased (Gaussians at the real-valued joint positions)')
    if cfg.DATASET.DATASET == 'mpii':
        # DATASET.ROOT decoded once and resident on every rank's device; each rank augments its rank::world share of the
        # epoch's permutation (lib/dataset/mpii.py); every rank holds and validates its block of the validation set
        loader, valid_loader, valid_set = mpii(cfg, dev, rank, world)
    elif cfg.DATASET.DATASET == 'coco':                  # the same for a COCO directory (lib/dataset/coco.py)
        loader, valid_loader, valid_set = coco(cfg, dev, rank, world)
    elif cfg.DATASET.DATASET == 'synthetic_aug':
        # seeded scenes resident on the device; every batch is augmented there (half-body, scale / rotation jitter, flip),
        # cropped and given its targets by three kernels (lib/dataset/device_dataset.py)
        loader, valid_loader, valid_set = synthetic_aug(cfg, dev, rank, world_size=world)
    else:
        train_set = SyntheticPose(cfg, cfg.DATASET.NUM_SAMPLES, seed=rank)
        loader = torch.utils.data.DataLoader(train_set, batch_size=bs, shuffle=cfg.TRAIN.SHUFFLE, num_workers=0,
                                             pin_memory=cfg.PIN_MEMORY, drop_last=True, collate_fn=train_set.collate)
        valid_set = SyntheticPose(cfg, cfg.DATASET.NUM_VALID_SAMPLES, seed=1009)
        valid_loader = torch.utils.data.DataLoader(valid_set, batch_size=cfg.TEST.BATCH_SIZE_PER_GPU, num_workers=0,
                                                   sampler=range(*block_range(len(valid_set), rank, world)),
                                                   pin_memory=cfg.PIN_MEMORY, collate_fn=valid_set.collate)
    if args.max_iters:
        import itertools
        full = loader

        class _Limited(object):
            def __iter__(self):
                return itertools.islice(iter(full), args.max_iters)

            def __len__(self):
                return min(len(full), args.max_iters)
        loader = _Limited()
    if tmodel is not None and cfg.KD.TEACHER == 'synthetic':          # give the random teacher sane eval-mode BN statistics once
        x0 = next(iter(loader))[0]
        t = tmodel.module
        cal = E.GraphInstance(t.device_state(), t.cfg_hg, x0.shape[0], x0.shape[2], x0.shape[3], train=True).finalize()
        cal.image().copy_(x0)
        cal.run('prep'); cal.run('fwd')
        cal.calibrate_running_stats()
        del cal

    optimizer = get_optimizer(cfg, model)                                                     # :218
    ema = ModelEma(model, decay=float(cfg.TRAIN.EMA_DECAY), warmup=bool(cfg.TRAIN.EMA_WARMUP)) if cfg.TRAIN.EMA else None
    clip = get_grad_clipper(cfg, model)                    # TRAIN.CLIP_GRAD_NORM: None when 0; a negative value raises
    if clip is not None:
        logger.info('=> gradient clipping: global L2 norm %g', clip.max_norm)
    accum = get_accum_steps(cfg)                           # TRAIN.ACCUM_STEPS: batches per optimizer update; below 1 raises
    if accum > 1:
        logger.info('=> gradient accumulation: %d micro-batches of %d per update, effective batch %d', accum, bs * world,
                    accum * bs * world)
    begin_epoch, best_perf = cfg.TRAIN.BEGIN_EPOCH, 0.0
    ckpt = os.path.join(out_dir, 'checkpoint.pth')
    if cfg.AUTO_RESUME and os.path.exists(ckpt):                                              # :224-234
        state = torch.load(ckpt, map_location=dev)
        begin_epoch, best_perf = state['epoch'], state['perf']
        model.load_state_dict(state['state_dict'])
        optimizer.load_state_dict(state['optimizer'])
        logger.info("=> loaded checkpoint '%s' (epoch %d)", ckpt, state['epoch'])
        if ema is not None and 'ema_state_dict' in state:
            ema.load_state_dict({'state_dict': state['ema_state_dict'], 'updates': state.get('ema_updates', 0)})
        elif ema is not None:
            logger.warning('=> checkpoint %s has no ema_state_dict: the average restarts from the resumed weights', ckpt)
            ema.set(model)
    base_lr = float(optimizer.param_groups[0].get('initial_lr', cfg.TRAIN.LR))               # :236-239 MultiStepLR
    optimizer.param_groups[0]['initial_lr'] = base_lr
    allreduce = fdist.make_allreduce(dist) if world > 1 else None
    writer_dict = {'writer': None, 'train_global_steps': 0, 'valid_global_steps': 0}
    # :243-250: before the first epoch the reference evaluates the teacher and then the student on the validation set (the
    # two "Test:" blocks in front of epoch 0 in its logs).  Both go through core.function.validate on EVERY rank, each over
    # its block of the set (the reference validates on its DataParallel model, :143,244); rank 0 gathers and evaluates.
    gather = fdist.make_gather(dist) if world > 1 else None
    if tmodel is not None:
        validate(cfg, valid_loader, valid_set, tmodel, val_criterion, out_dir, cfg.LOG_DIR, writer_dict, gather=gather, rank=rank)
    validate(cfg, valid_loader, valid_set, model, val_criterion, out_dir, cfg.LOG_DIR, writer_dict, gather=gather, rank=rank)
    for epoch in range(begin_epoch, cfg.TRAIN.END_EPOCH):                                     # :252-286
        t0 = time.time()
        optimizer.param_groups[0]['lr'] = multistep_lr(base_lr, cfg.TRAIN.LR_STEP, cfg.TRAIN.LR_FACTOR, epoch)   # :253
        if train_type == 'FPD':                                                               # :255-264
            loss = fpd_train(cfg, loader, model, tmodel, pose_criterion, kd_pose_criterion, optimizer, epoch, out_dir,
                             cfg.LOG_DIR, writer_dict, allreduce=allreduce, world_size=world, rank=rank, ema=ema, clip=clip,
                             accum=accum)
        else:
            loss = train(cfg, loader, model, pose_criterion, optimizer, epoch, out_dir, cfg.LOG_DIR, writer_dict,
                         allreduce=allreduce, world_size=world, rank=rank, ema=ema, clip=clip, accum=accum)
        torch.cuda.synchronize()
        logger.info('=> epoch %d done in %.1fs, %.1f samples/s, last logged loss %.5f', epoch, time.time() - t0,
                    len(loader) * bs * world / max(time.time() - t0, 1e-9), loss)
        # :266-285: evaluate on the validation set (flip test etc. per cfg.TEST) on every rank, keep the best model on rank 0
        # float(): MPII's indicator is a numpy scalar, which a weights-only torch.load of the checkpoint refuses
        # TRAIN.EMA: the averaged weights are what is evaluated and kept as the best model
        eval_model = ema.module if ema is not None else model
        perf_indicator = float(validate(cfg, valid_loader, valid_set, eval_model, val_criterion, out_dir, cfg.LOG_DIR, writer_dict,
                                        gather=gather, rank=rank))
        if rank == 0:
            best_model = perf_indicator >= best_perf
            best_perf = max(best_perf, perf_indicator)
            states = {'epoch': epoch + 1, 'model': cfg.MODEL.NAME, 'state_dict': model.state_dict(),
                      'best_state_dict': model.module.state_dict(), 'perf': perf_indicator,
                      'optimizer': optimizer.state_dict()}
            if ema is not None:
                e = ema.state_dict()
                states.update(best_state_dict=e['state_dict'], ema_state_dict=e['state_dict'], ema_updates=e['updates'])
            save_checkpoint(states, best_model, out_dir)
        if world > 1:
            dist.barrier()       # ranks != 0 wait for rank 0's checkpoint HERE, explicitly, rather than inside the first
                                 # gradient all-reduce of the next epoch
    if rank == 0:
        torch.save((ema.module if ema is not None else model.module).state_dict(), os.path.join(out_dir, 'final_state.pth'))      # :288-294
    if world > 1:
        dist.destroy_process_group()


def main():
    run(parse_args())


if __name__ == '__main__':
    main()
