#!/usr/bin/env python
"""Validation entry point with the reference's command line (/root/reference/tools/test.py:38-135):

    python tools/test.py --cfg S.yaml [TEST.MODEL_FILE model.pth] [KEY VALUE ...]

Same flow as the reference's main(): config merge, `models.<NAME>.get_pose_net(cfg, is_train=False)`, weights from
TEST.MODEL_FILE (strict=False like the reference, :88-90) or <output dir>/final_state.pth (:91-96), JointsMSELoss,
validation loader, `core.function.validate` (flip test / heat-map shift / post-processing per cfg.TEST).  What differs: the
model runs on the HIP path, on one GPU or, under `python -m torch.distributed.run --nproc_per_node=N tools/test.py ...`, on N
(every rank validates its block of the set, rank 0 gathers and evaluates); DATASET.DATASET 'synthetic' feeds the seeded synthetic validation set of
tools/fpd_train.py ('synthetic_aug': its validation scenes, cropped on the device), 'mpii' DATASET.ROOT / TEST_SET with the
PCKh table, 'coco' DATASET.ROOT / TEST_SET from ground-truth or detection boxes (TEST.USE_GT_BBOX, TEST.COCO_BBOX_FILE) with the
keypoint AP table.  TEST.USE_EMA true evaluates the averaged weights (ema_state_dict) of a full checkpoint.pth written by a
TRAIN.EMA run and given as TEST.MODEL_FILE; a file without them is an error."""
import argparse
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import torch  # noqa: E402
import torch.utils.data  # noqa: E402

from fpd_amd import dist as fdist  # noqa: E402
from fpd_amd.lib import models  # noqa: E402,F401
from fpd_amd.lib.config import cfg, update_config  # noqa: E402
from fpd_amd.lib.core.function import validate  # noqa: E402
from fpd_amd.lib.core.loss import JointsMSELoss  # noqa: E402
from fpd_amd.lib.dataset import SyntheticPose, coco, mpii, synthetic_aug  # noqa: E402
from fpd_amd.lib.dataset.device_pipeline import unbiased_targets  # noqa: E402
from fpd_amd.lib.dataset.device_dataset import block_range  # noqa: E402
from fpd_amd.lib.utils.utils import load_checkpoint  # noqa: E402


def parse_args():
    p = argparse.ArgumentParser(description='Test keypoints network')
    p.add_argument('--cfg', help='experiment configure file name', required=True, type=str)
    p.add_argument('opts', help='Modify config options using the command-line', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--modelDir', default='', type=str)
    p.add_argument('--logDir', default='', type=str)
    p.add_argument('--dataDir', default='', type=str)
    return p.parse_args()


def main():
    args = parse_args()
    update_config(cfg, args)
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    logging.basicConfig(level=logging.INFO if rank == 0 else logging.WARNING, format='%(asctime)-15s %(message)s')
    logger = logging.getLogger()
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    gather = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
        gather = fdist.make_gather(dist)
    out_dir = os.path.join(cfg.OUTPUT_DIR, cfg.DATASET.DATASET, cfg.MODEL.NAME, os.path.basename(args.cfg).split('.')[0])
    os.makedirs(out_dir, exist_ok=True)

    torch.manual_seed(1)
    model = eval('models.' + cfg.MODEL.NAME + '.get_pose_net')(cfg, is_train=False)          # :84-86
    model_file = cfg.TEST.MODEL_FILE or os.path.join(out_dir, 'final_state.pth')              # :88-96
    logger.info('=> loading model from %s', model_file)
    if cfg.TEST.USE_EMA:
        state = torch.load(model_file, map_location='cpu')
        if not isinstance(state, dict) or not isinstance(state.get('ema_state_dict'), dict):
            raise ValueError('TEST.USE_EMA: %s holds no ema_state_dict (give the checkpoint.pth of a TRAIN.EMA run as '
                             'TEST.MODEL_FILE)' % model_file)
        logger.info('=> evaluating the averaged weights (%d updates)', int(state.get('ema_updates', 0)))
        load_checkpoint(state['ema_state_dict'], model, strict=True, model_info=cfg.MODEL.NAME)
    else:
        load_checkpoint(model_file, model, strict=not cfg.TEST.MODEL_FILE, model_info=cfg.MODEL.NAME)
    model = fdist.DataParallelReplica(model.to(dev))
    criterion = JointsMSELoss(use_target_weight=cfg.LOSS.USE_TARGET_WEIGHT).to(dev)          # :101-103

    if cfg.DATASET.DATASET not in ('synthetic', 'synthetic_aug', 'mpii', 'coco'):
        sys.exit('dataset %r is not available here; use DATASET.DATASET synthetic, synthetic_aug, mpii or coco' % cfg.DATASET.DATASET)
    if unbiased_targets(cfg):                            # the validation loss is then taken against the unbiased targets; `synthetic` raises
        logger.info('=> targets: MODEL.TARGET_TYPE gaussian_unbiased (Gaussians at the real-valued joint positions)')
    if cfg.DATASET.DATASET == 'mpii':                    # DATASET.ROOT / TEST_SET, resident on the device; PCKh
        _, valid_loader, valid_set = mpii(cfg, dev, rank, world, train=False)
    elif cfg.DATASET.DATASET == 'coco':                  # DATASET.ROOT / TEST_SET; OKS NMS on the device, keypoint AP
        _, valid_loader, valid_set = coco(cfg, dev, rank, world, train=False)
    elif cfg.DATASET.DATASET == 'synthetic_aug':          # the validation scenes of tools/fpd_train.py, cropped on the device
        _, valid_loader, valid_set = synthetic_aug(cfg, dev, rank, train=False, world_size=world)
    else:
        valid_set = SyntheticPose(cfg, cfg.DATASET.NUM_VALID_SAMPLES, seed=1009)
        valid_loader = torch.utils.data.DataLoader(valid_set, batch_size=cfg.TEST.BATCH_SIZE_PER_GPU, num_workers=0,
                                                   sampler=range(*block_range(len(valid_set), rank, world)), pin_memory=cfg.PIN_MEMORY, collate_fn=valid_set.collate)
    perf = validate(cfg, valid_loader, valid_set, model, criterion, out_dir, cfg.LOG_DIR, gather=gather, rank=rank)    # :130-132
    if rank == 0:
        logger.info('=> validation done: perf indicator %.4f, loss %.5f, accuracy %.4f', perf, validate.last['loss'], validate.last['acc'])
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
