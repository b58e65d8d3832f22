#!/usr/bin/env python
"""Plain (non-distillation) training entry point with the reference's command line (tools/train.py:40-73 there):

    python tools/train.py --cfg X.yaml [--max-iters N] [KEY VALUE ...]
    python -m torch.distributed.run --nproc-per-node 8 tools/train.py --cfg ...      (data parallel)

Same flow as the reference's main() (:99-236): config merge, `models.<NAME>.get_pose_net(cfg, is_train=True)`, the criterion
the config asks for, utils.get_optimizer (TRAIN.OPTIMIZER adam | sgd with TRAIN.MOMENTUM / WD / NESTEROV | adamw with TRAIN.WD / AMSGRAD / NO_DECAY_NORM_BIAS), AUTO_RESUME,
MultiStepLR, per epoch core.function.train + validate, checkpoints, final_state.pth; TRAIN.EMA, TRAIN.CLIP_GRAD_NORM and
TRAIN.ACCUM_STEPS as there.  It is tools/fpd_train.py's run with the
NORMAL branch forced and no teacher config: one loop, two command lines.
"""
import fpd_train


def main():
    fpd_train.run(fpd_train.parse_args('Train keypoints network', with_teacher=False), normal=True)


if __name__ == '__main__':
    main()
