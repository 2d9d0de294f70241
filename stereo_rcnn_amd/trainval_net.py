"""Train Stereo R-CNN on KITTI: the reference's trainval_net.py on this project's pieces.

    python -m stereo_rcnn_amd.trainval_net --kitti-path data/kitti --split data/kitti/splits/train.txt [--epochs 20 --bs 1 ...]

datasets.kitti.build_roidb (annotations, flipped copies, filter, ratio ranking) -> data.TrainLoader (PNG decode in worker
processes, batch assembly in csrc/loader.hip) -> training.train_step per batch (forward_train, multi-task loss, backward, clipped
SGD step) with training.make_optimizer's groups and the six log-variances `uncert` initialised to -1 (trainval_net.py:155-156);
net_utils.adjust_learning_rate at the decay epochs (:189-191), net_utils.save_checkpoint at each epoch's end (:248-254: 'epoch' is
the NEXT epoch, 'model', 'optimizer', 'uncert').  Losses are read to the host only every --disp_interval iterations; in between
nothing waits for the device.  --resume loads model, optimiser state and uncert back and continues at the stored epoch.
--val-split FILE --val-label-dir DIR [--val-every N] [--val-precision f16x3|f32] (an extension: the reference has none): after
every N-th epoch the model's inference weights are refreshed in place (plan.Plan.refresh), the split runs through the inference
pipeline and kitti_eval, <save_dir>/ap_epoch<E>.json is written and the Car Moderate line logged (validation.py); training itself
is bit-identical with and without it.
--backward-precision f32|f16x3 (default f32; logged in trainlog.txt): the engine of the convolution gradients
(training.train_step's backward_precision).
--forward-precision f32|f16x3 (default f32; logged in trainlog.txt only when it is not the default): the engine of the forward of
every convolution / linear layer that has a graph (training.train_step's forward_precision; srcnn_conv2d_forward_f16x3).
--no-reuse-maxima: with an f16x3 precision, every call finds max |x| of its input itself (training.train_step's
reuse_maxima=False); by default each activation's maximum is found once and handed on.  The results are bit-identical.
Either precision also takes `auto`: autograd.choose_engine picks f32 or f16x3 per layer and direction from the layer's GEMM size.
--prepared-weights (logged in trainlog.txt only when set): max |w| and the f16x3 planes of every layer's weight are prepared once
at the start of each step, in one call (training.train_step's prepared_weights=True); the f16x3 calls then launch no pass over
a weight.  The results are bit-identical.
--device-fold (implies --prepared-weights; logged in trainlog.txt only when set): the frozen-BN fold and the re-layout of every
weight, and their adjoint, run on the device in one call each (training.train_step's device_fold=True; csrc/train_fold.hip) in
place of the per-layer torch operators.  The results are bit-identical.
--accum N (default 1; logged in trainlog.txt only when set): N consecutive loader batches form one step -- N forwards and
backwards summing their gradients, one update with their mean (training.train_step's accum_steps=N); iterations count steps, and
a trailing group of fewer than N batches at an epoch's end is not trained on.  The way to a larger effective batch at --bs 1:
no image is padded.
--guard (default off; logged in trainlog.txt only when set): the update is skipped, on the device, where a gradient is not finite
(training.train_step's guard=True; csrc/optim.hip): one Inf or NaN costs one step and not the run.  The count of skipped steps is
read and logged with the losses every --disp_interval iterations, and nowhere else.

The model starts from the reference's random initialisation (_init_weights) unless --init names a state dict (an ImageNet-
initialised or earlier Stereo R-CNN checkpoint): the reference's `pretrained=True` reads a caffe ResNet file this project does not ship.
"""
import argparse
import os
import sys
import time

import torch

PRE_NMS_ADVICE = ("cfg.TRAIN.RPN_PRE_NMS_TOP_N = %d: the proposal kernel ranks at most %d candidates, so on full-size images "
                  "forward_train refuses it.  Lower it to %d (--pre_nms_top_n %d), as the README's training paragraph says.")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Train the Stereo R-CNN network')
    p.add_argument('--kitti-path', dest='kitti_path', required=True, help='KITTI object root (holds training/image_2, image_3, label_2, calib)')
    p.add_argument('--split', required=True, help='split file: one frame id per line')
    p.add_argument('--start_epoch', default=1, type=int)
    p.add_argument('--epochs', dest='max_epochs', default=20, type=int)
    p.add_argument('--save_dir', default='models_stereo')
    p.add_argument('--nw', dest='num_workers', default=4, type=int, help='PNG decode processes (0: decode in-process)')
    p.add_argument('--prefetch', default=2, type=int)
    p.add_argument('--bs', dest='batch_size', default=1, type=int)
    p.add_argument('--lr', default=None, type=float, help='default: cfg.TRAIN.LEARNING_RATE')
    p.add_argument('--lr_decay_step', default=5, type=int, help='unit: epoch')
    p.add_argument('--lr_decay_gamma', default=0.1, type=float)
    p.add_argument('--disp_interval', default=100, type=int)
    p.add_argument('--net', default=101, type=int, help='ResNet depth')
    p.add_argument('--init', default=None, help='state dict (or checkpoint with a "model" entry) to start from')
    p.add_argument('--resume', default=None, help='checkpoint written by an earlier run')
    p.add_argument('--pre_nms_top_n', default=None, type=int, help='sets cfg.TRAIN.RPN_PRE_NMS_TOP_N')
    p.add_argument('--no_flip', action='store_true', help='do not append the flipped copies (cfg.TRAIN.USE_FLIPPED)')
    p.add_argument('--seed', default=None, type=int, help='default: cfg.RNG_SEED')
    p.add_argument('--val-split', dest='val_split', default=None,
                   help='validate on this split (one frame id per line, frames under <kitti-path>/training) after every --val-every-th '
                        'epoch: <save_dir>/ap_epoch<E>.json and a Car Moderate line in trainlog.txt')
    p.add_argument('--val-label-dir', dest='val_label_dir', default=None, help='KITTI label_2 directory of the validation frames')
    p.add_argument('--val-every', dest='val_every', default=1, type=int, help='unit: epoch')
    p.add_argument('--val-precision', dest='val_precision', choices=['f16x3', 'f32'], default='f16x3')
    p.add_argument('--backward-precision', dest='backward_precision', choices=['f32', 'f16x3', 'auto'], default='f32',
                   help='engine of the convolution gradients: the exact fp32 backward, or the 3 x f16 split (independent of --forward-precision)')
    p.add_argument('--forward-precision', dest='forward_precision', choices=['f32', 'f16x3', 'auto'], default='f32',
                   help='engine of the training forward of the layers that have a graph: the exact fp32 engine, or the 3 x f16 split '
                        'with scales found on the device')
    p.add_argument('--prepared-weights', dest='prepared_weights', action='store_true',
                   help="prepare max |w| and the f16x3 planes of every layer's weight once per step, in one call, instead of inside "
                        "every f16x3 convolution call (bit-identical results)")
    p.add_argument('--device-fold', dest='device_fold', action='store_true',
                   help="fold the frozen BNs and re-lay-out every weight on the device, one call per direction, in place of the "
                        "per-layer torch operators (implies --prepared-weights; bit-identical results)")
    p.add_argument('--no-reuse-maxima', dest='reuse_maxima', action='store_false',
                   help="f16x3 precisions only: let every convolution call scan its input for max |x| itself instead of taking it from "
                        "the call that produced the tensor (same bits either way)")
    p.add_argument('--accum', dest='accum', default=1, type=int,
                   help='loader batches per optimiser step: their gradients are summed on the device and the update uses the mean')
    p.add_argument('--guard', dest='guard', action='store_true',
                   help='skip the update, on the device, of a step whose gradients are not all finite; the count is logged with the losses')
    args = p.parse_args(argv)
    if args.accum < 1:
        p.error('--accum must be >= 1')
    args.prepared_weights = args.prepared_weights or args.device_fold
    return args


def _groups(batches, n):
    """Lists of n consecutive items of `batches`; a trailing shorter group is dropped."""
    group = []
    for b in batches:
        group.append(b)
        if len(group) == n:
            yield group
            group = []


def main(argv=None):
    """Runs the loop; returns the list of checkpoint files written."""
    args = parse_args(argv)
    from . import data, training
    from .datasets import kitti
    from .model.stereo_rcnn.resnet import load_checkpoint, resnet
    from .model.utils import net_utils
    from .model.utils.config import cfg

    if args.pre_nms_top_n is not None:
        cfg.TRAIN.RPN_PRE_NMS_TOP_N = int(args.pre_nms_top_n)
    limit = training.PROPOSAL_MAX_PRE_NMS
    if cfg.TRAIN.RPN_PRE_NMS_TOP_N > limit:
        print(PRE_NMS_ADVICE % (cfg.TRAIN.RPN_PRE_NMS_TOP_N, limit, limit, limit))
        return []
    if not torch.cuda.is_available():
        raise RuntimeError("training needs a GPU")
    dev = torch.device('cuda:0')
    seed = int(cfg.RNG_SEED if args.seed is None else args.seed)

    roidb, ratio_list, ratio_index = kitti.build_roidb(args.kitti_path, args.split, use_flipped=not args.no_flip)
    train_size = len(roidb)
    os.makedirs(args.save_dir, exist_ok=True)
    log_info = open(os.path.join(args.save_dir, 'trainlog.txt'), 'a' if args.resume else 'w')

    def log_string(s):
        log_info.write(s + '\n')
        log_info.flush()
        print(s)

    log_string('{:d} roidb entries'.format(train_size))
    log_string('backward precision: %s' % args.backward_precision)
    if args.forward_precision != 'f32':
        log_string('forward precision: %s' % args.forward_precision)
    if args.prepared_weights:
        log_string('prepared weights: once per step')
    if args.device_fold:
        log_string('device fold: BN fold and weight re-layout in one call per direction')
    if args.accum != 1:
        log_string('gradient accumulation: %d batches per step' % args.accum)
    if args.guard:
        log_string('guard: steps with non-finite gradients are skipped on the device')
    model = resnet(kitti.CLASSES, args.net, pretrained=False)
    model.create_architecture()
    if args.init:
        load_checkpoint(model, args.init)
    model.to(dev)
    lr = cfg.TRAIN.LEARNING_RATE if args.lr is None else args.lr
    uncert = torch.full((6,), -1.0, dtype=torch.float32, device=dev, requires_grad=True)
    optimizer = training.make_optimizer(model, uncert, lr=lr)
    start_epoch = args.start_epoch
    if args.resume:
        log_string('loading checkpoint %s' % args.resume)
        ckpt = torch.load(args.resume, map_location=dev)
        start_epoch = int(ckpt['epoch'])
        model.load_state_dict(ckpt['model'])
        optimizer.load_state_dict(ckpt['optimizer'])
        with torch.no_grad():
            uncert.copy_(ckpt['uncert'].to(dev))
        lr = optimizer.param_groups[0]['lr']

    gen_host = torch.Generator().manual_seed(seed)
    gen_dev = torch.Generator(device=dev).manual_seed(seed)
    loader = data.TrainLoader(roidb, ratio_index, args.batch_size, dev, generator=gen_host, workers=args.num_workers,
                              prefetch=args.prefetch)
    iters_per_epoch = int(train_size / args.batch_size) // args.accum
    validate = None
    if args.val_split:
        if not args.val_label_dir:
            raise SystemExit('--val-split needs --val-label-dir')
        from . import validation              # (only here: a run without --val-split imports none of the inference drivers)
        validate = validation.Validator(model, args.kitti_path, args.val_split, args.val_label_dir, args.save_dir,
                                        precision=args.val_precision, device=dev, log=log_string)
    written = []
    try:
        for epoch in range(start_epoch, args.max_epochs + 1):
            start = time.time()
            if epoch % (args.lr_decay_step + 1) == 0:
                net_utils.adjust_learning_rate(optimizer, args.lr_decay_gamma)
                lr *= args.lr_decay_gamma
            step = -1
            for step, group in enumerate(_groups(loader, args.accum)):
                if step >= iters_per_epoch:              # trainval_net.py:183,194: the leftover samples are not trained on
                    break
                batch = group[0] if args.accum == 1 else group
                res = training.train_step(model, optimizer, uncert, batch, clip_norm=10., generator=gen_dev,
                                          backward_precision=args.backward_precision, forward_precision=args.forward_precision,
                                          reuse_maxima=args.reuse_maxima, prepared_weights=args.prepared_weights,
                                          device_fold=args.device_fold, accum_steps=args.accum, guard=args.guard)
                if args.disp_interval > 0 and step % args.disp_interval == 0:
                    vals = {k: float(v) for k, v in res.items() if v is not None}          # the only host reads of the loop
                    log_string('[epoch %2d][iter %4d/%4d] loss: %.4f, lr: %.2e' % (epoch, step, iters_per_epoch, vals['loss'], lr))
                    log_string('\t\t\tuncert: ' + ', '.join('%.4f' % v for v in uncert.detach().cpu().tolist()))
                    log_string('\t\t\trpn_cls: %.4f, rpn_box_left_right: %.4f, rcnn_cls: %.4f, rcnn_box_left_right %.4f, dim_orien %.4f, '
                               'kpts %.4f, grad norm %.3f' % tuple([vals[k] for k in training.LOSS_NAMES] + [vals['grad_norm']]))
                    if args.guard:
                        log_string('\t\t\tskipped steps: %d%s' % (int(vals['skipped_steps']),
                                                                 '' if vals['ok'] != 0 else ' (this step was skipped: its gradients were not finite)'))
            save_name = os.path.join(args.save_dir, 'stereo_rcnn_{}_{}.pth'.format(epoch, min(step, iters_per_epoch - 1)))
            net_utils.save_checkpoint({'epoch': epoch + 1, 'model': model.state_dict(), 'optimizer': optimizer.state_dict(),
                                       'uncert': uncert.detach().clone()}, save_name)
            written.append(save_name)
            log_string('save model: {}'.format(save_name))
            log_string('time %.4f' % (time.time() - start))
            if validate is not None and args.val_every > 0 and epoch % args.val_every == 0:
                validate(epoch)
    finally:
        loader.close()
        log_info.close()
    return written


if __name__ == '__main__':
    main(sys.argv[1:])
