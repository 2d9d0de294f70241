"""The training forward of Stereo R-CNN: one call returns the reference's 15-tuple with live losses, and backward() of them fills
.grad of every parameter the reference trains.

Reference: lib/model/stereo_rcnn/stereo_rcnn.py:141-324 and lib/model/rpn/stereo_rpn.py:62-138, followed line for line on the
exact-fp32 engine.  The model's modules stay parameter containers (its train() / forward() keep raising): this function reads
their parameters and composes
  * the differentiable NHWC convolution / linear layer (autograd.conv2d_nhwc, autograd.linear), frozen BatchNorms folded in-graph;
  * autograd.upsample_add / subsample2 (FPN top-down, P6) and autograd.conv_transpose2x2 (the end of the keypoint tower);
  * srcnn_rpn_score + _ProposalLayer on detached tensors with the cfg.TRAIN RPN settings, _AnchorTargetLayer, _ProposalTargetLayer;
  * the fused pyramid ROIAlign and its backward, NHWC on both sides, left | right written into the channel halves of one tensor;
  * losses.rpn_losses / losses.rcnn_losses.
RCNN_layer0 and the first cfg.RESNET.FIXED_BLOCKS stages run without a graph.  Both eyes go through the trunk, the FPN and
RPN_Conv as one batch of 2B images (the B left ones first), as plan.py does.

Host reads: one -- im_info[0][0], the image height the ROIAlign level scales divide by (the reference reads the same value,
stereo_rcnn.py:128); pass im_info as a CPU tensor and nothing waits for the device.  The proposal target layer's "no candidates"
status stays a device word (taps['proposal_status']).

Randomness: `generator` (a generator of the model's device) feeds, in this order, the anchor target layer's keys, the proposal
target layer's keys and draws, and the two dropout masks of RCNN_top.  Dropout(p=0.2) in training mode (resnet.py:256-263) is a
multiply by mask / 0.8, mask = [torch.rand(...) >= 0.2].

Limit: srcnn_proposal_layer ranks at most 8192 candidates before the NMS, so cfg.TRAIN.RPN_PRE_NMS_TOP_N (12000 in the
reference's configuration) has to be set to 8192 or less for any image with more anchors than that; forward_train raises otherwise.

The rest of an iteration of trainval_net.py:207-227 is here too: make_optimizer builds the reference's parameter groups on
stereo_rcnn_amd.optim.SGD, and train_step runs zero-grad, forward_train, the multi-task loss, backward() and the clipped SGD step
(csrc/optim.hip: one norm pass over the gradients, one fused update) as one call without a further host read.  After training, an
inference plan's prepared weights (plan.py, engine.prep_*) are copies made from the parameters as they were: call
Plan.refresh(model) before running inference -- it overwrites them in place on the device (csrc/prep_weights.hip) and keeps the
plan's buffers and, where no weight scale moved, its recorded launch programs (trainval_net --val-split does so every epoch).

The data side is stereo_rcnn_amd/datasets/kitti.py (annotations -> roidb, once) and stereo_rcnn_amd/data.py (TrainLoader: PNG
decode in worker processes, batch assembly in csrc/loader.hip), and stereo_rcnn_amd/trainval_net.py is the reference's training
loop on these pieces.
"""
import contextlib

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, autograd, engine
from .model.rpn.anchor_target_layer import _AnchorTargetLayer
from .model.rpn.proposal_target_layer import _ProposalTargetLayer
from .model.stereo_rcnn import losses
from .model.utils.config import cfg

PROPOSAL_MAX_PRE_NMS = 8192     # srcnn_proposal_layer's top-K limit (csrc/rpn_proposal.hip)
DROPOUT_P = 0.2          # RCNN_top's nn.Dropout(p=0.2), resnet.py:259,262


def trainable_parameters(model):
    """{name: parameter} of what the reference leaves requires_grad=True (resnet.py:288-309): everything but RCNN_layer0, the
    first cfg.RESNET.FIXED_BLOCKS stages and every BatchNorm of RCNN_layer0..4."""
    assert 0 <= cfg.RESNET.FIXED_BLOCKS < 4
    frozen = set()
    for name, m in model.named_modules():
        if isinstance(m, nn.BatchNorm2d):
            frozen.update(name + '.' + k for k, _ in m.named_parameters(recurse=False))
    fixed = tuple('RCNN_layer%d.' % i for i in range(0, cfg.RESNET.FIXED_BLOCKS + 1))
    return {k: p for k, p in model.named_parameters() if k not in frozen and not k.startswith(fixed)}


def make_optimizer(model, uncert, lr=None):
    """The optimiser of trainval_net.py:153-168 on optim.SGD: one group per trainable parameter -- a name containing 'bias' gets
    lr * (DOUBLE_BIAS + 1) and weight decay `BIAS_DECAY and WEIGHT_DECAY or 0`, every other one lr and WEIGHT_DECAY -- and a last
    group for `uncert` (the six log-variances of the multi-task loss) with lr and no weight decay; momentum cfg.TRAIN.MOMENTUM."""
    from . import optim
    T = cfg.TRAIN
    lr = T.LEARNING_RATE if lr is None else lr
    params = []
    for key, value in trainable_parameters(model).items():
        if 'bias' in key:
            params.append({'params': [value], 'lr': lr * (T.DOUBLE_BIAS + 1), 'weight_decay': T.BIAS_DECAY and T.WEIGHT_DECAY or 0})
        else:
            params.append({'params': [value], 'lr': lr, 'weight_decay': T.WEIGHT_DECAY})
    params.append({'params': [uncert], 'lr': lr})
    return optim.SGD(params, momentum=T.MOMENTUM)


LOSS_NAMES = ('rpn_loss_cls', 'rpn_loss_bbox_left_right', 'RCNN_loss_cls', 'RCNN_loss_bbox', 'RCNN_loss_dim_orien', 'RCNN_loss_kpts')


def train_step(model, optimizer, uncert, batch, clip_norm=10., generator=None, backward_precision='f32', forward_precision='f32',
               reuse_maxima=True, prepared_weights=False, device_fold=False, accum_steps=1, guard=False):
    """One iteration of trainval_net.py:207-227.  batch: forward_train's nine inputs (im_left, im_right, im_info, gt_boxes_left,
    gt_boxes_right, gt_boxes_merge, gt_dim_orien, gt_kpts, num_boxes).  Gradients are set to None, forward_train and
    losses.multi_task_loss build the total, backward() fills the gradients, and optimizer.step clips the MODEL's gradients to
    `clip_norm` (uncert's stays as it is, as in the reference) inside the fused update.  backward_precision, forward_precision,
    reuse_maxima: forward_train's.  prepared_weights: True builds a TrainWeights for the model (kept on the optimiser and reused)
    and calls its prepare() at the start of EVERY step -- never a cache keyed on a version counter: optimizer.step writes the
    parameters through raw pointers, which torch's counter does not see.  device_fold (it needs prepared_weights=True, ValueError
    otherwise): that prepare() folds and re-lays-out the weights on the device (TrainWeights.prepare).  Returns device scalars: 'loss', the six
    terms by name, 'grad_norm' (the model's gradient norm before clipping).  The only host read is forward_train's im_info[0][0].

    accum_steps = N > 1: `batch` is a sequence of N such batches (images of different sizes are fine: nothing is padded).  For each,
    in order, forward_train, the multi-task loss and backward() run, autograd summing into .grad; ONE optimizer.step with
    grad_scale = 1 / N follows, the update of the mean gradient, clipped by the mean gradient's norm ('grad_norm').  `generator`
    goes on from micro-batch to micro-batch.  prepare() runs once per train_step (the weights do not change in between; every
    backward but the last keeps the fold's graph).  Each returned scalar is the mean over the micro-batches: summed in order, then
    multiplied by 1 / N, on the device.  The host reads im_info[0][0] once per micro-batch and nothing else.
    guard=True: optim.SGD.step's guard -- where a gradient is not finite the step changes no parameter and no momentum buffer;
    the result also carries 'ok' (device float, 1 or 0) and 'skipped_steps' (the optimiser's device counter).
    accum_steps=1, guard=False is the plain step, call for call."""
    if device_fold and not prepared_weights:
        raise ValueError("device_fold=True needs prepared_weights=True: it is TrainWeights.prepare's fold that moves to the device")
    accum_steps = int(accum_steps)
    if accum_steps < 1:
        raise ValueError("accum_steps must be >= 1, got %d" % accum_steps)
    batches = [batch] if accum_steps == 1 else list(batch)
    if len(batches) != accum_steps:
        raise ValueError("accum_steps = %d needs a sequence of %d batches, got %d" % (accum_steps, accum_steps, len(batches)))
    optimizer.zero_grad(set_to_none=True)
    for p in model.parameters():
        p.grad = None
    weights = None
    if prepared_weights:
        weights = getattr(optimizer, '_train_weights', None)
        if weights is None or weights.model is not model:
            weights = optimizer._train_weights = TrainWeights(model)
        weights.prepare(device_fold=device_fold)
    sums = None
    for i, one in enumerate(batches):
        out = forward_train(model, *one, generator=generator, backward_precision=backward_precision, forward_precision=forward_precision,
                            reuse_maxima=reuse_maxima, weights=weights)
        terms = list(out[8:14])                     # scalars: the reference's .mean() of each is the identity on one device
        total = losses.multi_task_loss(terms, uncert)
        # the prepared weights' fold is one graph under every micro-batch's: it is released by the last backward
        total.backward(retain_graph=weights is not None and i + 1 < accum_steps)
        values = [total.detach()] + [t.detach() for t in terms]
        sums = values if sums is None else [s + v for s, v in zip(sums, values)]
    clip_params = [p for p in model.parameters() if p.requires_grad]
    if accum_steps == 1 and not guard:
        optimizer.step(clip_norm=clip_norm, clip_params=clip_params)
    else:
        optimizer.step(clip_norm=clip_norm, clip_params=clip_params, guard=guard, grad_scale=1.0 / accum_steps)
        if accum_steps > 1:
            sums = [s * (1.0 / accum_steps) for s in sums]
    result = dict(zip(('loss',) + LOSS_NAMES, sums))
    result['grad_norm'] = optimizer.last_norm[0] if clip_norm is not None else None
    if guard:
        result['ok'] = optimizer.last_norm[2]
        result['skipped_steps'] = optimizer.skipped_steps
    return result


def _bn(m):
    return {'weight': m.weight, 'bias': m.bias, 'running_mean': m.running_mean, 'running_var': m.running_var}


class _Taps(object):
    def __init__(self, store):
        self.store = store

    def __call__(self, name, t):
        if self.store is not None:
            self.store[name] = t.detach()
        return t


def _conv(m, x, prec, relu=False, residual=None, bn=None, weights=None):
    return autograd.conv2d_nhwc(x, m.weight, m.bias, int(m.stride[0]), int(m.padding[0]), relu, residual, None if bn is None else _bn(bn),
                                _prec=prec, prepared=None if weights is None else weights[m])


def _bottleneck(blk, x, name, tap, prec, weights=None):
    """resnet.py:66-100: relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + shortcut(x)), the ReLUs and the residual fused
    into the convolutions as the engine fuses them."""
    t = tap(name + '.conv1', _conv(blk.conv1, x, prec, True, bn=blk.bn1, weights=weights))
    t = tap(name + '.conv2', _conv(blk.conv2, t, prec, True, bn=blk.bn2, weights=weights))
    res = x if not hasattr(blk, 'downsample') else _conv(blk.downsample[0], x, prec, False, bn=blk.downsample[1], weights=weights)
    return tap(name + '.out', _conv(blk.conv3, t, prec, True, residual=res, bn=blk.bn3, weights=weights))


def _linear(layer, x, prec, relu=False):
    """autograd.linear over a PreparedLayer of TrainWeights: its w (out, 1, 1, K) is the linear layer's (out, K)."""
    return autograd.linear(x, layer.w.view(int(layer.w.shape[0]), -1), layer.b, relu=relu, _prec=prec, prepared=layer)


class TrainWeights(object):
    """Every weight forward_train's graph layers use, folded and prepared for the f16x3 engine ONCE per step: specs() lists
    exactly the (weight, bias, bn) combinations forward_train composes -- the bottleneck convolutions of the stages with a graph
    (their frozen BNs folded by autograd's own fold, inside the graph), the FPN layers, RPN_Conv, the concatenated RPN head, RCNN_top[0]'s
    permuted view and RCNN_top[3], the concatenated box heads, the keypoint tower, its deconvolution in row order (i, j, co) and
    kpts_class --, fold() folds them, and prepare() then makes one engine.prepare_train_weights call over all of them (csrc/train_weights.hip: max |w| and the
    four hi / lo planes of every layer in a fixed number of launches).  weights[key] is the autograd.PreparedLayer: key is the
    module for a plain convolution, 'rpn_head', 'RCNN_top.0', 'RCNN_top.3', 'box_heads', 'RCNN_kpts.12' otherwise.  The folded
    weights carry the graph, so prepare() belongs to ONE forward_train + backward: call it at the start of every step, after the
    optimiser's update (train_step(prepared_weights=True) does).  The fold and the re-layout are eager torch operators by default;
    prepare(device_fold=True) runs them, and their adjoint, on the device in one call each."""

    def __init__(self, model):
        self.model = model
        self.layers = {}

    def __getitem__(self, key):
        return self.layers[key]

    def enumerate(self):
        """[(key, folded w, folded b)] in forward_train's order of first use: specs() folded by eager torch operators."""
        return [(key,) + autograd.fold_spec(s) for key, s in self.specs()]

    def specs(self):
        """[(key, engine.FoldSpec)] in forward_train's order of first use: THE inventory of the graph layers, each named by its
        PARAMETERS (parts are concatenated along the output rows).  Both folds, and through them forward_train, read it."""
        model, S = self.model, engine.FoldSpec
        for p in trainable_parameters(model).values():
            p.requires_grad_(True)
        out = []
        for li in (1, 2, 3, 4):
            if li <= cfg.RESNET.FIXED_BLOCKS:
                continue
            for blk in getattr(model, 'RCNN_layer%d' % li)[0]:
                pairs = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2)]
                if hasattr(blk, 'downsample'):
                    pairs.append((blk.downsample[0], blk.downsample[1]))
                pairs.append((blk.conv3, blk.bn3))
                out += [(m, S('conv', [(m.weight, m.bias)], _bn(bn))) for m, bn in pairs]
        rpn = model.RCNN_rpn
        for m in (model.RCNN_toplayer, model.RCNN_latlayer1, model.RCNN_smooth1, model.RCNN_latlayer2, model.RCNN_smooth2,
                  model.RCNN_latlayer3, model.RCNN_smooth3, rpn.RPN_Conv):
            out.append((m, S('conv', [(m.weight, m.bias)])))
        out.append(('rpn_head', S('conv', [(m.weight, m.bias) for m in (rpn.RPN_cls_score, rpn.RPN_bbox_pred_left_right)])))
        top0, top3 = model.RCNN_top[0], model.RCNN_top[3]
        out.append(('RCNN_top.0', S('conv', [(top0.weight, top0.bias)])))           # viewed (2048, 1, 1, 49 * 512) by fold()
        out.append(('RCNN_top.3', S('conv', [(top3.weight, top3.bias)])))           # 1x1: the linear layer's (out, 1, 1, K)
        out.append(('box_heads', S('linear', [(m.weight, m.bias) for m in (model.RCNN_bbox_pred, model.RCNN_dim_orien_pred,
                                                                          model.RCNN_cls_score)])))
        for i in (0, 2, 4, 6, 8, 10):
            m = model.RCNN_kpts[i]
            out.append((m, S('conv', [(m.weight, m.bias)])))
        up = model.RCNN_kpts[12]
        out.append(('RCNN_kpts.12', S('deconv2x2', [(up.weight, up.bias)])))
        out.append((model.kpts_class, S('conv', [(model.kpts_class.weight, model.kpts_class.bias)])))
        return out

    def fold(self, device_fold=False):
        """Every layer folded, without planes (PreparedLayer.planes None: the f16x3 calls make their own).  device_fold: False folds
        layer by layer with eager torch operators (autograd.fold_spec: what enumerate() returns); True replaces them (per layer a float64 fold, a
        permute().contiguous(), a torch.cat) by ONE autograd.fold_all over specs() -- two library calls per step, forward and adjoint
        (csrc/train_fold.hip).  Every folded tensor and every parameter gradient has the same bits either way."""
        named = self.specs()
        folded = autograd.fold_all([s for _, s in named]) if device_fold else [autograd.fold_spec(s) for _, s in named]
        self.layers = {}
        for (key, _), (w, b) in zip(named, folded):
            w = w.contiguous()
            if key == 'RCNN_top.0':
                w = w.view(int(w.shape[0]), 1, 1, -1)           # the 7x7/7 conv sees one window: a linear layer over (kh, kw, c)
            self.layers[key] = autograd.PreparedLayer(w, b, None)
        return self

    def prepare(self, device_fold=False):
        """fold(device_fold), then the planes of every folded weight in one engine.prepare_train_weights call."""
        self.fold(device_fold)
        planes = engine.prepare_train_weights([layer.w for layer in self.layers.values()])
        self.layers = {key: layer._replace(planes=p) for (key, layer), p in zip(self.layers.items(), planes)}
        return self


def _stem(model, im_left, im_right):
    """RCNN_layer0 (always frozen): stem pack, 7x7/2 conv + BN + ReLU, 3x3/2 ceil-mode max-pool; (2B, h, w, 64)."""
    B, _, H, W = (int(v) for v in im_left.shape)
    dev = im_left.device
    N = 2 * B
    cw = engine.prep_stem(model.RCNN_layer0[0].weight.detach(), {k: v.detach() for k, v in _bn(model.RCNN_layer0[1]).items()}, dev)
    packed = torch.empty((N, H + 6, W + 8, 4), dtype=torch.float32, device=dev)
    engine.stem_pack_pair(im_left.detach().float().contiguous(), im_right.detach().float().contiguous(), packed)
    sh, sw = engine.conv_out_hw(H, W, 7, 7, 2, 3)
    stem_out = torch.empty((N, sh, sw, 64), dtype=torch.float32, device=dev)
    engine.conv2d(cw, packed, N, H + 6, W + 8, stem_out, sh, sw, x_cstride=4, precision='f32')
    ph, pw = -(-(sh - 3) // 2) + 1, -(-(sw - 3) // 2) + 1           # ceil_mode (resnet.py:113)
    if (ph - 1) * 2 >= sh:
        ph -= 1
    if (pw - 1) * 2 >= sw:
        pw -= 1
    c1 = torch.empty((N, ph, pw, 64), dtype=torch.float32, device=dev)
    engine.maxpool3x3s2_ceil(stem_out, N, sh, sw, 64, c1, ph, pw)
    return stem_out, c1


class _PyramidRoIFeatNHWC(torch.autograd.Function):
    """PyramidRoI_Feat (stereo_rcnn.py:110-139) NHWC to NHWC for one or two eyes: eye e's features of its rois go into channels
    [e C, e C + C) of one (n, A, A, eyes C) tensor -- the torch.cat of stereo_rcnn.py:248-249 never materialises.  maps: eye 0's
    four levels P2..P5, then eye 1's."""

    @staticmethod
    def forward(ctx, im_height, A, eyes, *args):
        rois, maps = args[:eyes], args[eyes:]
        C, n = int(maps[0].shape[3]), int(rois[0].shape[0])
        out = torch.empty((n, A, A, eyes * C), dtype=torch.float32, device=maps[0].device)
        for e in range(eyes):
            lv = maps[4 * e:4 * e + 4]
            engine.pyramid_roi_align(lv, [(int(m.shape[1]), int(m.shape[2])) for m in lv], C, im_height, rois[e], n, A, out,
                                     eyes * C, e * C)
        ctx.save_for_backward(*rois)
        ctx.geometry = (im_height, A, eyes, C, [tuple(m.shape) for m in maps])
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rois = ctx.saved_tensors
        im_height, A, eyes, C, shapes = ctx.geometry
        g = grad_out.contiguous()
        grads = [torch.empty(s, dtype=torch.float32, device=g.device) for s in shapes]
        for e in range(eyes):
            gs, ss = grads[4 * e:4 * e + 4], shapes[4 * e:4 * e + 4]
            _lib.check(_lib.lib().srcnn_pyramid_roi_align_backward(g.data_ptr(), eyes * C, e * C, rois[e].data_ptr(), int(rois[e].shape[0]),
                                                                   A, C, im_height, _lib.ptr_array(gs), _lib.int_array(s[1] for s in ss),
                                                                   _lib.int_array(s[2] for s in ss), ss[0][0], _lib.FMT_F32, None,
                                                                   _lib.stream()), "srcnn_pyramid_roi_align_backward")
        return (None, None, None) + (None,) * eyes + tuple(grads)


def _roi_feat(maps_per_eye, rois_per_eye, im_height, A):
    eyes = len(rois_per_eye)
    rois = [r.detach().reshape(-1, 5).float().contiguous() for r in rois_per_eye]
    maps = [m.contiguous() for lv in maps_per_eye for m in lv]
    return _PyramidRoIFeatNHWC.apply(im_height, A, eyes, *(rois + maps))


def _dropout(x, generator, tap, name):
    mask = (torch.rand(x.shape, dtype=torch.float32, device=x.device, generator=generator) >= DROPOUT_P).float()
    tap(name, mask)
    return x * (mask / (1.0 - DROPOUT_P))


def forward_train(model, im_left, im_right, im_info, gt_boxes_left, gt_boxes_right, gt_boxes_merge, gt_dim_orien, gt_kpts, num_boxes,
                  generator=None, taps=None, backward_precision='f32', forward_precision='f32', reuse_maxima=True, weights=None):
    """The reference's training forward (stereo_rcnn.py:141-324).  model: a _StereoRCNN on the GPU; images (B, 3, H, W) on the
    same device; im_info (B, 3) (CPU or device), ground truth as the reference's data loader gives it.  Returns (rois_left,
    rois_right, cls_prob, bbox_pred, dim_orien_pred, kpts_prob, left_border_prob, right_border_prob, rpn_loss_cls,
    rpn_loss_bbox_left_right, RCNN_loss_cls, RCNN_loss_bbox, RCNN_loss_dim_orien, RCNN_loss_kpts, rois_label).  The six losses carry
    a graph; the parameters of trainable_parameters(model) are switched to requires_grad=True, so backward() sets their .grad and
    leaves every other parameter's None.  taps (a dict) receives named detached intermediates: every ReLU output by layer name,
    'rois_left' / 'rois_right' (the proposals), 'anchor_targets' and 'proposal_targets' (the layers' output lists),
    'proposal_status', 'dropout1' / 'dropout2'.  backward_precision: 'f32' (the exact fp32 backward, the default) or 'f16x3'
    (srcnn_conv2d_backward_f16x3) for the gradients of every convolution / linear layer that has a graph.  forward_precision: 'f32'
    (the exact-fp32 engine, the default: outputs and losses keep their bits whatever backward_precision is) or 'f16x3'
    (srcnn_conv2d_forward_f16x3: the 3 x f16 split with scales found on the device, no host read) for the forward of the same
    layers; RCNN_layer0 and the first cfg.RESNET.FIXED_BLOCKS stages, which have no graph, stay on the fp32 engine.  The two are
    independent.  reuse_maxima (default True; it matters only where a precision is 'f16x3'): each activation's max |x| is found at
    most once -- in the epilogue of the f16x3 convolution that produced it, or by one scan -- and handed to every f16x3 call that
    consumes it (stereo_rcnn_amd.autograd); every output and gradient keeps its bits.  Either precision may be 'auto':
    autograd.choose_engine picks the engine per layer and direction from the layer's GEMM size (the frozen stages stay fp32);
    `with autograd.record_engines() as log:` around the call receives (M, N, K, forward engine, backward engine) of every
    convolution call in call order.  weights: a
    TrainWeights(model) whose prepare() ran for THIS call (after the last optimiser update): the layers take their folded weights
    and their f16x3 planes from it and the f16x3 calls launch no pass over a weight; layers on the fp32 engine ignore the planes.
    It composes with every precision and changes no bit.  None: a TrainWeights made and folded for this call, without planes."""
    prec = autograd.Precision(forward_precision, backward_precision, reuse_maxima)
    dev = model.RCNN_toplayer.weight.device
    if dev.type != 'cuda' or not im_left.is_cuda:
        raise NotImplementedError
    tap = _Taps(taps if isinstance(taps, dict) else None)
    wts = weights if weights is not None else TrainWeights(model).fold()     # (specs() switches the trainable parameters' requires_grad on)
    B = int(im_left.shape[0])
    im_info_host = im_info.detach().cpu() if im_info.is_cuda else im_info.detach()
    im_height = float(im_info_host[0][0])
    im_info = im_info.detach().to(device=dev, dtype=torch.float32)
    on_dev = lambda t: t.detach().to(dev)
    gt_boxes_left, gt_boxes_right, gt_boxes_merge = on_dev(gt_boxes_left), on_dev(gt_boxes_right), on_dev(gt_boxes_merge)
    gt_dim_orien, gt_kpts, num_boxes = on_dev(gt_dim_orien), on_dev(gt_kpts), on_dev(num_boxes)

    # ---- bottom-up (stereo_rcnn.py:155-159, 172-176), both eyes as one batch
    with torch.no_grad():
        stem_out, x = _stem(model, im_left, im_right)
        tap('RCNN_layer0', stem_out)
    c = []
    for li in (1, 2, 3, 4):
        frozen = li <= cfg.RESNET.FIXED_BLOCKS
        with (torch.no_grad() if frozen else contextlib.nullcontext()):
            for b, blk in enumerate(getattr(model, 'RCNN_layer%d' % li)[0]):
                x = _bottleneck(blk, x, 'RCNN_layer%d.0.%d' % (li, b), tap, prec.without_graph() if frozen else prec,
                                None if frozen else wts)
        c.append(x)
    c2, c3, c4, c5 = c

    # ---- top-down (:161-168, 178-185)
    p5 = _conv(model.RCNN_toplayer, c5, prec, weights=wts)
    p4 = _conv(model.RCNN_smooth1, autograd.upsample_add(p5, _conv(model.RCNN_latlayer1, c4, prec, weights=wts)), prec, weights=wts)
    p3 = _conv(model.RCNN_smooth2, autograd.upsample_add(p4, _conv(model.RCNN_latlayer2, c3, prec, weights=wts)), prec, weights=wts)
    p2 = _conv(model.RCNN_smooth3, autograd.upsample_add(p3, _conv(model.RCNN_latlayer3, c2, prec, weights=wts)), prec, weights=wts)
    p6 = autograd.subsample2(p5)
    levels = [p2, p3, p4, p5, p6]
    shapes = [(int(p.shape[1]), int(p.shape[2])) for p in levels]

    # ---- stereo RPN (stereo_rpn.py:73-95)
    rpn = model.RCNN_rpn
    head = wts['rpn_head']
    n_anchors = sum(3 * h * w for h, w in shapes)
    probs = torch.empty((B, n_anchors, 2), dtype=torch.float32, device=dev)
    deltas = torch.empty((B, n_anchors, 6), dtype=torch.float32, device=dev)
    scores, bbox_preds, off = [], [], 0
    for l, (p, (h, w)) in enumerate(zip(levels, shapes)):
        r = tap('RPN_Conv.%d' % l, _conv(rpn.RPN_Conv, p, prec, True, weights=wts))     # (2B, h, w, 512): left images, then right
        hd = autograd.conv2d_nhwc(torch.cat((r[:B], r[B:]), 3), head.w.permute(0, 3, 1, 2), head.b, _prec=prec, prepared=head)  # [cls 6 | bbox 18]
        # :89,91: NHWC rows viewed as (-1, 2) / (-1, 6) -- the raw scores pair channels (0, 1) (2, 3) (4, 5)
        scores.append(hd[..., :6].reshape(B, h * w * 3, 2))
        bbox_preds.append(hd[..., 6:].reshape(B, h * w * 3, 6))
        _lib.check(_lib.lib().srcnn_rpn_score(hd.detach().data_ptr(), B, h * w, 24, probs.data_ptr(), deltas.data_ptr(), off, n_anchors,
                                              _lib.stream()), "srcnn_rpn_score")
        off += 3 * h * w
    rpn_cls_score_alls, rpn_bbox_pred_alls = torch.cat(scores, 1), torch.cat(bbox_preds, 1)
    T = cfg.TRAIN
    # the proposal kernel ranks at most PROPOSAL_MAX_PRE_NMS candidates: a larger cfg.TRAIN.RPN_PRE_NMS_TOP_N (the reference's
    # default is 12000) on an image with more anchors than that is refused here, never silently lowered
    pre_nms = min(int(T.RPN_PRE_NMS_TOP_N), n_anchors)
    if pre_nms > PROPOSAL_MAX_PRE_NMS:
        raise ValueError("cfg.TRAIN.RPN_PRE_NMS_TOP_N = %d on %d anchors: srcnn_proposal_layer ranks at most %d candidates; set it "
                         "to %d or less" % (T.RPN_PRE_NMS_TOP_N, n_anchors, PROPOSAL_MAX_PRE_NMS, PROPOSAL_MAX_PRE_NMS))
    rois_left, rois_right = rpn.RPN_proposal.run(probs, deltas, im_info, [list(s) for s in shapes], pre_nms,
                                                 T.RPN_POST_NMS_TOP_N, T.RPN_NMS_THRESH)
    tap('rois_left', rois_left), tap('rois_right', rois_right)
    anchor_layer = _AnchorTargetLayer(rpn.feat_stride, rpn.anchor_ratios)
    rpn_data = anchor_layer((rpn_cls_score_alls.detach(), gt_boxes_left, gt_boxes_right, gt_boxes_merge, im_info, num_boxes, shapes),
                            generator=generator)
    if tap.store is not None:
        tap.store['anchor_targets'] = [t.detach() for t in rpn_data]
    rpn_loss_cls, rpn_loss_box = losses.rpn_losses(rpn_cls_score_alls, rpn_bbox_pred_alls, *rpn_data)

    # ---- proposal targets (stereo_rcnn.py:199-230)
    target_layer = _ProposalTargetLayer(model.n_classes)
    roi_data = target_layer(rois_left, rois_right, gt_boxes_left, gt_boxes_right, gt_dim_orien, gt_kpts, num_boxes, generator=generator)
    if tap.store is not None:
        tap.store['proposal_targets'] = [t.detach() for t in roi_data]
        tap.store['proposal_status'] = target_layer.status
    rois_left, rois_right, rois_label = roi_data[0], roi_data[1], roi_data[2]
    n = int(rois_left.shape[0]) * int(rois_left.shape[1])

    # ---- box head (:248-257): 7x7 left | right -> RCNN_top as two GEMMs (the 7x7/7 conv sees one window) -> three linear heads
    left_maps, right_maps = [p[:B] for p in levels[:4]], [p[B:] for p in levels[:4]]
    feat = _roi_feat([left_maps, right_maps], [rois_left, rois_right], im_height, cfg.POOLING_SIZE)
    t = tap('RCNN_top.0', _linear(wts['RCNN_top.0'], feat.reshape(n, -1), prec, relu=True))
    t = _dropout(t, generator, tap, 'dropout1')
    t = tap('RCNN_top.3', _linear(wts['RCNN_top.3'], t, prec, relu=True))
    t = _dropout(t, generator, tap, 'dropout2')                                           # .mean(3).mean(2) over a 1x1 map
    n_bbox, n_dim = int(model.RCNN_bbox_pred.weight.shape[0]), int(model.RCNN_dim_orien_pred.weight.shape[0])
    fc = _linear(wts['box_heads'], t, prec)
    bbox_all, dim_all, cls_score = fc[:, :n_bbox], fc[:, n_bbox:n_bbox + n_dim], fc[:, n_bbox + n_dim:]
    cls_prob = F.softmax(cls_score, 1)

    # ---- keypoint head (:260-271)
    k = _roi_feat([left_maps], [rois_left], im_height, cfg.POOLING_SIZE * 2)
    for i in (0, 2, 4, 6, 8, 10):
        k = tap('RCNN_kpts.%d' % i, _conv(model.RCNN_kpts[i], k, prec, True, weights=wts))
    up = model.RCNN_kpts[12]
    k = tap('RCNN_kpts.12', autograd.conv_transpose2x2(k, up.weight, up.bias, relu=True, _prec=prec,
                                                               prepared=wts['RCNN_kpts.12']))
    kpts_pred_all = _conv(model.kpts_class, k, prec, weights=wts).sum(1).permute(0, 2, 1).contiguous()       # (n, 28, 28, 6) -> sum over H -> (n, 6, G)
    G = cfg.KPTS_GRID
    kpts_prob = F.softmax(kpts_pred_all[:, :4, :].reshape(n, 4 * G), 1)
    left_border_prob = F.softmax(kpts_pred_all[:, 4, :], 1)
    right_border_prob = F.softmax(kpts_pred_all[:, 5, :], 1)

    # ---- losses (:274-311)
    loss_cls, loss_bbox, loss_dim_orien, loss_kpts = losses.rcnn_losses(cls_score, bbox_all, dim_all, kpts_pred_all, *roi_data[2:])
    sel = rois_label.reshape(n, 1, 1).long()
    bbox_pred = torch.gather(bbox_all.reshape(n, -1, 6), 1, sel.expand(n, 1, 6)).squeeze(1)
    dim_orien_pred = torch.gather(dim_all.reshape(n, -1, 5), 1, sel.expand(n, 1, 5)).squeeze(1)
    return (rois_left.view(B, -1, 5), rois_right.view(B, -1, 5), cls_prob.view(B, -1, cls_prob.shape[1]), bbox_pred.view(B, -1, 6),
            dim_orien_pred.view(B, -1, 5), kpts_prob, left_border_prob, right_border_prob, rpn_loss_cls, rpn_loss_box,
            loss_cls, loss_bbox, loss_dim_orien, loss_kpts, rois_label.view(B, -1))
