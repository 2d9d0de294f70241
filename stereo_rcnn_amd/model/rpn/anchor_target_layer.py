"""_AnchorTargetLayer on the HIP kernels (srcnn_anchor_targets, csrc/targets.hip).

Reference: lib/model/rpn/anchor_target_layer.py:26-190.  Same constructor and `forward(input)` as the reference; what differs:
  * nothing is read back from the device -- the reference's nonzero / `sum(keep) > 0` / `sum_fg[i] > num_fg` reads are
    comparisons inside the kernels;
  * the random subsampling takes its draws as tensors (include/srcnn_hip.h, "training target layers"): one uint32 key per
    anchor for the foreground and one for the background, drawn here on the device from `generator` (plain torch, no host
    read), or passed in (`fg_keys=`, `bg_keys=`: how a test replays the reference's recorded numpy permutations);
  * labels come back as int32 (what `rpn_losses` takes without a conversion).
CPU tensors raise NotImplementedError, as the project's other ops.
"""
import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from ..utils.config import cfg

_anchor_cache = {}


def pyramid_anchors(feat_shapes, device, ratios=None):
    """generate_anchors_all_pyramids (generate_anchors.py:112-173) for cfg's FPN scales / strides, built on the device in
    float64 and rounded to float32 once -- the arithmetic of the proposal kernel's analytic anchors (csrc/rpn_proposal.hip:
    gather_decode_kernel), bit-equal to the numpy anchors cast to float32.  (N, 4), anchor index = level offset + 3 loc + ratio.
    Cached per (shapes, ratios, device): a training loop builds them once."""
    ratios = list(cfg.ANCHOR_RATIOS if ratios is None else ratios)
    shapes = tuple((int(h), int(w)) for h, w in feat_shapes)
    key = (shapes, tuple(ratios), str(device))
    if key not in _anchor_cache:
        root = np.sqrt(np.asarray(ratios, dtype=np.float64))
        levels = []
        for scale, stride, (h, w) in zip(cfg.FPN_ANCHOR_SCALES, cfg.FPN_FEAT_STRIDES, shapes):
            half_w = torch.tensor(0.5 * (scale * root), dtype=torch.float64, device=device)
            half_h = torch.tensor(0.5 * (scale / root), dtype=torch.float64, device=device)
            step = cfg.FPN_ANCHOR_STRIDE
            cy = (torch.arange(0, h, step, dtype=torch.float64, device=device) * stride).view(-1, 1, 1)
            cx = (torch.arange(0, w, step, dtype=torch.float64, device=device) * stride).view(1, -1, 1)
            cy, cx = cy.expand(-1, cx.shape[1], 3), cx.expand(cy.shape[0], -1, 3)
            levels.append(torch.stack((cx - half_w, cy - half_h, cx + half_w, cy + half_h), 3).reshape(-1, 4))
        _anchor_cache[key] = torch.cat(levels, 0).float().contiguous()
    return _anchor_cache[key]


def draw_keys(shape, device, generator=None):
    """uint32 sampling keys as int32 bit patterns, drawn on the device."""
    return torch.randint(-2 ** 31, 2 ** 31, shape, dtype=torch.int32, device=device, generator=generator)


def as_key_bits(keys):
    """Any integer tensor of uint32 values (or int32 bit patterns) -> the contiguous int32 bit patterns the kernels read."""
    if keys.dtype != torch.int32:
        k = keys.to(torch.int64) & 0xFFFFFFFF
        keys = torch.where(k >= 2 ** 31, k - 2 ** 32, k).to(torch.int32)
    return keys.contiguous()


def anchor_targets(anchors, gt_left, gt_right, gt_merge, im_info, fg_keys, bg_keys, batch_size, num_fg, negative_overlap=None,
                   positive_overlap=None, clobber_positives=None, inside_weight=None, want_max_overlaps=False):
    """srcnn_anchor_targets on torch tensors.  Returns (labels (B, N) int32, targets_left (B, N, 4), targets_right (B, N, 4),
    inside_w (B, N), outside_w (B, N), max_overlaps (B, N) or None)."""
    if not gt_left.is_cuda:
        raise NotImplementedError
    dev = gt_left.device
    B, K = int(gt_left.shape[0]), int(gt_left.shape[1])
    N = int(anchors.shape[0])
    f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
    anchors, gt_left, gt_right, gt_merge, im_info = f32(anchors), f32(gt_left), f32(gt_right), f32(gt_merge), f32(im_info)
    fg_keys, bg_keys = as_key_bits(fg_keys), as_key_bits(bg_keys)
    assert tuple(fg_keys.shape) == (B, N) and tuple(bg_keys.shape) == (B, N), "one key per (image, anchor)"
    T = cfg.TRAIN
    params = _lib.AnchorTargetParams(
        float(T.RPN_NEGATIVE_OVERLAP if negative_overlap is None else negative_overlap),
        float(T.RPN_POSITIVE_OVERLAP if positive_overlap is None else positive_overlap),
        int(T.RPN_CLOBBER_POSITIVES if clobber_positives is None else clobber_positives), int(batch_size), int(num_fg),
        float(T.RPN_BBOX_INSIDE_WEIGHTS[0] if inside_weight is None else inside_weight))
    labels = torch.empty((B, N), dtype=torch.int32, device=dev)
    targets_left = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    targets_right = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    inside_w = torch.empty((B, N), dtype=torch.float32, device=dev)
    outside_w = torch.empty((B, N), dtype=torch.float32, device=dev)
    max_overlaps = torch.empty((B, N), dtype=torch.float32, device=dev) if want_max_overlaps else None
    L = _lib.lib()
    ws_bytes = L.srcnn_anchor_targets_workspace_bytes(B, K)
    ws = _lib.workspace(ws_bytes, dev, key="anchor_targets")
    _lib.check(L.srcnn_anchor_targets(_lib.ptr(anchors), N, _lib.ptr(gt_left), _lib.ptr(gt_right), _lib.ptr(gt_merge), B, K,
                                      _lib.ptr(im_info), _lib.ptr(fg_keys), _lib.ptr(bg_keys), params, _lib.ptr(labels),
                                      _lib.ptr(targets_left), _lib.ptr(targets_right), _lib.ptr(inside_w), _lib.ptr(outside_w),
                                      _lib.ptr(max_overlaps), ws.data_ptr(), ws_bytes, _lib.stream()), "srcnn_anchor_targets")
    return labels, targets_left, targets_right, inside_w, outside_w, max_overlaps


class _AnchorTargetLayer(nn.Module):
    """Assign anchors to ground-truth targets: classification labels and bounding-box regression targets for the RPN."""

    def __init__(self, feat_stride, ratios, generator=None, rpn_batchsize=None, rpn_fg_fraction=None):
        super(_AnchorTargetLayer, self).__init__()
        self._anchor_ratios = ratios
        self._feat_stride = feat_stride
        self._generator = generator
        self._rpn_batchsize = rpn_batchsize
        self._rpn_fg_fraction = rpn_fg_fraction
        if cfg.TRAIN.RPN_POSITIVE_WEIGHT >= 0:
            raise NotImplementedError("only the uniform example weighting (RPN_POSITIVE_WEIGHT < 0) exists: the reference's "
                                      "other branch (anchor_target_layer.py:143-145) never defines its weights")
        self.max_overlaps = None

    def forward(self, input, generator=None, fg_keys=None, bg_keys=None, rpn_batchsize=None, rpn_fg_fraction=None,
                want_max_overlaps=False):
        """input = (scores, gt_boxes_left, gt_boxes_right, gt_boxes_merge, im_info, num_boxes, feat_shapes), as the reference's.
        Returns [labels (B, N) int32, bbox_targets_left (B, N, 4), bbox_targets_right (B, N, 4), bbox_inside_weights (B, N),
        bbox_outside_weights (B, N)]; with want_max_overlaps the merged max overlap (B, N; -2 outside the image) is left in
        `self.max_overlaps`."""
        gt_left, gt_right, gt_merge, im_info, feat_shapes = input[1], input[2], input[3], input[4], input[6]
        if not gt_left.is_cuda:
            raise NotImplementedError
        dev = gt_left.device
        B = int(gt_left.shape[0])
        anchors = pyramid_anchors(feat_shapes, dev, self._anchor_ratios)
        N = int(anchors.shape[0])
        pick = lambda *vs: next(v for v in vs if v is not None)
        batch = int(pick(rpn_batchsize, self._rpn_batchsize, cfg.TRAIN.RPN_BATCHSIZE))
        num_fg = int(pick(rpn_fg_fraction, self._rpn_fg_fraction, cfg.TRAIN.RPN_FG_FRACTION) * batch)    # :102
        gen = generator if generator is not None else self._generator
        if fg_keys is None:
            fg_keys = draw_keys((B, N), dev, gen)
        if bg_keys is None:
            bg_keys = draw_keys((B, N), dev, gen)
        labels, tl, tr, inside_w, outside_w, self.max_overlaps = anchor_targets(
            anchors, gt_left, gt_right, gt_merge, im_info, fg_keys, bg_keys, batch, num_fg, want_max_overlaps=want_max_overlaps)
        return [labels, tl, tr, inside_w, outside_w]

    def backward(self, top, propagate_down, bottom):
        """This layer does not propagate gradients."""
        pass

    def reshape(self, bottom, top):
        """Reshaping happens during the call to forward."""
        pass
