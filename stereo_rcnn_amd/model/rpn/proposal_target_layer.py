"""_ProposalTargetLayer on the HIP kernel (srcnn_proposal_targets, csrc/targets.hip).

Reference: lib/model/rpn/proposal_target_layer.py:21-333.  Same constructor and `forward` as the reference; what differs:
  * nothing is read back from the device (the reference loops in Python over every foreground roi and goes through
    np.union1d on the host); where the reference raises -- an image with neither foreground nor background candidates --
    the image's outputs are all zero and `self.status[b]` is 1: `check_status()` reads it when the caller chooses to;
  * the sampling takes its draws as tensors (include/srcnn_hip.h, "training target layers"): a uint32 key per candidate roi
    for the foreground permutation and a float64 u in [0, 1) per output row for the draws with replacement, drawn here on
    the device from `generator` or passed in (`fg_keys=`, `u=`);
  * labels and keypoint targets come back as int32 (what `rcnn_losses` takes without a conversion).
CPU tensors raise NotImplementedError, as the project's other ops.
"""
import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from ..utils.config import cfg
from .anchor_target_layer import as_key_bits, draw_keys


def proposal_targets(rois_left, rois_right, gt_left, gt_right, gt_dim_orien, gt_kpts, fg_keys, u, rois_per_image, fg_rois_per_image,
                     want_keep_inds=False):
    """srcnn_proposal_targets on torch tensors.  Returns the ten tensors of proposal_target_layer.py:66-67, then status (B) int32
    and keep_inds (B, S) int32 or None."""
    if not gt_left.is_cuda:
        raise NotImplementedError
    dev = gt_left.device
    B, R, K, S = int(rois_left.shape[0]), int(rois_left.shape[1]), int(gt_left.shape[1]), int(rois_per_image)
    f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
    rois_left, rois_right, gt_left, gt_right = f32(rois_left), f32(rois_right), f32(gt_left), f32(gt_right)
    gt_dim_orien, gt_kpts = f32(gt_dim_orien), f32(gt_kpts)
    fg_keys = as_key_bits(fg_keys)
    u = u.detach().to(device=dev, dtype=torch.float64).contiguous()
    assert tuple(fg_keys.shape) == (B, R + K) and tuple(u.shape) == (B, S), "keys (B, R + K), u (B, rois_per_image)"
    T = cfg.TRAIN
    c4, c5 = _lib.c_float * 4, _lib.c_float * 5
    params = _lib.ProposalTargetParams(float(T.FG_THRESH), float(T.BG_THRESH_HI), float(T.BG_THRESH_LO), S, int(fg_rois_per_image),
                                       int(cfg.KPTS_GRID), c4(*T.BBOX_NORMALIZE_MEANS), c4(*T.BBOX_NORMALIZE_STDS),
                                       c5(*T.DIM_NORMALIZE_MEANS), c5(*T.DIM_NORMALIZE_STDS), c4(*T.BBOX_INSIDE_WEIGHTS))
    new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    out_left, out_right, labels = new((B, S, 5)), new((B, S, 5)), new((B, S), torch.int32)
    tgt_left, tgt_right, dim_orien = new((B, S, 4)), new((B, S, 4)), new((B, S, 5))
    kpts_targets, kpts_weight = new((B, S, 3), torch.int32), new((B, S, 3))
    inside_w, outside_w = new((B, S, 4)), new((B, S, 4))
    status = new((B,), torch.int32)
    keep_inds = new((B, S), torch.int32) if want_keep_inds else None
    L = _lib.lib()
    ws_bytes = L.srcnn_proposal_targets_workspace_bytes(B, R, K)
    ws = _lib.workspace(ws_bytes, dev, key="proposal_targets")
    _lib.check(L.srcnn_proposal_targets(_lib.ptr(rois_left), _lib.ptr(rois_right), B, R, _lib.ptr(gt_left), _lib.ptr(gt_right),
                                        _lib.ptr(gt_dim_orien), _lib.ptr(gt_kpts), K, _lib.ptr(fg_keys), _lib.ptr(u), params,
                                        _lib.ptr(out_left), _lib.ptr(out_right), _lib.ptr(labels), _lib.ptr(tgt_left),
                                        _lib.ptr(tgt_right), _lib.ptr(dim_orien), _lib.ptr(kpts_targets), _lib.ptr(kpts_weight),
                                        _lib.ptr(inside_w), _lib.ptr(outside_w), _lib.ptr(status), _lib.ptr(keep_inds),
                                        ws.data_ptr(), ws_bytes, _lib.stream()), "srcnn_proposal_targets")
    return (out_left, out_right, labels, tgt_left, tgt_right, dim_orien, kpts_targets, kpts_weight, inside_w, outside_w, status,
            keep_inds)


class _ProposalTargetLayer(nn.Module):
    """Assign object detection proposals to ground-truth targets: classification labels, box / dimension / keypoint targets."""

    def __init__(self, nclasses, generator=None, batch_size=None, fg_fraction=None):
        super(_ProposalTargetLayer, self).__init__()
        self._num_classes = nclasses
        self._generator = generator
        self._batch_size = batch_size
        self._fg_fraction = fg_fraction
        if not (cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED and cfg.TRAIN.DIM_NORMALIZE_TARGETS_PRECOMPUTED):
            raise NotImplementedError("the kernel always normalises its targets (the reference's configuration)")
        self.status = None
        self.keep_inds = None

    def forward(self, all_rois_left, all_rois_right, gt_boxes_left, gt_boxes_right, gt_dim_orien, gt_kpts, num_boxes,
                generator=None, fg_keys=None, u=None, batch_size=None, fg_fraction=None, want_keep_inds=False):
        """Returns rois_left, rois_right (B, S, 5), labels (B, S) int32, bbox_targets_left, bbox_targets_right (B, S, 4),
        dim_orien_targets (B, S, 5), kpts_targets (B, S, 3) int32, kpts_weight (B, S, 3), bbox_inside_weights,
        bbox_outside_weights (B, S, 4) -- proposal_target_layer.py:66-67.  `self.status` (B) int32 stays on the device."""
        if not gt_boxes_left.is_cuda:
            raise NotImplementedError
        dev = gt_boxes_left.device
        B, R, K = int(all_rois_left.shape[0]), int(all_rois_left.shape[1]), int(gt_boxes_left.shape[1])
        pick = lambda *vs: next(v for v in vs if v is not None)
        rois_per_image = int(pick(batch_size, self._batch_size, cfg.TRAIN.BATCH_SIZE))                        # :55-56, one image
        fg_rois = int(np.round(pick(fg_fraction, self._fg_fraction, cfg.TRAIN.FG_FRACTION) * rois_per_image))   # :57
        gen = generator if generator is not None else self._generator
        if fg_keys is None:
            fg_keys = draw_keys((B, R + K), dev, gen)
        if u is None:
            u = torch.rand((B, rois_per_image), dtype=torch.float64, device=dev, generator=gen)
        out = proposal_targets(all_rois_left, all_rois_right, gt_boxes_left, gt_boxes_right, gt_dim_orien, gt_kpts, fg_keys, u,
                               rois_per_image, fg_rois, want_keep_inds=want_keep_inds)
        self.status, self.keep_inds = out[10], out[11]
        return out[:10]

    def check_status(self):
        """The reference's ValueError (proposal_target_layer.py:285), raised when the caller asks: this reads `status` back."""
        if self.status is not None and bool(self.status.any()):
            raise ValueError("bg_num_rois = 0 and fg_num_rois = 0 in image(s) %s" % self.status.nonzero().view(-1).tolist())

    def backward(self, top, propagate_down, bottom):
        """This layer does not propagate gradients."""
        pass

    def reshape(self, bottom, top):
        """Reshaping happens during the call to forward."""
        pass
