"""`RoIAlignFunction` - reference lib/model/roi_align/functions/roi_align.py:7-47 (forward and backward)."""
import torch

from .... import _lib


def _forward(features, rois, ah, aw, scale):
    b, c, h, w = features.shape
    n = int(rois.shape[0])
    out = torch.zeros((n, c, ah, aw), dtype=torch.float32, device=features.device)   # zero-filled as functions/roi_align.py:22
    # return value (1 ok / 0 bad roi shape) is ignored by the reference caller too
    _lib.lib().roi_align_forward_cuda(ah, aw, scale, features.data_ptr(), b, c, h, w, rois.data_ptr(), n,
                                      int(rois.shape[1]) if rois.dim() == 2 else 0, out.data_ptr(), _lib.stream())
    return out


def _backward(grad_output, rois, feature_size, ah, aw, scale):
    """(n, C, ah, aw) gradient -> (B, C, H, W) gradient of the features (roi_align_backward_cuda)."""
    b, c, h, w = feature_size
    grad_output = grad_output.contiguous().float()
    # the native op overwrites every element, so no zero fill (functions/roi_align.py:38-39) -- except for a bad roi shape,
    # which it refuses before any launch, leaving the tensor alone: that case keeps the reference's zeros
    good = rois.dim() == 2 and int(rois.shape[1]) == 5 and 1 <= ah <= 255 and 1 <= aw <= 255
    grad_input = (torch.empty if good else torch.zeros)((b, c, h, w), dtype=torch.float32, device=grad_output.device)
    _lib.lib().roi_align_backward_cuda(ah, aw, scale, grad_output.data_ptr(), rois.data_ptr(), int(rois.shape[0]),
                                       int(rois.shape[1]) if rois.dim() == 2 else 0, grad_input.data_ptr(), b, c, h, w,
                                       _lib.stream())
    return grad_input


class _RoIAlign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, rois, ah, aw, scale):
        ctx.save_for_backward(rois)
        ctx.geometry = (tuple(features.shape), ah, aw, scale)
        return _forward(features, rois, ah, aw, scale)

    @staticmethod
    def backward(ctx, grad_output):
        rois, = ctx.saved_tensors
        size, ah, aw, scale = ctx.geometry
        return _backward(grad_output, rois, size, ah, aw, scale), None, None, None, None


class RoIAlignFunction(object):
    """Callable with the reference's constructor / forward / backward signatures.  With grad mode on and features that
    require grad the result carries a `grad_fn` (the native backward op, roi_align_kernel.cu:94-143 as a gather with a
    defined summation order: include/srcnn_hip.h); the gradient with respect to `rois` is None, as in the reference."""

    def __init__(self, aligned_height, aligned_width, spatial_scale):
        self.aligned_width = int(aligned_width)
        self.aligned_height = int(aligned_height)
        self.spatial_scale = float(spatial_scale)
        self.rois = None
        self.feature_size = None

    def forward(self, features, rois):
        if not features.is_cuda:
            raise NotImplementedError          # functions/roi_align.py:28-29
        differentiable = torch.is_grad_enabled() and features.requires_grad
        features = features.contiguous().float()
        rois = rois.contiguous().float()
        self.rois = rois.detach()                      # functions/roi_align.py:16-17
        self.feature_size = tuple(features.shape)
        if differentiable:
            return _RoIAlign.apply(features, self.rois, self.aligned_height, self.aligned_width, self.spatial_scale)
        return _forward(features, rois, self.aligned_height, self.aligned_width, self.spatial_scale)

    def backward(self, grad_output):
        """The reference's explicit method (functions/roi_align.py:33-47): after a forward, (grad_input, None)."""
        assert self.feature_size is not None and grad_output.is_cuda
        return _backward(grad_output, self.rois, self.feature_size, self.aligned_height, self.aligned_width,
                         self.spatial_scale), None

    __call__ = forward
