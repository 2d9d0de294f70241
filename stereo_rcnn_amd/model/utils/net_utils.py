"""`_smooth_l1_loss` - reference lib/model/utils/net_utils.py:79-99, on the fused HIP kernels (srcnn_smooth_l1 and its backward).

The reference composes the loss from about ten eager tensor operations; here the forward is two launches and the backward one,
nothing is read back to the host, and the sum has a defined order (include/srcnn_hip.h), so a step is repeatable bit for bit.
"""
import torch

from ... import _lib, optim


def clip_gradient(model, clip_norm):
    """Reference signature and effect (net_utils.py:37-49): every gradient of the model's trainable parameters is multiplied in
    place by clip_norm / max(total L2 norm, clip_norm).  One norm pass and one scaling pass on the device (srcnn_grad_norm,
    srcnn_grad_scale); the coefficient is never read back.  Returns the norm as a 0-d device tensor.  Parameters without a
    gradient are passed over (the reference would raise on them).  `optim.SGD.step(clip_norm=...)` folds the same coefficient
    into the update and needs no call of this function."""
    grads = [p.grad for p in model.parameters() if p.requires_grad and p.grad is not None]
    if not grads:
        raise ValueError("clip_gradient: the model has no gradients")
    if not grads[0].is_cuda:
        raise NotImplementedError
    out = optim.grad_norm(grads, clip_norm)
    optim.scale_grads(grads, out[1:])
    return out[0]


def adjust_learning_rate(optimizer, decay=0.1):
    """net_utils.py:70-73: every group's learning rate times `decay`."""
    for param_group in optimizer.param_groups:
        param_group['lr'] = decay * param_group['lr']


def save_checkpoint(state, filename):
    """net_utils.py:76-77."""
    torch.save(state, filename)


def _workspace(rows, device):
    nbytes = _lib.lib().srcnn_loss_workspace_bytes(int(rows))
    buf = _lib.workspace(nbytes, device, key="loss")
    return buf, buf.numel()


def _weight_arg(w, pred):
    """(tensor, per_row) for a weight of pred's shape: a view expanded along the last dimension (stride 0) is passed as one
    weight per row and never materialised (stereo_rpn.py:129-132 expands a per-anchor weight to 6 columns)."""
    if w is None:
        return None, 0
    if tuple(w.shape) != tuple(pred.shape):
        w = w.expand_as(pred)
    w = w.detach()
    if w.dtype != torch.float32:
        w = w.float()
    if pred.dim() >= 1 and pred.shape[-1] > 1 and w.stride(-1) == 0:
        return w[..., 0].contiguous(), 1
    return w.contiguous(), 0


class _SmoothL1(torch.autograd.Function):
    """loss = sum(w_out * smooth_l1(w_in * (pred[:, sel] - target))) / divisor; gradient to `pred` only."""

    @staticmethod
    def forward(ctx, pred, target, w_in, w_in_per_row, w_out, w_out_per_row, selector, n_sel, rows, D, sigma, divisor):
        L = _lib.lib()
        dev = pred.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        norm = torch.empty(1, dtype=torch.float32, device=dev)         # the normaliser stays on the device for the backward
        ws, ws_bytes = _workspace(rows, dev)
        _lib.check(L.srcnn_smooth_l1(pred.data_ptr(), _lib.ptr(selector), n_sel, target.data_ptr(), _lib.ptr(w_in), w_in_per_row,
                                     _lib.ptr(w_out), w_out_per_row, rows, D, sigma, divisor, loss.data_ptr(),
                                     norm.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream()), "srcnn_smooth_l1")
        ctx.save_for_backward(pred, target, w_in, w_out, selector, norm)
        ctx.meta = (w_in_per_row, w_out_per_row, n_sel, rows, D, sigma)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        pred, target, w_in, w_out, selector, norm = ctx.saved_tensors
        w_in_per_row, w_out_per_row, n_sel, rows, D, sigma = ctx.meta
        g = grad_loss.detach().float().contiguous()                    # stays on the device: the kernel reads it there
        grad = torch.empty_like(pred)                                  # every element is written by the kernel
        _lib.check(_lib.lib().srcnn_smooth_l1_backward(pred.data_ptr(), _lib.ptr(selector), n_sel, target.data_ptr(), _lib.ptr(w_in),
                                                       w_in_per_row, _lib.ptr(w_out), w_out_per_row, rows, D, sigma,
                                                       norm.data_ptr(), g.data_ptr(), grad.data_ptr(), _lib.stream()),
                   "srcnn_smooth_l1_backward")
        return (grad,) + (None,) * 11


def smooth_l1(pred, target, inside_weights=None, outside_weights=None, sigma=1.0, divisor=None, selector=None, n_sel=1):
    """The op behind `_smooth_l1_loss`.  pred (..., n_sel * D), target (..., D); `selector` (int, one per row) picks the slice
    [sel * D, sel * D + D) of a row -- the torch.gather by rois_label of stereo_rcnn.py:274-280 -- and a selector outside
    [0, n_sel) drops the row.  The sum over every element is divided by `divisor` (default: the number of rows)."""
    if not pred.is_cuda:
        raise NotImplementedError
    D = int(target.shape[-1]) if target.dim() else 1
    rows = target.numel() // max(D, 1)
    assert pred.numel() == rows * n_sel * D, "pred must be (rows, n_sel * D)"
    if divisor is None:
        divisor = rows
    pred32 = pred if pred.dtype == torch.float32 else pred.float()
    pred2 = pred32.contiguous().view(rows, n_sel * D)
    target2 = target.detach().float().contiguous().view(rows, D)
    w_in, in_per_row = _weight_arg(inside_weights, target)
    w_out, out_per_row = _weight_arg(outside_weights, target)
    if selector is not None:
        selector = selector.detach().reshape(-1).to(torch.int32).contiguous()
    return _SmoothL1.apply(pred2, target2, w_in, in_per_row, w_out, out_per_row, selector, int(n_sel), int(rows), D, float(sigma),
                           float(divisor))


def _smooth_l1_loss(bbox_pred, bbox_targets, bbox_inside_weights=None, bbox_outside_weights=None, sigma=1.0, dim=[1]):
    """Reference signature and result (net_utils.py:79-99): the element losses are summed over `dim` and the rest is averaged,
    i.e. the sum over everything divided by numel / prod(shape[dim]) -- for (B, A, 6) RPN predictions and dim=[1] that is
    B * 6, not B * A, as in the reference."""
    if not bbox_pred.is_cuda:
        raise NotImplementedError
    shape = tuple(bbox_pred.shape)
    summed = 1
    for i in set(int(d) % len(shape) for d in dim):
        summed *= shape[i]
    divisor = max(bbox_pred.numel() // max(summed, 1), 1)
    if tuple(bbox_targets.shape) != shape:
        bbox_targets = bbox_targets.expand(shape)
    return smooth_l1(bbox_pred, bbox_targets, bbox_inside_weights, bbox_outside_weights, sigma=sigma, divisor=divisor)
