"""The training losses of Stereo R-CNN on the fused HIP kernels (srcnn_cross_entropy, srcnn_smooth_l1 and their backwards).

Reference: lib/model/rpn/stereo_rpn.py:113-136 (`rpn_losses`), lib/model/stereo_rcnn/stereo_rcnn.py:204-230, 274-311
(`rcnn_losses`), trainval_net.py:214-219 (`multi_task_loss`).  The functions take exactly the tensors the anchor / proposal
target layers hand over.  Nothing here waits for the device: the reference's nonzero() + index_select over the RPN labels is the
kernel's ignore rule, its three `torch.sum(weight).data[0] < 1` reads are a comparison inside the kernel, and the backward reads
the upstream gradient and the normaliser from device memory.  DELIBERATE DIFFERENCE: with no kept row a cross-entropy term is 0
with a zero gradient (the reference gives NaN or raises).  CPU tensors raise NotImplementedError, as the project's other ops.
"""
import torch

from ... import _lib
from ..utils.net_utils import _workspace, smooth_l1


def _ce_forward(logits_ptr, rows, cols, stride, labels, weights, mode, device):
    loss = torch.empty((), dtype=torch.float32, device=device)
    norm = torch.empty(1, dtype=torch.float32, device=device)      # kept count / weight sum: stays on the device for the backward
    ws, ws_bytes = _workspace(rows, device)
    _lib.check(_lib.lib().srcnn_cross_entropy(logits_ptr, rows, cols, stride, _lib.ptr(labels), _lib.ptr(weights), mode,
                                              loss.data_ptr(), norm.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream()),
               "srcnn_cross_entropy")
    return loss, norm


def _ce_backward(logits_ptr, rows, cols, stride, labels, weights, mode, norm, grad_loss, grad_ptr, grad_stride):
    g = grad_loss.detach().float().contiguous()                    # a device scalar: the kernel reads it there
    _lib.check(_lib.lib().srcnn_cross_entropy_backward(logits_ptr, rows, cols, stride, _lib.ptr(labels), _lib.ptr(weights), mode,
                                                       norm.data_ptr(), g.data_ptr(), grad_ptr, grad_stride, _lib.stream()),
               "srcnn_cross_entropy_backward")


def _int32(t):
    return t.detach().reshape(-1).to(torch.int32).contiguous()


def _float32(t):
    return None if t is None else t.detach().reshape(-1).float().contiguous()


class _CrossEntropyRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, weights, mode):
        rows, cols = int(logits.shape[0]), int(logits.shape[1])
        stride = int(logits.stride(0)) if rows > 1 else cols
        loss, norm = _ce_forward(logits.data_ptr(), rows, cols, stride, labels, weights, mode, logits.device)
        ctx.save_for_backward(logits, labels, weights, norm)
        ctx.meta = (rows, cols, stride, mode)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        logits, labels, weights, norm = ctx.saved_tensors
        rows, cols, stride, mode = ctx.meta
        grad = torch.empty((rows, cols), dtype=torch.float32, device=logits.device)     # every element is written by the kernel
        _ce_backward(logits.data_ptr(), rows, cols, stride, labels, weights, mode, norm, grad_loss, grad.data_ptr(), cols)
        return grad, None, None, None


def cross_entropy_rows(logits, labels, weights=None):
    """Cross-entropy over the rows of `logits` (rows, cols).  A row is kept when 0 <= label < cols; any other label (-1, the
    RPN's "don't care") is ignored and never used as an index.
      weights None : the mean over the kept rows -- the reference's nonzero + index_select + F.cross_entropy (stereo_rpn.py:115-119);
      weights (rows): S = sum(loss_i w_i), W = sum(w_i) over the kept rows; S if W < 1 else S / W (stereo_rcnn.py:294-310).
    Rows of a view with a row stride (columns contiguous) are read in place."""
    if not logits.is_cuda:
        raise NotImplementedError
    assert logits.dim() == 2, "logits must be (rows, cols)"
    if logits.dtype != torch.float32:
        logits = logits.float()
    rows, cols = logits.shape
    if rows > 0 and not (logits.stride(1) == 1 and (rows == 1 or logits.stride(0) >= cols)):
        logits = logits.contiguous()
    mode = _lib.CE_MEAN_KEPT if weights is None else _lib.CE_WEIGHTED
    return _CrossEntropyRows.apply(logits, _int32(labels), _float32(weights), mode)


class _KptsCrossEntropy(torch.autograd.Function):
    """The keypoint, left-border and right-border terms (stereo_rcnn.py:264-270, 292-310) on kpts_pred_all (n, 6, G) in place:
    rows of 4G, G and G logits with row stride 6G, no .contiguous() copies; the backward's three launches write the three
    column ranges of ONE (n, 6, G) gradient, every element once."""

    @staticmethod
    def forward(ctx, kpts_pred_all, labels3, weights3):
        n, six, G = (int(v) for v in kpts_pred_all.shape)
        base, dev = kpts_pred_all.data_ptr(), kpts_pred_all.device
        parts = ((0, 4 * G), (4 * G, G), (5 * G, G))
        out = [_ce_forward(base + 4 * off, n, cols, 6 * G, labels3[i], weights3[i], _lib.CE_WEIGHTED, dev)
               for i, (off, cols) in enumerate(parts)]
        ctx.save_for_backward(kpts_pred_all, labels3, weights3, *[norm for _, norm in out])
        ctx.parts = parts
        return tuple(loss for loss, _ in out)

    @staticmethod
    def backward(ctx, *grad_losses):
        kpts_pred_all, labels3, weights3 = ctx.saved_tensors[:3]
        norms = ctx.saved_tensors[3:]
        n, six, G = (int(v) for v in kpts_pred_all.shape)
        grad = torch.empty_like(kpts_pred_all)
        for i, (off, cols) in enumerate(ctx.parts):
            g = grad_losses[i] if grad_losses[i] is not None else torch.zeros((), dtype=torch.float32, device=grad.device)
            _ce_backward(kpts_pred_all.data_ptr() + 4 * off, n, cols, 6 * G, labels3[i], weights3[i], _lib.CE_WEIGHTED, norms[i], g,
                         grad.data_ptr() + 4 * off, 6 * G)
        return grad, None, None


def rpn_losses(rpn_cls_score_alls, rpn_bbox_pred_alls_left_right, rpn_label, targets_left, targets_right, inside_w, outside_w):
    """(rpn_loss_cls, rpn_loss_box_left_right) of stereo_rpn.py:113-136.
    rpn_cls_score_alls (B, A, 2), rpn_bbox_pred_alls_left_right (B, A, 6); from the anchor target layer: rpn_label (B x A values,
    -1 = don't care), targets_left / targets_right (B, A, 4), inside_w / outside_w (B, A) per-anchor weights."""
    if not rpn_cls_score_alls.is_cuda:
        raise NotImplementedError
    B, A = int(rpn_bbox_pred_alls_left_right.shape[0]), int(rpn_bbox_pred_alls_left_right.shape[1])
    rpn_loss_cls = cross_entropy_rows(rpn_cls_score_alls.reshape(-1, 2), rpn_label)
    # stereo_rpn.py:124-127: [left dx dy dw dh | right dx | right dw]
    targets = torch.cat((targets_left.view(B, A, 4), targets_right.view(B, A, 4)[:, :, 0:1], targets_right.view(B, A, 4)[:, :, 2:3]), 2)
    # stereo_rpn.py:129-132 expands the per-anchor weights to 6 columns: the kernel takes them per row; dim=[1] over (B, A, 6)
    # leaves B * 6 values for .mean()
    inside = inside_w.view(B, A).unsqueeze(2).expand(B, A, 6)
    outside = outside_w.view(B, A).unsqueeze(2).expand(B, A, 6)
    rpn_loss_box = smooth_l1(rpn_bbox_pred_alls_left_right.view(B, A, 6), targets, inside, outside, sigma=3, divisor=B * 6)
    return rpn_loss_cls, rpn_loss_box


def _six_from_four(w4):
    """stereo_rcnn.py:209-215: [w0 w1 w2 w3 | w0 w1]."""
    w4 = w4.reshape(-1, 4)
    return torch.cat((w4, w4[:, 0:2]), 1)


def rcnn_losses(cls_score, bbox_pred, dim_orien_pred, kpts_pred_all, rois_label, rois_target_left, rois_target_right,
                rois_target_dim_orien, kpts_label_all, kpts_weight_all, rois_inside_ws4, rois_outside_ws4):
    """(RCNN_loss_cls, RCNN_loss_bbox, RCNN_loss_dim_orien, RCNN_loss_kpts) of stereo_rcnn.py:204-230, 274-311.
    cls_score (n, n_cls), bbox_pred (n, 6 n_cls) and dim_orien_pred (n, 5 n_cls) as the heads give them (the gather by
    rois_label happens in the kernel), kpts_pred_all (n, 6, G) after .sum(2); from the proposal target layer: rois_label (n
    values), rois_target_left / _right (.., 4), rois_target_dim_orien (.., 5), kpts_label_all / kpts_weight_all (.., 3),
    rois_inside_ws4 / rois_outside_ws4 (.., 4)."""
    if not cls_score.is_cuda:
        raise NotImplementedError
    n, n_cls = int(cls_score.shape[0]), int(cls_score.shape[1])
    label = _int32(rois_label)
    loss_cls = cross_entropy_rows(cls_score, label)
    left, right = rois_target_left.reshape(n, 4), rois_target_right.reshape(n, 4)
    target6 = torch.cat((left, right[:, 0:1], right[:, 2:3]), 1)
    loss_bbox = smooth_l1(bbox_pred, target6, _six_from_four(rois_inside_ws4), _six_from_four(rois_outside_ws4),
                          selector=label, n_sel=int(bbox_pred.shape[1]) // 6)
    loss_dim_orien = smooth_l1(dim_orien_pred, rois_target_dim_orien.reshape(n, 5), selector=label,
                               n_sel=int(dim_orien_pred.shape[1]) // 5)
    labels3 = kpts_label_all.detach().reshape(n, 3).t().to(torch.int32).contiguous()
    weights3 = kpts_weight_all.detach().reshape(n, 3).t().float().contiguous()
    kp = kpts_pred_all if kpts_pred_all.dtype == torch.float32 else kpts_pred_all.float()
    loss_kpts, loss_left, loss_right = _KptsCrossEntropy.apply(kp.contiguous(), labels3, weights3)
    return loss_cls, loss_bbox, loss_dim_orien, (loss_kpts + loss_left + loss_right) / 3.0


def multi_task_loss(losses, uncert):
    """trainval_net.py:214-219: sum_i L_i exp(-u_i) + u_i over the six terms (plain torch: six scalars)."""
    total = 0
    for i, loss in enumerate(losses):
        total = total + loss * torch.exp(-uncert[i]) + uncert[i]
    return total
