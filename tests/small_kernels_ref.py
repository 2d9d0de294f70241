"""Plain references of the small kernels around the conv engines (csrc/heads.hip, pool_resize.hip, rpn_proposal.hip), for
tests/test_small_kernels_gpu.py.  numpy / torch on the CPU, float64 wherever arithmetic is involved; nothing here imports the
product package.  tests/test_small_kernels_ref_cpu.py pins every function below against independent CPU code (torch.softmax,
F.max_pool2d, F.interpolate, oracle.postprocess, oracle.ops.nms, numpy.float16), so that a wrong reference cannot bless a
wrong kernel.

Error bounds live here too, next to the arithmetic they describe: they are DERIVED from the float32 evaluation model (one
rounding of 2^-24 relative per operation, the device expf at the 1 ulp ROCm documents for it), never tuned to what the kernels
return.
"""
import numpy as np
import torch

U = 2.0 ** -24              # float32 unit roundoff (half an ulp, relative)
ULP = 2.0 ** -23            # one float32 ulp, relative
F32_MIN_NORMAL = 2.0 ** -126


# ------------------------------------------------------------------------------------------------ softmax
def softmax_rows(x):
    """Row softmax of float32 logits in float64, max-shifted.  x (rows, cols) -> float64 (rows, cols)."""
    x = np.asarray(x, np.float64)
    d = x - x.max(axis=1, keepdims=True)
    e = np.exp(d)
    return e / e.sum(axis=1, keepdims=True)


def softmax_bound(x):
    """Per-element bound on |float32 softmax - softmax_rows(x)| for the kernels' evaluation p = expf(x - m) / sum_k expf(x_k - m)
    (softmax_rows_kernel, box_head_tail_kernel, kpts_tail_kernel, rpn_score_kernel; sequential float32 sum).

    relative:  (|x - m| + cols + 3) * 2^-23, from
      * d = x - m is one float32 subtraction: |error| <= |d| 2^-24, which the exponential turns into a RELATIVE error of
        |d| 2^-24 -- counted as |d| 2^-23, twice what is needed;
      * the numerator's expf: 1 ulp (ROCm's documented maximum for expf) = 2^-23;
      * the denominator: every term is positive and carries (|d_k| 2^-24 + 2^-23); since the largest term is expf(0) = 1
        exactly, sum >= 1 and sum_k e_k |d_k| <= (cols - 1) / e, so the terms' own errors weigh at most
        ((cols - 1) / e) 2^-24 + 2^-23 relative to the sum; the cols - 1 sequential additions add (cols - 1) 2^-24.  Together
        below (cols - 1) 2^-23 + 2^-23 = cols 2^-23;
      * the (correctly rounded) division: 2^-24;
      so the constant is 1 (numerator expf) + 0.5 (division) + 1.5 of slack for the second-order products of the above.
    absolute: 2^-126.  A probability below the smallest normal float32 has no relative accuracy (expf underflows gradually or
      flushes to zero), so such results are held to the smallest normal instead."""
    x = np.asarray(x, np.float64)
    cols = x.shape[1]
    d = np.abs(x - x.max(axis=1, keepdims=True))
    return (d + cols + 3.0) * ULP * softmax_rows(x) + F32_MIN_NORMAL


def kpts_tail(logits):
    """stereo_rcnn.py:260-271 after the kpts_class conv: logits (n, G, G, 6) NHWC (n, h, w, channel) -> sum over h, then three
    softmaxes: over the 4 G bins of channels 0-3 in (channel, w) order, over the G bins of channel 4, over those of channel 5.
    Returns float64 (kpts_prob (n, 4G), left_prob (n, G), right_prob (n, G)) and the summed columns (n, 6, G)."""
    lg = np.asarray(logits, np.float64)
    n, G = lg.shape[0], lg.shape[1]
    col = lg.sum(axis=1).transpose(0, 2, 1)          # (n, w, ch) -> (n, ch, w)
    k = softmax_rows(col[:, :4, :].reshape(n, 4 * G))
    return k, softmax_rows(col[:, 4, :]), softmax_rows(col[:, 5, :]), col


# ------------------------------------------------------------------------------------------------ SPLIT16
def split16_halves(x):
    """The two halves of the SPLIT16 activation format for float32 values: hi = float16(x), lo = float16(x - float32(hi)), both
    round-to-nearest-even (numpy's float16 conversion)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split16_pack(x):
    """float32 (..., C), C % 8 == 0 -> the SPLIT16 bytes as a float32-typed array of the same shape.  Layout (restated from
    csrc/conv_common.h): per pixel, every group of 8 channels occupies the 32 bytes its 8 floats had, as 8 float16 hi followed
    by 8 float16 lo."""
    x = np.ascontiguousarray(x, np.float32)
    C = x.shape[-1]
    assert C % 8 == 0
    hi, lo = split16_halves(x.reshape(-1, C // 8, 8))
    raw = np.stack([hi, lo], axis=2)                 # (pixels, groups, {hi, lo}, 8) float16 = 32 bytes per group
    return np.ascontiguousarray(raw).view(np.float32).reshape(x.shape)


def split16_unpack(raw):
    """Inverse view of split16_pack: float32-typed SPLIT16 bytes (..., C) -> float32(hi) + float32(lo), added in float32."""
    raw = np.ascontiguousarray(raw, np.float32)
    C = raw.shape[-1]
    h = raw.reshape(-1, C // 8, 8).view(np.float16).reshape(-1, C // 8, 2, 8)
    with np.errstate(invalid='ignore'):
        v = h[:, :, 0, :].astype(np.float32) + h[:, :, 1, :].astype(np.float32)
    return v.reshape(raw.shape)


def split16_step(v):
    """One step of the split at value v: lo is a float16 of a residual of at most half a float16 ulp of v (|v| 2^-11), so lo's
    own spacing is at most 2^-10 of that = |v| 2^-21, and never finer than the float16 subnormal spacing 2^-24."""
    return np.abs(np.asarray(v, np.float64)) * 2.0 ** -21 + 2.0 ** -24


# ------------------------------------------------------------------------------------------------ pooling / resize / layout
def ceil_pool_out(n):
    """Output length of a 3-wide, stride-2, unpadded, ceil-mode pooling (PyTorch's rule: the last window must START inside)."""
    o = -(-(n - 3) // 2) + 1
    if (o - 1) * 2 >= n:
        o -= 1
    return max(o, 1)


def maxpool3x3s2_ceil(x):
    """x (B, H, W, C) NHWC float32 -> (B, OH, OW, C): maximum over the 3x3 window at (2 oh, 2 ow), clipped at the border."""
    x = np.asarray(x, np.float32)
    B, H, W, C = x.shape
    OH, OW = ceil_pool_out(H), ceil_pool_out(W)
    y = np.empty((B, OH, OW, C), np.float32)
    for oh in range(OH):
        for ow in range(OW):
            y[:, oh, ow] = x[:, 2 * oh:min(2 * oh + 3, H), 2 * ow:min(2 * ow + 3, W)].reshape(B, -1, C).max(axis=1)
    return y


def _taps(n_in, n_out):
    """align_corners source taps of every output index, index arithmetic in float32 as ATen's float path and the kernel do it:
    r = (in - 1) / (out - 1), s = r * i, i0 = trunc(s), lambda1 = s - i0, lambda0 = 1 - lambda1 (all float32)."""
    r = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    s = (r * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = s.astype(np.int64)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def upsample_add(top, lateral):
    """top (B, TH, TW, C), lateral (B, H, W, C) NHWC -> float64 bilinear(top -> (H, W), align_corners=True) + lateral, and the
    magnitude sum |w v| over the four taps + |lateral| that the rounding bound scales with."""
    top, lat = np.asarray(top, np.float64), np.asarray(lateral, np.float64)
    H, W = lat.shape[1:3]
    h0, h1, a0, a1 = _taps(top.shape[1], H)
    w0, w1, b0, b1 = _taps(top.shape[2], W)
    a0, a1 = a0[None, :, None, None], a1[None, :, None, None]
    b0, b1 = b0[None, None, :, None], b1[None, None, :, None]
    t00, t01 = top[:, h0][:, :, w0], top[:, h0][:, :, w1]
    t10, t11 = top[:, h1][:, :, w0], top[:, h1][:, :, w1]
    y = a0 * (b0 * t00 + b1 * t01) + a1 * (b0 * t10 + b1 * t11) + lat
    mag = a0 * (b0 * np.abs(t00) + b1 * np.abs(t01)) + a1 * (b0 * np.abs(t10) + b1 * np.abs(t11)) + np.abs(lat)
    return y, mag


def upsample_add_f32(top, lateral):
    """float32 restatement of the shared tap and blend (csrc/bilinear_tap.h: align_ratio, align_tap, align_blend) followed by
    the lateral, operation by operation: (l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d)) + lateral with every product
    and sum rounded to float32 on its own (numpy's float32 arithmetic; the library is built with -ffp-contract=off).
    top (B, TH, TW, C), lateral (B, H, W, C) float32 -> float32 (B, H, W, C)."""
    top, lat = np.asarray(top, np.float32), np.asarray(lateral, np.float32)
    H, W = lat.shape[1:3]
    f = lambda a: a.astype(np.float32)               # exact: _taps computed them in float32
    h0, h1, a0, a1 = _taps(top.shape[1], H)
    w0, w1, b0, b1 = _taps(top.shape[2], W)
    a0, a1 = f(a0)[None, :, None, None], f(a1)[None, :, None, None]
    b0, b1 = f(b0)[None, None, :, None], f(b1)[None, None, :, None]
    t00, t01 = top[:, h0][:, :, w0], top[:, h0][:, :, w1]
    t10, t11 = top[:, h1][:, :, w0], top[:, h1][:, :, w1]
    y = (a0 * (b0 * t00 + b1 * t01) + a1 * (b0 * t10 + b1 * t11)) + lat
    assert y.dtype == np.float32
    return y


def upsample_add_bound(mag):
    """|float32 kernel - upsample_add| <= 6 * 2^-24 * (sum |w v| + |lateral|): the weights are the same float32 numbers on
    both sides; a tap's value passes through at most five float32 roundings on its way to the result (w product, inner sum,
    h product, outer sum, + lateral), the lateral through one; one more unit for the second-order terms."""
    return 6.0 * U * np.asarray(mag, np.float64)


def subsample2(x):
    """MaxPool2d(1, stride=2) on NHWC: every second row and column."""
    return np.ascontiguousarray(np.asarray(x)[:, ::2, ::2, :])


def nchw_to_nhwc(x):
    return np.ascontiguousarray(np.asarray(x).transpose(0, 2, 3, 1))


def nhwc_to_nchw(x):
    return np.ascontiguousarray(np.asarray(x).transpose(0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------ RPN score
def rpn_score(head, level_offset=0, a_total=None):
    """head (B, hw, >= 24): channels [0, 6) class logits, [6, 24) deltas.  stereo_rpn.py:81-91 -- the softmax pairs channel c
    (background) with channel c + 3 (foreground), and the NHWC flatten then reads CONSECUTIVE channels as an anchor's pair:
    anchor a of location loc gets (p[2a], p[2a + 1]) of the six probabilities and deltas 6a .. 6a + 5.
    -> float64 probs (B, 3 hw, 2), float32 deltas (B, 3 hw, 6), the softmax bound (B, 3 hw, 2)."""
    head = np.asarray(head, np.float32)
    B, hw = head.shape[:2]
    s = head[:, :, :6].astype(np.float64)
    p = np.empty((B, hw, 6), np.float64)
    bound = np.empty((B, hw, 6), np.float64)
    for c in range(3):
        pair = s[:, :, [c, c + 3]].reshape(-1, 2)
        p[:, :, [c, c + 3]] = softmax_rows(pair).reshape(B, hw, 2)
        bound[:, :, [c, c + 3]] = softmax_bound(pair).reshape(B, hw, 2)
    return p.reshape(B, hw * 3, 2), head[:, :, 6:24].reshape(B, hw * 3, 6).copy(), bound.reshape(B, hw * 3, 2)


# ------------------------------------------------------------------------------------------------ decode
def decode_detections(rois_l, rois_r, bbox_pred, dim_pred, kpts_prob, left_prob, right_prob, im_info, n_cls, G):
    """demo.py:144-218 through the oracle (oracle.postprocess.decode_detections) for any class count and keypoint grid: the
    oracle reads the grid from its config module, which is set to G for the duration of the call.
    rois (n, 5), bbox_pred (n, 6 n_cls), dim_pred (n, 5 n_cls), probabilities (n, 4G) / (n, G), im_info (3,) -> dict of numpy."""
    from oracle import config as ocfg
    from oracle import postprocess as opost
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    out = {'cls_prob': torch.zeros(1, len(rois_l), n_cls), 'rois_left': t(rois_l)[None], 'rois_right': t(rois_r)[None],
           'bbox_pred': t(bbox_pred)[None], 'dim_orien_pred': t(dim_pred)[None], 'kpts_prob': t(kpts_prob),
           'left_border_prob': t(left_prob), 'right_border_prob': t(right_prob)}
    saved = ocfg.KPTS_GRID
    ocfg.KPTS_GRID = G
    try:
        det = opost.decode_detections(out, t(im_info).view(1, 3), n_classes=n_cls)
    finally:
        ocfg.KPTS_GRID = saved
    return {k: det[k].numpy() for k in ('boxes_left', 'boxes_right', 'dim_orien', 'kpts')}


def argmax_first(p):
    """Index of the FIRST maximum of each row (what torch.max returns on the CPU, pinned in the CPU test)."""
    return np.argmax(np.asarray(p), axis=1)


def pack_detections(scores, boxes_l, boxes_r, dim_orien, kpts, keep_idx, num, j, rec_cols, flag=0.0):
    """include/srcnn_hip.h, srcnn_pack_detections: (n + 1, rec_cols) float32; row 0 = [count, range flag, 0 ...]; row 1 + r =
    [score, left box 4, right box 4, dim_orien 5, kpts 5, roi index, 0 ...] of the r-th kept roi; rows past the count zero."""
    n = scores.shape[0]
    rec = np.zeros((n + 1, rec_cols), np.float32)
    rec[0, 0], rec[0, 1] = num, flag
    for r in range(num):
        i = int(keep_idx[r])
        rec[1 + r, 0] = scores[i, j]
        rec[1 + r, 1:5] = boxes_l[i, 4 * j:4 * j + 4]
        rec[1 + r, 5:9] = boxes_r[i, 4 * j:4 * j + 4]
        rec[1 + r, 9:14] = dim_orien[i, 5 * j:5 * j + 5]
        rec[1 + r, 14:19] = kpts[i]
        rec[1 + r, 19] = i
    return rec


# ------------------------------------------------------------------------------------------------ class NMS
def class_nms(scores, boxes, j, score_thresh, nms_thresh, nms=None):
    """demo.py:231-251 for class j: score > thresh (strict), stable descending sort (ties by ascending roi index), greedy NMS
    on the left boxes of that class, mapped back to roi indices.  scores (n, n_cls), boxes (n, 4 n_cls) float32.
    -> keep_idx (n,) int32 padded with -1, num."""
    if nms is None:
        from oracle.ops import nms
    scores, boxes = np.asarray(scores, np.float32), np.asarray(boxes, np.float32)
    n = scores.shape[0]
    s = scores[:, j]
    inds = np.nonzero(s > np.float32(score_thresh))[0]
    order = inds[np.argsort(-s[inds].astype(np.float64), kind='stable')]
    keep_idx = np.full((n,), -1, np.int32)
    if order.size == 0:
        return keep_idx, 0
    dets = np.concatenate([boxes[order, 4 * j:4 * j + 4], s[order, None]], 1).astype(np.float32)
    keep = nms(dets, nms_thresh)
    keep_idx[:len(keep)] = order[keep]
    return keep_idx, len(keep)
