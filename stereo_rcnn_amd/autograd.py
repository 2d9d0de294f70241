"""Differentiable convolution and linear layers on the exact-fp32 HIP engine.

Every learnable layer of the network goes through the conv engine (the ResNet and FPN convs, RPN_Conv and its heads, RCNN_top,
the linear heads, the keypoint tower).  These functions are that engine with a backward: the forward is `engine.conv2d(...,
precision='f32')`, the backward `engine.conv2d_backward` (srcnn_conv2d_backward: dx, dw, db on the fp32 MFMA; include/srcnn_hip.h
states the sums and their order).  Tensors are NCHW at the edge and NHWC inside, like the ROIAlign modules.  Nothing here waits for
the device.  CPU tensors raise NotImplementedError, as the project's other ops.
"""
import torch

from . import engine


def _bn_scale_shift(bn, eps=1e-5):
    """engine.fold_bn's factors in float64: y = conv(x, w) * scale + shift."""
    s = bn['weight'].detach().double() / torch.sqrt(bn['running_var'].detach().double() + eps)
    return s, bn['bias'].detach().double() - bn['running_mean'].detach().double() * s


class _Conv2dNHWC(torch.autograd.Function):
    """x (B, H, W, Cin), weight (Cout, KH, KW, Cin) engine layout and already BN-folded, bias (Cout) or None, residual
    (B, OH, OW, Cout) or None; all contiguous float32 on the device."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, stride, pad, relu):
        B, H, W, cin = (int(v) for v in x.shape)
        cout, kh, kw = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        cw = engine.ConvW(weight.detach(), None if bias is None else bias.detach(), kh, kw, stride, pad, relu)
        OH, OW = engine.conv_out_hw(H, W, kh, kw, stride, pad)
        y = torch.empty((B, OH, OW, cout), dtype=torch.float32, device=x.device)
        engine.conv2d(cw, x.detach(), B, H, W, y, OH, OW, residual=None if residual is None else residual.detach(),
                      precision='f32', plan=(0, 0, 0, 0, 0))
        ctx.save_for_backward(x, weight, y if relu else None)
        ctx.geom = (B, H, W, OH, OW, kh, kw, stride, pad, bool(relu), bias is not None, residual is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        B, H, W, OH, OW, kh, kw, stride, pad, relu, has_bias, has_res = ctx.geom
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        need_b, need_r = need_b and has_bias, need_r and has_res
        dy = dy.contiguous()
        want = tuple(k for k, n in (('dx', need_x), ('dw', need_w), ('db', need_b)) if n)
        # the residual branch's gradient is the masked gradient itself; without a ReLU that is dy
        g_out = torch.empty_like(dy) if (need_r and relu) else None
        res = {}
        if want or g_out is not None:
            cw = engine.ConvW(weight, None, kh, kw, stride, pad, relu)
            res = engine.conv2d_backward(cw, x, B, H, W, y, dy, OH, OW, want=want, g_out=g_out)
        return (res.get('dx'), res.get('dw'), res.get('db'), (g_out if relu else dy) if need_r else None, None, None, None)


def _check(x, weight):
    if not (x.is_cuda and weight.is_cuda):
        raise NotImplementedError
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TypeError("float32 tensors only")


class _ToNHWC(torch.autograd.Function):
    """(B, C, H, W) -> (B, H, W, C) through the library's layout kernels, both directions."""

    @staticmethod
    def forward(ctx, x):
        return engine.nchw_to_nhwc(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return engine.nhwc_to_nchw(g.contiguous())


class _ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return engine.nhwc_to_nchw(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return engine.nchw_to_nhwc(g.contiguous())


def _fold(weight_eng, bias, bn):
    """Frozen BatchNorm (the reference's set_bn_fix freezes every BN: it gets no gradient) folded as engine.fold_bn folds it --
    in float64, stored float32 -- but inside the graph: d(w * scale) / dw = scale, so the gradient with respect to the UNFOLDED
    weight is dw_folded * scale[n], and a conv bias under a BN receives db * scale[n]."""
    if bn is None:
        return weight_eng, bias
    scale, shift = _bn_scale_shift(bn)
    w = (weight_eng.double() * scale.view(-1, 1, 1, 1)).float()
    b = shift.float() if bias is None else (bias.double() * scale + shift).float()
    return w, b


def conv2d(x, weight, bias=None, stride=1, padding=0, relu=False, residual=None, bn=None):
    """relu?(bn?(conv2d(x, weight) + bias) + residual) on the exact-fp32 engine, differentiable with respect to x, weight, bias
    and residual.  x (B, Cin, H, W) with Cin a multiple of 32, weight (Cout, Cin, KH, KW) as nn.Conv2d holds it, residual
    (B, Cout, OH, OW); bn: a dict with 'weight', 'bias', 'running_mean', 'running_var' -- the frozen BatchNorm that follows the
    convolution (no gradient reaches it).  Returns (B, Cout, OH, OW)."""
    _check(x, weight)
    if int(x.shape[1]) % 32 != 0:
        raise ValueError("Cin must be a multiple of 32 (got %d)" % int(x.shape[1]))
    w, b = _fold(weight.permute(0, 2, 3, 1), bias, bn)
    r = None if residual is None else _ToNHWC.apply(residual)
    y = _Conv2dNHWC.apply(_ToNHWC.apply(x), w.contiguous(), b, r, int(stride), int(padding), bool(relu))
    return _ToNCHW.apply(y)


def linear(x, weight, bias=None, relu=False):
    """relu?(x @ weight.T + bias) as a 1x1 convolution over an (n, 1, 1, K) tensor: x (n, K), weight (out, K) as nn.Linear holds
    it.  K must be a multiple of 32."""
    _check(x, weight)
    n, K = int(x.shape[0]), int(x.shape[1])
    if K % 32 != 0:
        raise ValueError("linear: K must be a multiple of 32 (got %d)" % K)
    out = int(weight.shape[0])
    y = _Conv2dNHWC.apply(x.contiguous().view(n, 1, 1, K), weight.contiguous().view(out, 1, 1, K), bias, None, 1, 0, bool(relu))
    return y.view(n, out)
