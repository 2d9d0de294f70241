"""The 3 x f16 training forward (srcnn_conv2d_forward_f16x3, include/srcnn_hip.h) restated in numpy, its derived error bound, and
the cases of its tests.  The split arithmetic is the backward's, and so is its restatement: scale_of, split, matmul3 and the GEMM
part of the bound come from tests/conv_backward_f16x3_ref.py (one copy, as the kernels share one header).

THE SCHEME.  y = relu?(conv(x, w) + bias + residual) with the convolution as one GEMM, rows the B OH OW output pixels, K = KH KW Cin:
s_x, s_w one power of two per tensor, every product x_hi w_hi + x_hi w_lo + x_lo w_hi accumulated in float32, the sum times
1 / s_x times 1 / s_w (exact), then + bias, + residual, ReLU -- each one float32 operation.

THE BOUND.  Per element, with S = sum_k |x_k| |w_k|, K = KH KW Cin the reduction length (taps outside the image count: they are
zeros and only make the bound larger), X = max|x|, Wm = max|w| over the operand tensors:
    |got - exact| <= [c S + K 2^-37 X Wm]  +  2 * 2^-23 (S + |bias| + |residual|) + tiny,    c = 4 * 2^-22 + 1.002 (3 K + 8) 2^-23.
  * The bracket is conv_backward_f16x3_ref.bound with no split-K: its docstring derives it.
  * The epilogue adds at most two float32 additions (bias, residual), each rounding a value of magnitude at most
    |gemm| + |bias| + |residual| <= (1 + small) S + |bias| + |residual| by at most one ulp 2^-23 (the bracket's "+ 8" absorbs the
    "small").  ReLU rounds nothing and cannot increase a difference (|max(a, 0) - max(b, 0)| <= |a - b|).
  Neither term is taken from what the kernel gives.
"""
import numpy as np
import torch
import torch.nn.functional as F

import conv_backward_f16x3_ref as R3

scale_of, split, matmul3 = R3.scale_of, R3.split, R3.matmul3

# name: (B, H, W, Cin, Cout, k, stride, pad, relu, bias, residual, (y_cstride, y_coffset) or None, x_cstride or None)
CASES = {
    'single_k_tile': (1, 4, 5, 32, 32, 1, 1, 0, False, False, False, None, None),       # M = 20: below one row tile
    'ragged_3x3': (2, 7, 9, 32, 40, 3, 1, 1, True, True, False, None, None),            # M = 126, Cp = 64 > Cout, border taps
    'stride2_3x3': (1, 9, 11, 32, 32, 3, 2, 1, False, False, False, None, None),
    'stride2_1x1': (1, 9, 11, 32, 32, 1, 2, 0, False, False, False, None, None),
    'residual_relu': (1, 6, 7, 64, 64, 1, 1, 0, True, False, True, None, None),         # residual and mask with no bias
    'channel_offset': (1, 5, 6, 32, 24, 3, 1, 1, False, True, False, (64, 8), 48),      # floats behind Cin; y a 24-channel view
    'linear': (5, 1, 1, 64, 24, 1, 1, 0, False, True, False, None, None),               # H = W = 1
    'two_k_tiles_wide': (2, 12, 13, 64, 96, 3, 1, 1, False, True, False, None, None),   # M = 312: several row and column tiles
}


def make_case(name):
    """Float32 CPU inputs of a case: x (B, H, W, xcs) -- the floats behind Cin are NaN: reading one poisons the result -- w, bias
    or None, residual (B, OH, OW, Cout) or None, and the geometry."""
    B, H, W, cin, cout, k, s, p, relu, has_b, has_r, lay, xcs = CASES[name]
    # the seed and the draw order of x and w are conv_backward_f16x3_ref.make_case's: a case the two files share by name and shape
    # (ragged_3x3) has the same x and w in both, so that the autograd test can use the backward's measured limits
    gen = torch.Generator().manual_seed(1000 + sum(ord(c) for c in name))
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    ycs, yco = lay if lay else (cout, 0)
    xcs = xcs or cin
    x = torch.randn(B, H, W, xcs, generator=gen)
    x[..., cin:] = float('nan')
    w = torch.randn(cout, k, k, cin, generator=gen) / float(k * k * cin) ** 0.5
    bias = torch.randn(cout, generator=gen) if has_b else None
    res = torch.randn(B, OH, OW, cout, generator=gen) if has_r else None
    return dict(name=name, B=B, H=H, W=W, cin=cin, cout=cout, k=k, stride=s, pad=p, relu=relu, OH=OH, OW=OW, ycs=ycs, yco=yco, xcs=xcs,
                x=x, w=w, bias=bias, res=res)


def im2col(x, k, stride, pad, OH, OW):
    """(B, H, W, Cin) numpy -> (B OH OW, k k Cin), K ordered (kh, kw, c) as the engine's weights are."""
    B, H, W, cin = x.shape
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    col = np.zeros((B, OH, OW, k * k, cin), x.dtype)
    for kh in range(k):
        for kw in range(k):
            col[:, :, :, kh * k + kw] = xp[:, kh:kh + stride * OH:stride, kw:kw + stride * OW:stride]
    return col.reshape(B * OH * OW, k * k * cin)


def conv_forward3(x, w, bias, res, stride, pad, relu):
    """y (B, OH, OW, Cout) float32 of the scheme from float32 numpy x (B, H, W, Cin), w (Cout, KH, KW, Cin), bias / res or None."""
    B, H, W, cin = x.shape
    cout, k = w.shape[0], w.shape[1]
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = matmul3(im2col(x, k, stride, pad, OH, OW), np.ascontiguousarray(w.reshape(cout, -1).T), scale_of(x), scale_of(w))
    y = y.astype(np.float32).reshape(B, OH, OW, cout)
    if bias is not None:
        y = (y + bias.astype(np.float32)).astype(np.float32)
    if res is not None:
        y = (y + res.astype(np.float32)).astype(np.float32)
    return np.maximum(y, np.float32(0)) if relu else y


def reference(x, w, bias, res, stride, pad, relu):
    """Float64 torch on the same float32 inputs: (y, S, E) -- the result, S = conv(|x|, |w|) and E = |bias| + |residual|, all
    (B, OH, OW, Cout) float64."""
    xn, wn = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    y = F.conv2d(xn, wn, None if bias is None else bias.double(), stride, pad).permute(0, 2, 3, 1)
    S = F.conv2d(xn.abs(), wn.abs(), None, stride, pad).permute(0, 2, 3, 1).contiguous()
    E = torch.zeros_like(S)
    if bias is not None:
        E = E + bias.double().abs()
    if res is not None:
        y = y + res.double()
        E = E + res.double().abs()
    return (F.relu(y) if relu else y).contiguous(), S, E


def case_reference(c):
    return reference(c['x'][..., :c['cin']].contiguous(), c['w'], c['bias'], c['res'], c['stride'], c['pad'], c['relu'])


def bound(k_terms, S, E, xmax, wmax, tiny=1e-30):
    """The per-element assertion (see the module docstring)."""
    return R3.bound(k_terms, 0, S, xmax, wmax, tiny) + 2 * 2.0 ** -23 * (S + E)
