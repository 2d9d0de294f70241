"""The 3 x f16 convolution backward (srcnn_conv2d_backward_f16x3, include/srcnn_hip.h) restated in numpy, its derived error
bound, and the cases of its tests.

THE SCHEME.  For an operand tensor v: s = 2^(14 - floor(log2 max|v|)) (one power of two per tensor, exponent clamped to +-126),
t = s v (exact), hi = float16(t), lo = float16(t - hi) (t - hi is exact in float32).  A GEMM element is
    sum_k (a_hi b_hi + a_hi b_lo + a_lo b_hi)   accumulated in float32,   then / s_a / s_b (exact).

THE BOUND.  Per element, with S = sum_k |a_k| |b_k|, K the reduction length, A = max|a|, B = max|b| over the operand TENSORS:
    |got - exact| <= c S + K 2^-37 A B + tiny,     c = 4 * 2^-22 + 1.002 (3 K + splits + 8) 2^-23.
  * The split.  |t - hi| <= 2^-11 |t|; lo rounds the exact residual r: |r - lo| <= 2^-11 |r| <= 2^-22 |t| while lo is a normal
    float16, and <= 2^-25 (half the subnormal spacing 2^-24) otherwise.  So t = hi + lo + d with |d| <= 2^-22 |t| + 2^-25.
  * One product.  t_a t_b = (H_a + d_a)(H_b + d_b), H = hi + lo, and H_a H_b is the three computed products plus lo_a lo_b, which
    is dropped: |lo_a lo_b| <= 2^-22 |t_a t_b| (1 + 2^-10).  Together |t_a t_b - computed products| <= (1 + 2) 2^-22 |t_a t_b|
    + 2^-25 (|t_a| + |t_b|) + second-order terms; rounded up: 4 * 2^-22 |t_a t_b| + 2^-24 (|t_a| + |t_b|).
  * The absolute term is what underflows after scaling.  Back in the tensors' units 2^-24 (|a| / s_b + |b| / s_a), and
    1 / s <= 2^-14 max|v| because s max|v| >= 2^14: at most 2^-38 (|a| B + |b| A) <= 2^-37 A B per product, K 2^-37 A B per element.
    (A tensor whose maximum is below 2^-112 meets the clamp and is outside this bound.)
  * The accumulation.  The three products are exact in float32 (two 11-bit significands); 3 K of them are added, then main + cross,
    then `splits` partial sums.  Each addition errs by at most one ulp, 2^-23, of a partial sum that is at most the sum of
    the terms' magnitudes <= 1.002 S (|hi| + |lo| <= (1 + 2^-10) |t|) -- ONE ulp, not half: the matrix unit's adder is not
    documented as round-to-nearest.  That is 1.002 (3 K + splits + 1) 2^-23 S; the "+ 8" leaves room for the last stages.
  Neither c nor the absolute term is taken from what the kernels give.
"""
import numpy as np
import torch
import torch.nn.functional as F

TOP = 14

# name: (B, H, W, Cin, Cout, k, stride, pad, relu, (y_cstride, y_coffset) or None, x_cstride or None)
CASES = {
    'single_k_tile': (1, 4, 5, 32, 32, 1, 1, 0, False, None, None),      # M = 20 < 32: one partial K tile in wgrad
    'ragged_3x3': (2, 7, 9, 32, 40, 3, 1, 1, True, None, None),          # M = 126, Cp = 64 > Cout, border taps, ReLU mask with y == 0
    'stride2_3x3': (1, 9, 11, 32, 32, 3, 2, 1, False, None, None),       # the divisibility test of the gather
    'stride2_1x1': (1, 9, 11, 32, 32, 1, 2, 0, False, None, None),       # dx pixels never read must be exact zeros
    'channel_offset': (1, 5, 6, 32, 24, 3, 1, 1, False, (64, 8), 48),    # dy a channel view; dx / x with floats beyond Cin
    'linear': (5, 1, 1, 64, 24, 1, 1, 0, False, None, None),
    'forced_split': (2, 12, 13, 64, 64, 3, 1, 1, False, None, None),     # M = 312: 10 K tiles, splits = 3 -> 4 + 4 + 2
}


def make_case(name):
    """Float32 CPU inputs of a case: dict with x (B, H, W, xcs), w, dy_full (B, OH, OW, ycs), y32 (the saved output where relu,
    with exact zeros planted, else None) and the geometry."""
    B, H, W, cin, cout, k, s, p, relu, lay, xcs = CASES[name]
    gen = torch.Generator().manual_seed(1000 + sum(ord(c) for c in name))
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    ycs, yco = lay if lay else (cout, 0)
    xcs = xcs or cin
    x = torch.randn(B, H, W, xcs, generator=gen)
    w = torch.randn(cout, k, k, cin, generator=gen) / float(k * k * cin) ** 0.5
    dy_full = torch.randn(B, OH, OW, ycs, generator=gen) * 1e-3
    y32 = None
    if relu:
        y32 = F.conv2d(x[..., :cin].permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), None, s, p).permute(0, 2, 3, 1).contiguous()
        y32.view(-1)[::5] = 0.0                    # exact zeros: masked like negatives
        assert 0.2 < float((y32 > 0).float().mean()) < 0.8
    return dict(name=name, B=B, H=H, W=W, cin=cin, cout=cout, k=k, stride=s, pad=p, relu=relu, OH=OH, OW=OW, ycs=ycs, yco=yco, xcs=xcs,
                x=x, w=w, dy_full=dy_full, y32=y32)


def scale_of(t):
    """The tensor's power of two as float32 (pow2_scale of csrc/conv_backward_f16x3.hip)."""
    m = np.float32(np.max(np.abs(t))) if t.size else np.float32(0)
    e = int(m.view(np.uint32) >> 23) - 127
    return np.ldexp(np.float32(1), min(max(TOP - e, -126), 126))


def split(t, s):
    v = t.astype(np.float32) * s
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


def matmul3(a, b, sa, sb):
    """(M, K) @ (K, N) by the scheme: float16 hi / lo, three products, float32 accumulation, exact rescale."""
    ah, al = (h.astype(np.float32) for h in split(a, sa))
    bh, bl = (h.astype(np.float32) for h in split(b, sb))
    cross = (al @ bh + ah @ bl).astype(np.float32)
    main = (ah @ bh).astype(np.float32)
    return ((main + cross) * (np.float32(1) / sa)) * (np.float32(1) / sb)


def conv_backward3(x, w, g, stride, pad):
    """dx (B, H, W, Cin), dw (Cout, KH, KW, Cin) of the scheme from float32 numpy x (B, H, W, Cin), w (Cout, KH, KW, Cin) and the masked
    gradient g (B, OH, OW, Cout): the kernels' two GEMMs, dgrad in gather form and wgrad over the output pixels."""
    B, H, W, cin = x.shape
    cout, KH, KW, _ = w.shape
    _, OH, OW, _ = g.shape
    sg, sw, sx = scale_of(g), scale_of(w), scale_of(x)
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    xcol = np.zeros((B, OH, OW, KH * KW, cin), np.float32)
    gcol = np.zeros((B, H, W, KH * KW, cout), np.float32)
    for kh in range(KH):
        for kw in range(KW):
            tap = kh * KW + kw
            xcol[:, :, :, tap] = xp[:, kh:kh + stride * OH:stride, kw:kw + stride * OW:stride]
            for oh in range(OH):
                h = oh * stride - pad + kh
                if not 0 <= h < H:
                    continue
                for ow in range(OW):
                    ww = ow * stride - pad + kw
                    if 0 <= ww < W:
                        gcol[:, h, ww, tap] = g[:, oh, ow]
    M = B * OH * OW
    dw = matmul3(np.ascontiguousarray(g.reshape(M, cout).T), xcol.reshape(M, KH * KW * cin), sg, sx).reshape(cout, KH, KW, cin)
    wmat = np.ascontiguousarray(w.transpose(1, 2, 0, 3)).reshape(KH * KW * cout, cin)
    dx = matmul3(gcol.reshape(B * H * W, KH * KW * cout), wmat, sg, sw).reshape(B, H, W, cin)
    return dx, dw


def bound(k_terms, splits, S, amax, bmax, tiny=1e-30):
    """The per-element assertion (see the module docstring): S a float64 tensor, amax / bmax the operand tensors' max |.|."""
    c = 4 * 2.0 ** -22 + 1.002 * (3 * k_terms + splits + 8) * 2.0 ** -23
    return c * S + k_terms * 2.0 ** -37 * float(amax) * float(bmax) + tiny
