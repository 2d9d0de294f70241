"""Float64 reference of the convolution gradients (srcnn_conv2d_backward, stereo_rcnn_amd/autograd.py): torch's own F.conv2d in
double precision under torch.autograd, on the CPU.  Layouts are the engine's: x (B, H, W, Cin) and dy / y (B, OH, OW, Cout) NHWC,
w (Cout, KH, KW, Cin).

The ReLU mask is taken from the FLOAT32 forward output it is handed (`y32`), not from a float64 forward of its own: the kernel
masks with that tensor, and an output within a rounding error of zero would otherwise flip between the two.  y32 == 0 gives 0.

For every gradient element it also returns S = sum |a * b| over the element's products -- the same convolution applied to the
absolute values -- which is what a rounding-error bound of a dot product is stated in: for ANY summation order of K float32
products, |computed - exact| <= gamma_K * S, gamma_K = K u / (1 - K u), u = 2^-24.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def masked_gradient(dy, y32=None, relu=False):
    """g = dy, or dy * [y32 > 0] with relu: float64 (B, OH, OW, Cout).  Exactly representable in float32 for float32 inputs."""
    g = dy.detach().double()
    if relu:
        g = g * (y32.detach() > 0).double()
    return g


def _grads(x_nchw, w_nchw, g_nchw, stride, pad):
    x = x_nchw.clone().requires_grad_(True)
    w = w_nchw.clone().requires_grad_(True)
    out = F.conv2d(x, w, None, stride, pad)
    assert out.shape == g_nchw.shape, (out.shape, g_nchw.shape)
    dx, dw = torch.autograd.grad(out, (x, w), g_nchw)
    return dx, dw


def conv_backward(x, w, dy, stride, pad, y32=None, relu=False):
    """Returns a dict of float64 tensors: g (the masked gradient), dx (B, H, W, Cin), dw (Cout, KH, KW, Cin), db (Cout), and
    S_dx, S_dw, S_db of the same shapes (the sums of absolute products)."""
    g = masked_gradient(dy, y32, relu)
    xn = x.detach().double().permute(0, 3, 1, 2).contiguous()
    wn = w.detach().double().permute(0, 3, 1, 2).contiguous()
    gn = g.permute(0, 3, 1, 2).contiguous()
    dx, dw = _grads(xn, wn, gn, stride, pad)
    sdx, sdw = _grads(xn.abs(), wn.abs(), gn.abs(), stride, pad)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    return {'g': g, 'dx': nhwc(dx), 'dw': nhwc(dw), 'db': g.sum((0, 1, 2)),
            'S_dx': nhwc(sdx), 'S_dw': nhwc(sdw), 'S_db': g.abs().sum((0, 1, 2))}


def bound(k_terms, splits, S, tiny=1e-30):
    """The per-element assertion of the GPU tests: (K_terms + splits + 8) u S + tiny.  K_terms: the reduction length of that
    gradient; splits: partial sums added afterwards; + 8: the last reduction stages and a BN-scale multiply."""
    return (k_terms + splits + 8) * U * S + tiny
