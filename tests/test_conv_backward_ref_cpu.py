"""CPU: tests/conv_backward_ref.py (the float64 yardstick of the convolution-backward kernels) against central finite
differences in float64.  With the ReLU mask held fixed -- it comes from the float32 forward output the reference is handed --
L = sum(conv(x, w) * g) is bilinear in (x, w), so central differences are exact up to rounding."""
import pytest
import torch
import torch.nn.functional as F

import conv_backward_ref as R

B, H, W, CIN, COUT = 2, 5, 6, 32, 5


def _case(k, stride, relu, seed):
    gen = torch.Generator().manual_seed(seed)
    pad = k // 2
    x = torch.randn(B, H, W, CIN, generator=gen, dtype=torch.float64)
    w = torch.randn(COUT, k, k, CIN, generator=gen, dtype=torch.float64)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = torch.randn(B, OH, OW, COUT, generator=gen, dtype=torch.float64)
    y32 = torch.randn(B, OH, OW, COUT, generator=gen).float()
    y32.view(-1)[::7] = 0.0                      # exact zeros: gradient 0
    return x, w, dy, y32, pad


def _loss(x, w, g, stride, pad):
    out = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), None, stride, pad).permute(0, 2, 3, 1)
    return float((out * g).sum())


def _fd(t, fn, h=1e-3):
    out = torch.empty_like(t)
    flat, o = t.view(-1), out.view(-1)
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + h
        up = fn()
        flat[i] = keep - h
        down = fn()
        flat[i] = keep
        o[i] = (up - down) / (2 * h)
    return out


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('k,stride', [(1, 1), (1, 2), (3, 1), (3, 2)])
def test_reference_matches_central_differences(k, stride, relu):
    x, w, dy, y32, pad = _case(k, stride, relu, 100 * k + 10 * stride + int(relu))
    ref = R.conv_backward(x, w, dy, stride, pad, y32=y32, relu=relu)
    g = ref['g']
    if relu:
        assert torch.equal(g, dy * (y32 > 0).double()) and float(g.view(-1)[::7].abs().max()) == 0.0
    else:
        assert torch.equal(g, dy)
    fd_x = _fd(x, lambda: _loss(x, w, g, stride, pad))
    fd_w = _fd(w, lambda: _loss(x, w, g, stride, pad))
    for name, fd in (('dx', fd_x), ('dw', fd_w)):
        rel = float((ref[name] - fd).abs().max() / ref[name].abs().max())
        assert rel < 1e-6, (name, rel)
    # db: d/db of sum((conv + b) * g) = the sum of g over the pixels
    assert torch.allclose(ref['db'], g.reshape(-1, COUT).sum(0), rtol=1e-13, atol=1e-13)
    # S bounds every gradient (|sum| <= sum of absolute values) and equals it when nothing cancels
    for name in ('dx', 'dw', 'db'):
        assert bool((ref[name].abs() <= ref['S_' + name] * (1 + 1e-12) + 1e-300).all())
    pos = R.conv_backward(x.abs(), w.abs(), dy.abs(), stride, pad)
    for name in ('dx', 'dw', 'db'):
        assert torch.allclose(pos[name], pos['S_' + name], rtol=1e-12, atol=0)


def test_stride_two_one_by_one_leaves_untouched_pixels_at_zero():
    x, w, dy, y32, pad = _case(1, 2, False, 7)
    ref = R.conv_backward(x, w, dy, 2, 0)
    assert float(ref['dx'][:, 1::2].abs().max()) == 0.0 and float(ref['dx'][:, :, 1::2].abs().max()) == 0.0
    assert float(ref['S_dx'][:, 1::2].abs().max()) == 0.0
    assert float(ref['dx'][:, ::2, ::2].abs().min()) > 0.0


def test_bound_formula():
    assert R.bound(100, 3, 2.0, tiny=0.0) == 111 * 2.0 ** -24 * 2.0
