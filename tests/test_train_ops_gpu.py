"""GPU: the three adjoint kernels of csrc/train_ops.hip and their autograd functions against the float64 restatement
(tests/train_ops_ref.py; checked on the CPU by tests/test_train_ops_ref_cpu.py).

Bounds.  The bilinear adjoint sums at most n = (rows x columns x 4) terms per element in one fmaf chain with coefficients rounded
once: |err| <= (n + 2) u S, S the same sum over absolute values (the reference takes the device's float32 tap weights, so no
coefficient error enters).  The copies are exact.  The deconvolution's gradients are the conv backward's fmaf chains: the bound of
tests/conv_backward_ref.py.  tests/train_tolerances.py holds the measured values on top.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_backward_ref as R
import train_ops_ref as T
import train_tolerances as TT
from tolerances import observe

pytestmark = pytest.mark.gpu

UP_SHAPES = [((4, 11), (7, 21)), ((7, 21), (13, 41)), ((13, 41), (26, 82)), ((1, 1), (3, 5)), ((5, 5), (5, 5)), ((2, 3), (2, 7))]


@pytest.fixture(scope='module')
def ag(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import autograd
    return autograd


def _held(name, value):
    v = observe(name, value)
    lim = TT.LIMITS.get(name)
    if lim is not None:
        assert v <= lim, (name, v, lim)
    return v


def _up_backward(dy, TH, TW):
    from stereo_rcnn_amd import _lib
    B, H, W, C = dy.shape
    d_top = torch.full((B, TH, TW, C), float('nan'), device=dy.device)          # every element must be written
    _lib.check(_lib.lib().srcnn_upsample_add_backward(dy.data_ptr(), B, H, W, C, d_top.data_ptr(), TH, TW, _lib.stream()),
               "srcnn_upsample_add_backward")
    return d_top


@pytest.mark.parametrize('C', [8, 256])
@pytest.mark.parametrize('top_hw,out_hw', UP_SHAPES)
def test_upsample_add_backward(ag, dev, top_hw, out_hw, C):
    from stereo_rcnn_amd import engine
    (TH, TW), (H, W), B = top_hw, out_hw, 2
    gen = torch.Generator().manual_seed(100 + TH * TW + C)
    dy = torch.randn(B, H, W, C, generator=gen)
    top = torch.randn(B, TH, TW, C, generator=gen)
    got = _up_backward(dy.to(dev), TH, TW)
    assert torch.equal(got, _up_backward(dy.to(dev), TH, TW)), 'not repeatable bit for bit'
    ref, S = T.upsample_add_backward(dy, TH, TW)
    err = (got.cpu().double() - ref).abs()
    n = 4 * (-(-H // TH) * 2 + 2) * (-(-W // TW) * 2 + 2)            # terms one top pixel can receive
    assert bool((err <= (n + 2) * T.U * S + 1e-300).all()), float((err / (T.U * S + 1e-300)).max())
    _held('upsample_add_backward', float(err.max() / ref.abs().max()))
    # the adjoint identity against the product's own forward, both inner products in float64 from the float32 device tensors
    y = torch.empty(B, H, W, C, device=dev)
    engine.upsample_add(top.to(dev), TH, TW, torch.zeros(B, H, W, C, device=dev), B, H, W, C, y)
    lhs = float((y.cpu().double() * dy.double()).sum())
    rhs = float((top.double() * got.cpu().double()).sum())
    scale = float((T.upsample(top.abs(), H, W) * dy.double().abs()).sum())
    assert abs(lhs - rhs) <= (n + 8) * T.U * scale, (lhs, rhs, scale)
    # through autograd: the lateral's gradient is dy itself
    t, l = top.to(dev).requires_grad_(True), torch.randn(B, H, W, C, generator=gen).to(dev).requires_grad_(True)
    ag.upsample_add(t, l).backward(dy.to(dev))
    assert torch.equal(t.grad, got) and torch.equal(l.grad.cpu(), dy)


@pytest.mark.parametrize('top_hw,out_hw', [((1, 1), (3, 5)), ((3, 4), (5, 7)), ((2, 2), (2, 2))])
def test_upsample_add_backward_equals_the_float32_restatement(dev, top_hw, out_hw):
    """Bit for bit against train_ops_ref.upsample_add_backward_f32: the forward restatement's taps and weights, accumulated in
    the kernel's defined summation order with an exact fmaf.  A one-pixel top (r = 0: every output pixel lands on it), clamped
    last rows and columns where both taps are the same top pixel, and the identity size."""
    import numpy as np
    (TH, TW), (H, W), B, C = top_hw, out_hw, 2, 8
    gen = torch.Generator().manual_seed(400 + TH * TW + H)
    dy = torch.randn(B, H, W, C, generator=gen)
    got = _up_backward(dy.to(dev), TH, TW).cpu().numpy()
    want = T.upsample_add_backward_f32(dy.numpy(), TH, TW)
    differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print("upsample_add_backward %s -> %s: %d of %d words differ from the float32 restatement" % (top_hw, out_hw, differ, want.size))
    assert differ == 0
    if top_hw == out_hw:
        assert np.array_equal(got, dy.numpy())


@pytest.mark.parametrize('B,H,W,C', [(2, 7, 21, 256), (1, 4, 11, 8), (3, 1, 1, 8), (2, 6, 5, 40)])
def test_subsample2_backward(ag, dev, B, H, W, C):
    gen = torch.Generator().manual_seed(200 + H)
    x = torch.randn(B, H, W, C, generator=gen)
    xd = x.to(dev).requires_grad_(True)
    y = ag.subsample2(xd)
    assert torch.equal(y.detach().cpu(), x[:, ::2, ::2, :])
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy.to(dev))
    assert torch.equal(xd.grad.cpu(), T.subsample2_backward(dy, H, W))


@pytest.mark.parametrize('M,h,w,cq', [(3, 14, 14, 256), (2, 3, 5, 8), (1, 1, 1, 40)])
def test_pixel_shuffle2_both_ways(ag, dev, M, h, w, cq):
    gen = torch.Generator().manual_seed(300 + cq)
    x = torch.randn(M, h, w, 4 * cq, generator=gen)
    wide = ag.pixel_shuffle2(x.to(dev), cq)
    assert torch.equal(wide.cpu(), T.pixel_shuffle2(x, cq))
    assert torch.equal(ag.pixel_shuffle2(wide, cq, inverse=True).cpu(), x)
    g = torch.randn(M, 2 * h, 2 * w, cq, generator=gen)
    assert torch.equal(ag.pixel_shuffle2(g.to(dev), cq, inverse=True).cpu(), T.pixel_unshuffle2(g))


def test_pixel_shuffle2_refuses_what_it_cannot_map(ag, dev):
    z = lambda *shape: torch.zeros(shape, device=dev)
    for x, cq, inverse in ((z(1, 2, 2, 32), 16, False), (z(1, 3, 4, 8), 8, True), (z(1, 4, 3, 8), 8, True), (z(1, 4, 4, 16), 8, True),
                           (z(1, 2, 2, 16), 4, False), (z(2, 2, 32), 8, False)):
        with pytest.raises(ValueError):
            ag.pixel_shuffle2(x, cq, inverse=inverse)
    with pytest.raises(TypeError):
        ag.pixel_shuffle2(z(1, 2, 2, 32).double(), 8)
    # a non-contiguous view is copied, not read through a wrong pointer
    x = torch.randn(2, 3, 5, 64, device=dev)[:, :, :, :32]
    assert torch.equal(ag.pixel_shuffle2(x, 8).cpu(), T.pixel_shuffle2(x.cpu(), 8))


@pytest.mark.parametrize('M,h,w,cin,cout', [(3, 14, 14, 256, 256), (2, 5, 3, 64, 40)])
def test_conv_transpose2x2(ag, dev, M, h, w, cin, cout):
    gen = torch.Generator().manual_seed(400 + cout)
    x = torch.randn(M, h, w, cin, generator=gen)
    wt = torch.randn(cin, cout, 2, 2, generator=gen) / cin ** 0.5
    b = torch.randn(cout, generator=gen) * 0.1
    dy = torch.randn(M, 2 * h, 2 * w, cout, generator=gen)
    leaves = [t.to(dev).requires_grad_(True) for t in (x, wt, b)]
    y = ag.conv_transpose2x2(leaves[0], leaves[1], leaves[2], relu=True)
    assert y.shape == (M, 2 * h, 2 * w, cout)
    y.backward(dy.to(dev))
    # the ReLU mask from the device's float32 output (tests/test_autograd_conv_gpu.py says why)
    mask = (y.detach().cpu() > 0).double()
    assert 0.2 < float(mask.mean()) < 0.8
    ref = [t.double().requires_grad_(True) for t in (x.permute(0, 3, 1, 2), wt, b)]
    out = F.conv_transpose2d(ref[0], ref[1], ref[2], stride=2).permute(0, 2, 3, 1) * mask
    assert float((y.detach().cpu().double() - out.detach()).abs().max() / out.detach().abs().max()) < 1e-5
    out.backward(dy.double())
    S = T.conv_transpose2x2_backward(x, wt, dy.double() * mask)
    tag = 'conv_transpose_%d' % cout
    for name, got, want, Sk, kt in (('dx', leaves[0].grad, ref[0].grad.permute(0, 2, 3, 1), S['S_dx'], 4 * cout),
                                    ('dw', leaves[1].grad, ref[1].grad, S['S_dw'], M * h * w),
                                    ('db', leaves[2].grad, ref[2].grad, S['S_db'], 4 * M * h * w)):
        err = (got.cpu().double() - want).abs()
        worst = float((err / R.bound(kt, 64, Sk)).max())
        v = _held('%s_%s' % (tag, name), float(err.max() / want.abs().max()))
        print('%s %s: max err / bound %.3f, normalised %.3e' % (tag, name, worst, v))
        assert worst <= 1.0, (name, worst)
