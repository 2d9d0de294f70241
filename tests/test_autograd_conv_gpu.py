"""GPU: stereo_rcnn_amd.autograd (differentiable conv2d / linear on the exact-fp32 engine) against float64 torch autograd on the
CPU, and the proof that the training pieces compose: a box head trained for one backward pass from rcnn_losses.

ReLU masks: a float64 forward of its own would put an output that lies within a rounding error of zero on the other side of
the ReLU than the float32 forward; the seeds are fixed, and the first test's reference takes its mask from the device's
float32 output, as tests/conv_backward_ref.py does.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_backward_ref as R
import conv_backward_tolerances as CT
import losses_ref
from tolerances import observe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ag(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import autograd
    return autograd


def _norm_err(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def test_conv2d_with_bn_relu_and_residual(ag, dev):
    """relu(bn(conv(x)) + r) on the ragged 3x3 case: gradients for x, the UNFOLDED weight and the residual; none for the BN."""
    B, H, W, cin, cout, k, s, p = 2, 23, 37, 96, 200, 3, 1, 1
    gen = torch.Generator().manual_seed(41)
    x = torch.randn(B, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, k, k, generator=gen) / float(k * k * cin) ** 0.5
    r = torch.randn(B, cout, H, W, generator=gen)
    bn = {'weight': torch.rand(cout, generator=gen) + 0.5, 'bias': torch.randn(cout, generator=gen) * 0.1,
          'running_mean': torch.randn(cout, generator=gen) * 0.1, 'running_var': torch.rand(cout, generator=gen) + 0.5}
    dy = torch.randn(B, cout, H, W, generator=gen)

    leaves = [t.to(dev).requires_grad_(True) for t in (x, w, r)]
    bn_dev = {k_: v.to(dev).requires_grad_(True) for k_, v in bn.items()}
    y = ag.conv2d(leaves[0], leaves[1], None, s, p, relu=True, residual=leaves[2], bn=bn_dev)
    assert y.shape == (B, cout, H, W)
    y.backward(dy.to(dev))
    assert all(v.grad is None for v in bn_dev.values())
    mask = (y.detach().cpu() > 0).double()
    assert 0.2 < float(mask.mean()) < 0.8

    # float64: the same graph, the ReLU written as the float32 forward's mask
    scale = bn['weight'].double() / torch.sqrt(bn['running_var'].double() + 1e-5)
    shift = bn['bias'].double() - bn['running_mean'].double() * scale
    xd, wd, rd = (t.double().requires_grad_(True) for t in (x, w, r))
    out = (F.conv2d(xd, wd, None, s, p) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + rd) * mask
    assert _norm_err(y, out.detach()) < 1e-5
    out.backward(dy.double())

    # derived per-element bound, S from the same convolution on absolute values (the folded weight |w scale|)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    g = nhwc(dy.double() * mask)
    ref = R.conv_backward(nhwc(x), nhwc(w.double() * scale.view(-1, 1, 1, 1)), g, s, p)
    S_dx = ref['S_dx'].permute(0, 3, 1, 2)
    S_dw = ref['S_dw'].permute(0, 3, 1, 2) * scale.abs().view(-1, 1, 1, 1)       # d(w scale) / dw = scale
    for name, leaf, want, S, kt in (('dx', leaves[0], xd.grad, S_dx, k * k * cout), ('dw', leaves[1], wd.grad, S_dw, B * H * W)):
        err = (leaf.grad.cpu().double() - want).abs()
        worst = float((err / R.bound(kt, 64, S)).max())
        v = observe('autograd_conv_%s' % name, _norm_err(leaf.grad, want))
        print('autograd conv2d %s: max err / bound %.3f, normalised %.3e' % (name, worst, v))
        assert worst <= 1.0, (name, worst)
        lim = CT.LIMITS.get('autograd_conv_%s' % name)
        if lim is not None:
            assert v <= lim, (name, v, lim)
    assert torch.equal(leaves[2].grad.cpu().double(), rd.grad)        # dy * mask: exact


def test_linear_and_k_not_a_multiple_of_32(ag, dev):
    gen = torch.Generator().manual_seed(42)
    x, w, b = torch.randn(5, 2048, generator=gen), torch.randn(10, 2048, generator=gen) / 45.0, torch.randn(10, generator=gen)
    dy = torch.randn(5, 10, generator=gen)
    leaves = [t.to(dev).requires_grad_(True) for t in (x, w, b)]
    ag.linear(*leaves).backward(dy.to(dev))
    ref = [t.double().requires_grad_(True) for t in (x, w, b)]
    F.linear(*ref).backward(dy.double())
    ax, aw, ady = x.double().abs(), w.double().abs(), dy.double().abs()
    for name, a, r_, kt, S in (('dx', leaves[0], ref[0], 10, ady @ aw), ('dw', leaves[1], ref[1], 5, ady.t() @ ax),
                               ('db', leaves[2], ref[2], 5, ady.sum(0))):
        err = (a.grad.cpu().double() - r_.grad).abs()
        assert bool((err <= R.bound(kt, 1, S)).all()), (name, float((err / R.bound(kt, 1, S)).max()))
    with pytest.raises(ValueError):
        ag.linear(torch.zeros(3, 48, device=dev), torch.zeros(4, 48, device=dev))
    with pytest.raises(ValueError):
        ag.conv2d(torch.zeros(1, 48, 4, 4, device=dev), torch.zeros(8, 48, 1, 1, device=dev))
    # gradients that are not asked for are not computed
    xg = x.to(dev).requires_grad_(True)
    ag.linear(xg, w.to(dev), b.to(dev)).backward(dy.to(dev))
    assert torch.equal(xg.grad, leaves[0].grad)


# ---- the box head: RCNN_top as conv 7x7/7 (64 -> 128) + ReLU + conv 1x1 (128 -> 128) + ReLU, then the three linear heads
N_ROIS, N_CLS, G = 6, 4, 28
HEAD_SHAPES = {'top1_w': (128, 64, 7, 7), 'top1_b': (128,), 'top2_w': (128, 128, 1, 1), 'top2_b': (128,),
               'cls_w': (N_CLS, 128), 'cls_b': (N_CLS,), 'bbox_w': (6 * N_CLS, 128), 'bbox_b': (6 * N_CLS,),
               'dim_w': (5 * N_CLS, 128), 'dim_b': (5 * N_CLS,)}
# Derived ceiling (twice the measured maximum, tests/conv_backward_tolerances.py, holds as well): the chain is three fmaf chains forward and three
# backward of lengths K = 3136 (7 x 7 x 64), 128, 128; a K-term float32 dot product is off by at most (K + 8) u relative to its sum
# of absolute products, and normalising by the largest reference magnitude of a tensor puts that sum at the reference's own
# scale: sum over the six stages of (K_i + 8) u = 2 (3144 + 136 + 136) u = 4.1e-4.
HEAD_CEILING = 2 * (3136 + 8 + 128 + 8 + 128 + 8) * R.U


def _head_forward(params, feat, conv2d, linear):
    t = conv2d(feat, params['top1_w'], params['top1_b'], 7, 0, True)
    t = conv2d(t, params['top2_w'], params['top2_b'], 1, 0, True)
    t = t.reshape(t.shape[0], -1)
    return (linear(t, params['cls_w'], params['cls_b']), linear(t, params['bbox_w'], params['bbox_b']),
            linear(t, params['dim_w'], params['dim_b']))


def test_box_head_trains_one_backward_pass_from_rcnn_losses(ag, dev):
    from stereo_rcnn_amd.model.stereo_rcnn import losses
    gen = torch.Generator().manual_seed(43)
    params = {}
    for name, shape in HEAD_SHAPES.items():
        fan = 1
        for v in shape[1:]:
            fan *= v
        params[name] = torch.randn(shape, generator=gen) * (0.1 if name.endswith('_b') else 1.5 / float(fan) ** 0.5)
    feat = torch.randn(N_ROIS, 64, 7, 7, generator=gen)
    label = torch.tensor([0, 2, 2, 1, 3, 0]).float()                    # class 0 and a repeated class
    fg = (label > 0).float()
    kpts = torch.randn(N_ROIS, 6, G, generator=gen)                     # the keypoint term is fed a constant
    tl, tr = torch.randn(1, N_ROIS, 4, generator=gen), torch.randn(1, N_ROIS, 4, generator=gen)
    tdim = torch.randn(1, N_ROIS, 5, generator=gen)
    klabel = torch.stack((torch.randint(0, 4 * G, (N_ROIS,), generator=gen), torch.randint(0, G, (N_ROIS,), generator=gen),
                          torch.randint(0, G, (N_ROIS,), generator=gen)), 1).view(1, N_ROIS, 3)
    kweight = torch.stack((fg, fg, fg), 1).view(1, N_ROIS, 3)
    ws_in = fg.view(1, N_ROIS, 1) * torch.ones(1, N_ROIS, 4)
    ws_out = ws_in * torch.rand(1, N_ROIS, 4, generator=gen)
    targets = [label, tl, tr, tdim, klabel, kweight, ws_in, ws_out]

    def run(device, dtype, conv2d, linear, loss_fn):
        p = {k_: v.to(device=device, dtype=dtype).requires_grad_(True) for k_, v in params.items()}
        f = feat.to(device=device, dtype=dtype).requires_grad_(True)
        cls, bbox, dim = _head_forward(p, f, conv2d, linear)
        out = loss_fn(cls, bbox, dim, kpts.to(device=device, dtype=dtype), *[t.to(device) for t in targets])
        sum((0.7 + 0.3 * i) * l for i, l in enumerate(out[:3])).backward()
        grads = dict({k_: v.grad for k_, v in p.items()}, feat=f.grad)
        assert all(g is not None for g in grads.values())
        return [l.detach().cpu().double() for l in out[:3]], {k_: g.detach().cpu().double() for k_, g in grads.items()}

    got_l, got = run(dev, torch.float32, ag.conv2d, ag.linear, losses.rcnn_losses)
    again_l, again = run(dev, torch.float32, ag.conv2d, ag.linear, losses.rcnn_losses)
    ref_conv = lambda x, w, b, s, p, relu: F.relu(F.conv2d(x, w, b, s, p)) if relu else F.conv2d(x, w, b, s, p)
    ref_l, ref = run('cpu', torch.float64, ref_conv, F.linear, losses_ref.rcnn_losses)

    for a, b in zip(got_l, ref_l):
        assert abs(float(a) - float(b)) <= HEAD_CEILING * abs(float(b))
    worst = 0.0
    for name in sorted(ref):
        assert got[name].shape == ref[name].shape and float(ref[name].abs().max()) > 0, name
        assert torch.equal(got[name], again[name]), '%s: not repeatable bit for bit' % name
        v = float((got[name] - ref[name]).abs().max() / ref[name].abs().max())
        print('box head %s: normalised error %.3e' % (name, v))
        worst = max(worst, v)
        assert v <= HEAD_CEILING, (name, v)
    observe('autograd_box_head_grad', worst)
    lim = CT.LIMITS.get('autograd_box_head_grad')
    if lim is not None:
        assert worst <= lim, (worst, lim)
