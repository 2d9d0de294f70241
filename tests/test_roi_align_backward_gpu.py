"""GPU: the ROIAlign backward kernels (roi_align_backward_cuda, srcnn_pool2x2_s1_backward, srcnn_pyramid_roi_align_backward)
and the autograd surface on top of them.

Bounds are derived, not measured (tests/roi_align_backward_ref.py): u = 2^-24; an ordered float32 sum of k contributions,
each at most 3 roundings from its exact value, lies within gamma_(k+3) x sum |contribution| of the exact sum; two float32
sums of the same k contributions in different orders lie within k x 2^-23 x sum |contribution| of each other.

DELIBERATE DEVIATION from the issue for the reference's CONTRACTED build ('fma'): the issue asks for the reorder bound on the
elements none of whose coordinates lies within one ulp of an integer or the border.  A coordinate moved by contraction moves
the bilinear weights by that much, which at small k exceeds the reorder bound, so that bound cannot hold against that build
for any correct kernel.  The test adds the derived movement (`slack`, roi_align_backward_ref._bin_size / lattice_axis, pinned
on the CPU by an emulation of the build's two contractions) and leaves out the elements within that movement -- not one ulp
-- of an integer or the border, under the issue's 99 % cap.  That makes the 'fma' comparison about 1e-5 relative: it catches
gross errors only.  The tight checks are the bit-equality with the restatement and the un-contracted build ('nofma'), where
the issue's bound and its bit-equality for k <= 1 hold as stated."""
import ctypes

import numpy as np
import pytest
import torch

import roi_align_backward_ref as R
from test_ref_kernels_gpu import ROI_SHAPES, ROI_SIZES, roi_inputs

pytestmark = pytest.mark.gpu

U = R.U


def _lib():
    from stereo_rcnn_amd import _lib as m
    return m


def backward_cuda(top, rois, shape, ah, aw, scale):
    """roi_align_backward_cuda into a tensor full of NaN: the op overwrites every element."""
    m = _lib()
    grad = torch.full(shape, float('nan'), dtype=torch.float32, device=top.device)
    assert top.is_contiguous() and rois.is_contiguous()
    rc = m.lib().roi_align_backward_cuda(ah, aw, scale, top.data_ptr(), rois.data_ptr(), int(rois.shape[0]), int(rois.shape[1]),
                                         grad.data_ptr(), shape[0], shape[1], shape[2], shape[3], m.stream())
    assert rc == 1
    return grad


def forward_cuda(feat, rois, ah, aw, scale):
    m = _lib()
    b, c, h, w = feat.shape
    out = torch.zeros((int(rois.shape[0]), c, ah, aw), dtype=torch.float32, device=feat.device)
    assert m.lib().roi_align_forward_cuda(ah, aw, scale, feat.data_ptr(), b, c, h, w, rois.data_ptr(), int(rois.shape[0]), 5,
                                          out.data_ptr(), m.stream()) == 1
    return out


def pool_forward(x, take_max):
    m = _lib()
    n, c, h, w = x.shape
    y = torch.empty((n, c, h - 1, w - 1), dtype=torch.float32, device=x.device)
    m.check(m.lib().srcnn_pool2x2_s1(x.data_ptr(), n * c, h, w, y.data_ptr(), int(take_max), m.stream()))
    return y


def pool_backward(gy, x, take_max):
    m = _lib()
    n, c, oh, ow = gy.shape
    gx = torch.full((n, c, oh + 1, ow + 1), float('nan'), dtype=torch.float32, device=gy.device)
    m.check(m.lib().srcnn_pool2x2_s1_backward(gy.data_ptr(), x.data_ptr() if x is not None else None, n * c, oh + 1, ow + 1,
                                              gx.data_ptr(), int(take_max), m.stream()))
    return gx


def pyramid_forward(maps, rois, A, im_h, limit=None):
    m = _lib()
    C = int(maps[0].shape[3])
    n = int(rois.shape[0])
    out = torch.zeros((n, A, A, C), dtype=torch.float32, device=rois.device)
    ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in maps])
    mh = (ctypes.c_int * 4)(*[int(t.shape[1]) for t in maps])
    mw = (ctypes.c_int * 4)(*[int(t.shape[2]) for t in maps])
    m.check(m.lib().srcnn_pyramid_roi_align(ptrs, mh, mw, C, im_h, rois.data_ptr(), n, A, out.data_ptr(), C, 0, 0, 0,
                                            limit.data_ptr() if limit is not None else None, m.stream()))
    return out


def pyramid_backward(gout, cstride, coffset, rois, A, C, im_h, shapes, limit=None):
    """shapes: [(B, h, w)] x 4 -> four NHWC gradient maps (allocated full of NaN: every element is written)."""
    m = _lib()
    grads = [torch.full((b, h, w, C), float('nan'), dtype=torch.float32, device=gout.device) for b, h, w in shapes]
    ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in grads])
    mh = (ctypes.c_int * 4)(*[s[1] for s in shapes])
    mw = (ctypes.c_int * 4)(*[s[2] for s in shapes])
    m.check(m.lib().srcnn_pyramid_roi_align_backward(gout.data_ptr(), cstride, coffset, rois.data_ptr(), int(rois.shape[0]), A, C, im_h,
                                                     ptrs, mh, mw, shapes[0][0], 0, limit.data_ptr() if limit is not None else None,
                                                     m.stream()))
    return grads


def reference_backward(kind, top, rois, shape, ah, aw, scale):
    """the reference's own kernel (roi_align_kernel.cu:145-162) into a zeroed tensor"""
    from oracle import ref_ops
    L = ref_ops.lib(kind)
    L.ROIAlignBackwardLaucher.restype = ctypes.c_int
    L.ROIAlignBackwardLaucher.argtypes = [ctypes.c_void_p, ctypes.c_float] + [ctypes.c_int] * 7 + [ctypes.c_void_p] * 3
    grad = torch.zeros(shape, dtype=torch.float32, device=top.device)
    torch.cuda.synchronize()
    L.ROIAlignBackwardLaucher(top.data_ptr(), float(scale), shape[0], int(rois.shape[0]), shape[2], shape[3], shape[1], ah, aw,
                              rois.data_ptr(), grad.data_ptr(), None)
    torch.cuda.synchronize()
    return grad


def _cases():
    for shape, scale in ROI_SHAPES:
        for a in ROI_SIZES:
            yield pytest.param(('forward', a, shape, scale), id='a%d-%s' % (a, 'x'.join(map(str, shape))))
    yield pytest.param(('crowded',), id='crowded')
    yield pytest.param(('many',), id='many-rois')


def _inputs(case):
    if case[0] == 'crowded':
        return R.crowded_case()
    if case[0] == 'many':
        return R.many_rois_case()
    _, a, shape, scale = case
    _, rois = roi_inputs(a, shape)
    top = np.random.default_rng(1000 + a + shape[2]).standard_normal((len(rois), shape[1], a, a)).astype(np.float32)
    return top, rois, shape, a, scale


_STATS = {}


def _restated(case):
    """restatement + statistics of a case, computed once per session (shared by the bit-exact and the live-reference test)"""
    if case not in _STATS:
        top, rois, shape, a, scale = _inputs(case)
        _STATS[case] = R.roi_align_backward_np(top, rois, shape, a, a, scale, stats=True)
    return _STATS[case]


@pytest.mark.parametrize("case", _cases())
def test_backward_bit_equal_to_the_ordered_restatement(dev, case):
    top, rois, shape, a, scale = _inputs(case)
    want, k = _restated(case)[:2]
    got = backward_cuda(torch.from_numpy(top).to(dev), torch.from_numpy(rois).to(dev), shape, a, a, scale).cpu().numpy()
    assert not np.isnan(got).any()
    differ = got.view(np.uint32) != want.view(np.uint32)
    print('%s: %d elements, max k %d, %d differ' % (case[0], got.size, k.max(), differ.sum()))
    if case[0] == 'crowded':
        assert k.max() >= 2000
    assert not differ.any(), 'first differing element %s: %r vs %r' % (np.argwhere(differ)[0], got[differ][0], want[differ][0])


@pytest.mark.parametrize("kind", ['nofma', 'fma'])
@pytest.mark.parametrize("case", _cases())
def test_backward_against_the_reference_kernel_live(dev, case, kind):
    from oracle import ref_ops
    if not ref_ops.available(kind):
        pytest.skip('oracle/_ref was not built')
    top, rois, shape, a, scale = _inputs(case)
    _, k, sabs, slack, fragile = _restated(case)
    t, r = torch.from_numpy(top).to(dev), torch.from_numpy(rois).to(dev)
    got = backward_cuda(t, r, shape, a, a, scale).cpu().numpy().astype(np.float64)
    ref = reference_backward(kind, t, r, shape, a, a, scale).cpu().numpy()
    kk = np.broadcast_to(k[:, None], got.shape)
    bound = kk * 2.0 ** -23 * sabs
    err = np.abs(got - ref.astype(np.float64))
    if kind == 'nofma':
        single = kk <= 1
        assert np.array_equal(got.astype(np.float32)[single].view(np.uint32), ref[single].view(np.uint32))
        print('%s nofma: max err %.3e, max err / bound %.3f' % (case[0], err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
    else:
        # a build with contraction moves lattice coordinates (roi_align_backward_ref._bin_size / lattice_axis derive by how much:
        # it fuses `end * scale - start` and `i * bin + start`): the weights are linear in the coordinates with slope 1, so a
        # contribution moves by at most |g| x (dh wx + dw wy + dh dw) -- `slack` -- unless the movement carries the coordinate
        # across an integer or the map border (`fragile` elements, left out; they may not be more than 1 % of the non-zero
        # elements, so that leaving them out cannot hide a failure; tests/test_roi_align_backward_cpu.py confirms both on the CPU)
        keep = ~np.broadcast_to(fragile[:, None], got.shape)
        nz = (got != 0) & (kk > 0)
        print('%s fma: %d of %d non-zero elements compared, max err %.3e, max err / bound %.3f'
              % (case[0], (keep & nz).sum(), nz.sum(), err[keep].max(), (err / np.maximum(bound + slack, 1e-300))[keep].max()))
        assert (keep & nz).sum() >= 0.99 * nz.sum()
        assert (err <= bound + slack)[keep].all()


def _dot(a, b):
    return float((a.double().cpu() * b.double().cpu()).sum())


def test_adjoint_identity_legacy_op(dev):
    case = ('forward', 8, ROI_SHAPES[1][0], ROI_SHAPES[1][1])
    top, rois, shape, a, scale = _inputs(case)
    _, k, sabs, _, _ = _restated(case)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal(shape).astype(np.float32)).to(dev)
    t, r = torch.from_numpy(top).to(dev), torch.from_numpy(rois).to(dev)
    lhs = _dot(forward_cuda(x, r, a, a, scale), t)
    rhs = _dot(x, backward_cuda(t, r, shape, a, a, scale))
    # forward: one output is its exact value within 4 roundings of sum |x w| (three float products, the final cast); summed
    # against |g| that is sum_elements |x| x sum |contribution|, the quantity the backward's own bound multiplies
    bound = float((np.abs(x.cpu().numpy().astype(np.float64)) * sabs * (4 * U + R.gamma(k[:, None] + 3))).sum())
    print('legacy adjoint: %.9e vs %.9e, |diff| %.3e, bound %.3e' % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound and abs(lhs) > 1.0


@pytest.mark.parametrize("take_max", [False, True])
def test_adjoint_identity_pooling(dev, take_max):
    g = torch.Generator().manual_seed(11)
    n = 37 * 5 * 9 * 15
    x = (torch.randperm(n, generator=g).double() / n * 6 - 3).float().reshape(37, 5, 9, 15)      # distinct values: no ties
    gy = torch.randn(37, 5, 8, 14, generator=g)
    assert x.unique().numel() == x.numel()
    xd, gd = x.to(dev), gy.to(dev)
    lhs = _dot(pool_forward(xd, take_max), gd)
    rhs = _dot(xd, pool_backward(gd, xd, take_max))
    ax, ag = x.double().abs(), gy.double().abs()
    if take_max:       # forward exact (a selection); backward: at most 3 additions per lattice point
        bound = 3 * U * float((torch.nn.functional.max_pool2d(ax, 2, 1) * ag).sum())
    else:              # three additions each way (x 0.25 is exact)
        bound = 2 * R.gamma(3) * float((torch.nn.functional.avg_pool2d(ax, 2, 1) * ag).sum())
    print('pool adjoint (max=%d): |diff| %.3e, bound %.3e' % (take_max, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound and abs(lhs) > 1.0


def _pyramid_case(dev, n=96, C=64, B=2, seed=21):
    """rois spread over all four levels of a 320 x 640 input, each well away from a routing boundary"""
    g = np.random.default_rng(seed)
    im_h, im_w = 320.0, 640.0
    side = np.concatenate([g.uniform(12, 42, n // 4), g.uniform(60, 120, n // 4), g.uniform(160, 320, n // 4), g.uniform(420, 600, n // 4)])
    g.shuffle(side)
    aspect = g.uniform(0.6, 1.6, n)
    w, h = side * np.sqrt(aspect), side / np.sqrt(aspect)
    x1, y1 = g.uniform(-10, im_w - 20, n), g.uniform(-10, im_h - 20, n)
    rois = np.stack([g.integers(0, B, n), x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    level, margin = R.pyramid_levels(rois)
    assert margin.min() > 1e-3 and all((level == l).sum() >= n // 8 for l in range(4))
    shapes = [(B, 80, 160), (B, 40, 80), (B, 20, 40), (B, 10, 20)]
    return rois, level, shapes, im_h


@pytest.mark.parametrize("A", [7, 14])
def test_adjoint_identity_fused_pyramid(dev, A):
    C = 64
    rois, level, shapes, im_h = _pyramid_case(dev, C=C)
    g = torch.Generator().manual_seed(A)
    maps = [torch.randn(b, h, w, C, generator=g).to(dev) for b, h, w in shapes]
    gout = torch.randn(len(rois), A, A, C, generator=g).to(dev)
    r = torch.from_numpy(rois).to(dev)
    lhs = _dot(pyramid_forward(maps, r, A, im_h), gout)
    grads = pyramid_backward(gout, C, 0, r, A, C, im_h, shapes)
    rhs = sum(_dot(m, gm) for m, gm in zip(maps, grads))
    # bound: per level, sum |x| x sum |contribution| of the lattice gradient of |g|; forward 4 roundings for the lattice point +
    # 3 for the average, backward 3 for the lattice gradient + gamma_(k+3) for the map sum
    ag = gout.abs().cpu().numpy().transpose(0, 3, 1, 2).astype(np.float64)
    bound = 0.0
    for l, (b, h, w) in enumerate(shapes):
        idx = np.flatnonzero(level == l)
        lat = R.pool2x2_s1_backward_np(ag[idx].reshape(-1, A, A), None, False).reshape(len(idx), C, A + 1, A + 1)
        _, k, sabs, _, _ = R.roi_align_backward_np(lat.astype(np.float32), rois[idx], (b, C, h, w), A + 1, A + 1, np.float32(h / im_h), stats=True)
        ax = np.abs(maps[l].cpu().numpy().astype(np.float64)).transpose(0, 3, 1, 2)
        bound += float((ax * sabs * (7 * U + R.gamma(k[:, None] + 6))).sum()) * (1 + 1e-6)
    print('pyramid adjoint A=%d: %.9e vs %.9e, |diff| %.3e, bound %.3e' % (A, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound and abs(lhs) > 1.0


@pytest.mark.parametrize("A,limited,concat,n_rois", [(7, False, False, 96), (14, False, True, 96), (7, True, True, 96), (7, False, False, 2200),
                                                     (14, True, True, 1300)])
def test_fused_equals_composed(dev, A, limited, concat, n_rois):
    C = 64
    rois, level, shapes, im_h = _pyramid_case(dev, n=n_rois, C=C, seed=33)      # > 1024 rois: several chunks of the kernel's roi list
    n = len(rois)
    cstride, coffset = (2 * C, C) if concat else (C, 0)
    g = torch.Generator().manual_seed(100 + A)
    gout = torch.randn(n, A, A, cstride, generator=g).to(dev)
    r = torch.from_numpy(rois).to(dev)
    n_used = (61 if n < 1024 else 1100) if limited else n
    limit = torch.tensor([n_used], dtype=torch.int32, device=dev) if limited else None
    fused = pyramid_backward(gout, cstride, coffset, r, A, C, im_h, shapes, limit)
    g_nchw = gout[..., coffset:coffset + C].permute(0, 3, 1, 2).contiguous()
    for l, (b, h, w) in enumerate(shapes):
        idx = np.flatnonzero((level == l) & (np.arange(n) < n_used))
        sel = torch.from_numpy(idx).to(dev)
        lat = pool_backward(g_nchw[sel].contiguous(), None, False)
        # the scale the forward uses: mh / im_height in double, narrowed to float at the C boundary
        composed = backward_cuda(lat, r[sel].contiguous(), (b, C, h, w), A + 1, A + 1, float(np.float32(h / im_h)))
        got = fused[l].permute(0, 3, 1, 2).contiguous()
        assert not torch.isnan(got).any()
        assert torch.equal(got.view(torch.int32), composed.view(torch.int32)), 'level %d' % l
        assert (got != 0).any()


def test_autograd_surface(dev):
    from stereo_rcnn_amd.model.roi_align.functions.roi_align import RoIAlignFunction
    from stereo_rcnn_amd.model.roi_align.modules.roi_align import RoIAlign, RoIAlignAvg, RoIAlignMax
    feat_np, rois_np = roi_inputs(8, ROI_SHAPES[1][0])
    scale = 1 / 32.
    feat, rois = torch.from_numpy(feat_np).to(dev), torch.from_numpy(rois_np).to(dev)
    # no_grad / no requires_grad: no grad_fn, and bit-equal to the plain library calls
    plain = pool_forward(forward_cuda(feat, rois, 8, 8, scale), False)
    with torch.no_grad():
        y0 = RoIAlignAvg(7, 7, scale)(feat.clone().requires_grad_(), rois, scale)
    y1 = RoIAlignAvg(7, 7, scale)(feat, rois, scale)
    assert y0.grad_fn is None and y1.grad_fn is None and not y1.requires_grad
    assert torch.equal(y0, plain) and torch.equal(y1, plain)
    # average: autograd == the explicit op.backward path
    f = feat.clone().requires_grad_()
    y = RoIAlignAvg(7, 7, scale)(f, rois, scale)
    assert y.grad_fn is not None and torch.equal(y.detach(), plain)
    y.sum().backward()
    op = RoIAlignFunction(8, 8, scale)
    op.forward(feat, rois)
    explicit, none = op.backward(pool_backward(torch.ones_like(plain), None, False))
    assert none is None and f.grad is not None and (f.grad != 0).any()
    assert torch.equal(f.grad, explicit)
    # the bare lattice, and the function object itself
    f2 = feat.clone().requires_grad_()
    w = torch.randn(len(rois_np), feat.shape[1], 8, 8, device=dev)
    (RoIAlign(8, 8, scale)(f2, rois, scale) * w).sum().backward()
    assert torch.equal(f2.grad, backward_cuda(w, rois, tuple(feat.shape), 8, 8, scale))
    f3 = feat.clone().requires_grad_()
    r3 = rois.clone().requires_grad_()
    out = RoIAlignFunction(8, 8, scale)(f3, r3)
    (out * w).sum().backward()
    assert torch.equal(f3.grad, f2.grad) and r3.grad is None
    with pytest.raises(NotImplementedError):
        RoIAlignFunction(8, 8, scale)(feat.cpu(), rois.cpu())
    # maximum: a feature map with constant patches gives lattices full of ties; the gradient goes where torch's CPU
    # max_pool2d sends it
    tied = feat.clone()
    tied[:, :, 4:14, 10:40] = 1.5
    tied[:, :, :, 50:] = -0.25
    lattice = forward_cuda(tied, rois, 8, 8, scale)
    gy = torch.randn(lattice.shape[0], lattice.shape[1], 7, 7, device=dev)
    lc = lattice.cpu().requires_grad_()
    (torch.nn.functional.max_pool2d(lc, 2, 1) * gy.cpu()).sum().backward()
    assert ((lc.grad != 0).sum(dim=(2, 3)) < 49).any()                    # ties really occur
    routed = pool_backward(gy, lattice, True)
    assert torch.equal(routed.cpu(), lc.grad)
    f4 = tied.clone().requires_grad_()
    (RoIAlignMax(7, 7, scale)(f4, rois, scale) * gy).sum().backward()
    assert torch.equal(f4.grad, backward_cuda(routed, rois, tuple(feat.shape), 8, 8, scale))


@pytest.mark.parametrize("kpts", [False, True])
def test_pyramid_roi_feat_autograd(dev, kpts):
    from stereo_rcnn_amd.model.stereo_rcnn.stereo_rcnn import _StereoRCNN
    C = 64
    A = 14 if kpts else 7
    rois_np, level, shapes, im_h = _pyramid_case(dev, n=48, C=C, seed=44)
    g = torch.Generator().manual_seed(9)
    maps = [torch.randn(b, C, h, w, generator=g).to(dev) for b, h, w in shapes]
    rois = torch.from_numpy(rois_np).to(dev)
    im_info = torch.tensor([[im_h, 640.0, 1.0]])
    feat = lambda ms: _StereoRCNN.PyramidRoI_Feat(None, ms, rois, im_info, kpts=kpts)
    with torch.no_grad():
        y0 = feat([m.clone().requires_grad_() for m in maps])
    y1 = feat(maps)
    nhwc = [m.permute(0, 2, 3, 1).contiguous() for m in maps]
    plain = pyramid_forward(nhwc, rois, A, im_h).permute(0, 3, 1, 2).contiguous()
    assert y0.grad_fn is None and y1.grad_fn is None and torch.equal(y0, plain) and torch.equal(y1, plain)
    leaves = [m.clone().requires_grad_() for m in maps]
    y = feat(leaves)
    assert y.grad_fn is not None and torch.equal(y.detach(), plain)
    w = torch.randn(y.shape, generator=g).to(dev)
    (y * w).sum().backward()
    want = pyramid_backward(w.permute(0, 2, 3, 1).contiguous(), C, 0, rois, A, C, im_h, shapes)
    for leaf, gm in zip(leaves, want):
        assert leaf.grad is not None and (leaf.grad != 0).any()
        assert torch.equal(leaf.grad, gm.permute(0, 3, 1, 2))


def test_crowded_case_is_bit_repeatable_across_runs_and_streams(dev):
    from stereo_rcnn_amd import engine
    top, rois, shape, a, scale = R.crowded_case()
    t, r = torch.from_numpy(top).to(dev), torch.from_numpy(rois).to(dev)
    first = backward_cuda(t, r, shape, a, a, scale)
    second = backward_cuda(t, r, shape, a, a, scale)
    # ... and on a second stream while a convolution of the forward runs on another
    g = torch.Generator().manual_seed(1)
    cw = engine.prep_conv(torch.randn(256, 256, 3, 3, generator=g) * 0.02, None, 1, 1, True, device=dev)
    x = torch.randn(1, 152, 500, 256, generator=g).to(dev)
    y = torch.empty((1, 152, 500, 256), device=dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(3):
            engine.conv2d(cw, x, 1, 152, 500, y, 152, 500, precision='f32')
    with torch.cuda.stream(s2):
        third = backward_cuda(t, r, shape, a, a, scale)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    assert torch.equal(first.view(torch.int32), third.view(torch.int32))
    assert torch.isfinite(y).all()
