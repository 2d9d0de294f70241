"""CPU: argument checks of the ROIAlign backward ABI (validated before any launch), and the numpy restatement of its defined
arithmetic pinned by something independent -- float64 torch autograd through a ROIAlign written from torch ops -- before the
GPU tests trust it."""
import ctypes

import numpy as np
import pytest
import torch

import roi_align_backward_ref as R


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import _lib
    return _lib.lib()


def test_backward_argument_errors_without_gpu(L):
    from stereo_rcnn_amd import _lib
    assert L.roi_align_backward_cuda(8, 8, 1.0, None, None, 3, 4, None, 1, 1, 4, 4, None) == 0      # roi_cols != 5
    assert L.roi_align_backward_cuda(8, 8, 1.0, None, None, 3, 6, None, 1, 1, 4, 4, None) == 0
    ptrs = (ctypes.c_void_p * 4)(256, 256, 256, 256)
    mh, mw = (ctypes.c_int * 4)(8, 4, 2, 1), (ctypes.c_int * 4)(8, 4, 2, 1)
    rc = L.srcnn_pyramid_roi_align_backward(None, 64, 0, None, 1, 7, 64, 32.0, ptrs, mh, mw, 1, _lib.FMT_SPLIT16, None, None)
    assert rc == -1 and b'F32 only' in L.srcnn_last_error()
    rc = L.srcnn_pyramid_roi_align_backward(None, 64, 0, None, 1, 9, 64, 32.0, ptrs, mh, mw, 1, _lib.FMT_F32, None, None)
    assert rc == -1 and b'A must be 7 or 14' in L.srcnn_last_error()
    rc = L.srcnn_pyramid_roi_align_backward(None, 64, 32, None, 1, 7, 64, 32.0, ptrs, mh, mw, 1, _lib.FMT_F32, None, None)
    assert rc == -1 and b'slice' in L.srcnn_last_error()
    assert L.srcnn_pool2x2_s1_backward(None, None, 1, 8, 8, None, 0, None) == -1
    assert L.srcnn_pool2x2_s1_backward(256, None, 1, 8, 8, 256, 1, None) == -1 and b'needs the forward' in L.srcnn_last_error()
    assert L.srcnn_pool2x2_s1_backward(256, None, 1, 1, 8, 256, 0, None) == -1


def _small_case(seed, shape, a, scale, n=12):
    g = np.random.default_rng(seed)
    B, C, H, W = shape
    x1, y1 = g.uniform(-2 / scale, (W - 2) / scale, n), g.uniform(-2 / scale, (H - 2) / scale, n)
    rois = np.stack([g.integers(0, B, n), x1, y1, x1 + g.uniform(1, W / scale / 2, n), y1 + g.uniform(1, H / scale / 2, n)],
                    1).astype(np.float32)
    rois[0, 1:] = [10, 10, 10, 10]                                                # degenerate
    rois[1, 1:] = [(W - 1) / scale, (H - 1) / scale, (W + 5) / scale, (H + 5) / scale]    # hangs over the border
    rois[2] = rois[3]                                                             # a shared box
    top = g.standard_normal((n, C, a, a)).astype(np.float32)
    return top, rois


@pytest.mark.parametrize("shape,scale,a", [((1, 3, 12, 17), 1 / 16., 8), ((2, 2, 9, 11), 1 / 4., 15), ((1, 2, 6, 6), 1 / 8., 3)])
def test_restatement_against_float64_autograd(shape, scale, a):
    top, rois = _small_case(a + shape[2], shape, a, scale)
    got, k, sabs, _, _ = R.roi_align_backward_np(top, rois, shape, a, a, scale, stats=True)
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    lat = R.roi_align_torch64(x, rois, a, a, scale)
    (lat * torch.from_numpy(top).double()).sum().backward()
    want = x.grad.numpy()
    bound = R.backward_bound(k, sabs)
    err = np.abs(got.astype(np.float64) - want)
    print('max |restatement - autograd| %.3e, max bound %.3e, max k %d' % (err.max(), bound.max(), k.max()))
    assert k.max() > 4 and (want != 0).any()
    assert (err <= bound).all(), float((err - bound).max())
    # the bound's ingredient is pinned too: autograd run on |top| gives the signed-weight sum, which the sum of |contribution|
    # dominates (the two differ only where a clamped tap has a weight outside [0, 1])
    x2 = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    (R.roi_align_torch64(x2, rois, a, a, scale) * torch.from_numpy(np.abs(top)).double()).sum().backward()
    signed = x2.grad.numpy()
    assert (sabs >= np.abs(signed) * (1 - 1e-12)).all() and np.isclose(sabs, signed, rtol=1e-12).mean() > 0.5


@pytest.mark.parametrize("take_max", [False, True])
def test_pool_backward_restatement_against_torch(take_max):
    g = np.random.default_rng(3)
    x = g.standard_normal((6, 9, 7))
    if take_max:
        x[0, 2:4, 2:4] = 5.0                    # a window of four equal maxima, and its neighbours
        x[1, 0, 0] = x[1, 0, 1] = 7.0
        x[2, 4, 4] = np.nan
        x[3, 3, 3] = x[3, 3, 4] = np.nan        # two NaNs in one window: the later one takes the gradient
    gy = g.standard_normal((6, 8, 6))
    t = torch.from_numpy(x).requires_grad_()
    pool = torch.nn.functional.max_pool2d if take_max else torch.nn.functional.avg_pool2d
    (pool(t[None], 2, 1)[0] * torch.from_numpy(gy)).sum().backward()
    got = R.pool2x2_s1_backward_np(gy, x, take_max)
    assert np.allclose(got, t.grad.numpy(), rtol=1e-13, atol=1e-13)


def test_crowded_case_is_crowded_and_mostly_robust_to_contraction():
    """The GPU test's claims about its inputs, confirmed from the restatement alone on a channel subset (k, the fragile set and
    the routing do not depend on the channel)."""
    top, rois, shape, a, scale = R.crowded_case()
    assert len(rois) == 512 and shape == (1, 256, 38, 125) and a == 8
    assert (rois[100:228, 1:] == rois[100, 1:]).all()                  # >= 64 rois share one box
    sub = (1, 2) + shape[2:]
    got, k, sabs, slack, fragile = R.roi_align_backward_np(top[:, :2], rois, sub, a, a, scale, stats=True)
    print('max contributions to one element: %d' % k.max())
    assert k.max() >= 2000, k.max()
    nz = (got != 0) & np.broadcast_to(k[:, None] > 0, got.shape)
    robust = nz & ~np.broadcast_to(fragile[:, None], got.shape)
    print('robust to contraction: %d of %d non-zero elements' % (robust.sum(), nz.sum()))
    assert robust.sum() >= 0.99 * nz.sum(), (robust.sum(), nz.sum())


def _fma(a, b, c):
    """float32 fused multiply-add (the float64 product of two float32 values is exact)"""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def _contracted_geometry(roi, scale, ah, aw):
    """what the reference's kernel built with contraction computes: end * scale - start in one rounding"""
    f = np.float32
    s = f(scale)
    sw, sh = f(roi[1]) * s, f(roi[2]) * s
    size = [max(f(_fma(f(roi[i]), s, -st) + f(1)), f(0)) for i, st in ((3, sw), (4, sh))]
    bw = f(np.float64(size[0]) / (np.float64(aw) - 1.))
    bh = f(np.float64(size[1]) / (np.float64(ah) - 1.))
    return int(roi[0]), sw, sh, bw, bh, 0.0, 0.0


def _contracted_axis(i, bin_size, start, dbin, size):
    """... and i * bin + start in one rounding"""
    v = _fma(np.float32(i), bin_size, start)
    ok = not (v < 0 or v >= size)
    first = int(min(np.floor(v), np.float32(size - 2))) if ok else 0
    return ok, first, np.float32(v - np.float32(first)), v, 0.0, None


def _gpu_cases():
    from test_ref_kernels_gpu import ROI_SHAPES, ROI_SIZES, roi_inputs
    for shape, scale in ROI_SHAPES:
        for a in ROI_SIZES:
            rois = roi_inputs(a, shape)[1]
            c = min(shape[1], 2)
            top = np.random.default_rng(a).standard_normal((len(rois), c, a, a)).astype(np.float32)
            yield top, rois, (shape[0], c) + shape[2:], a, scale
    top, rois, shape, a, scale = R.crowded_case()
    yield top[:, :2], rois, (1, 2) + shape[2:], a, scale
    top, rois, shape, a, scale = R.many_rois_case()
    yield top[:, :2], rois, shape[:1] + (2,) + shape[2:], a, scale


def test_contraction_slack_and_fragile_set_on_the_gpu_tests_inputs(monkeypatch):
    """For every input of the live comparison with the reference's contracted build, from the restatement alone: the elements
    left out as fragile are under 1 % of the non-zero ones, and on the others a restatement with the two contractions that build
    performs (fused `end * scale - start`, fused `i * bin + start`) stays within the derived slack of the un-contracted one (same
    summation order on both sides, so only the roundings of the sum, gamma_k, come on top)."""
    for top, rois, shape, a, scale in _gpu_cases():
        base, k, sabs, slack, fragile = R.roi_align_backward_np(top, rois, shape, a, a, scale, stats=True)
        with monkeypatch.context() as m:
            m.setattr(R, 'roi_geometry', _contracted_geometry)
            m.setattr(R, 'lattice_axis', _contracted_axis)
            con = R.roi_align_backward_np(top, rois, shape, a, a, scale)
        kk = np.broadcast_to(k[:, None], base.shape)
        keep = ~np.broadcast_to(fragile[:, None], base.shape)
        nz = (base != 0) & (kk > 0)
        err = np.abs(base.astype(np.float64) - con)
        bound = 2 * R.gamma(kk) * sabs + slack
        print('a=%d %s: %d of %d non-zero elements kept, max err / bound %.3f, contraction moved %d elements'
              % (a, shape, (keep & nz).sum(), nz.sum(), (err / np.maximum(bound, 1e-300))[keep].max(), (err > 0).sum()))
        assert (keep & nz).sum() >= 0.99 * nz.sum()
        assert (err <= bound)[keep].all()
        assert (err > 0).any()
