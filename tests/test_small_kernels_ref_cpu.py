"""Pins the plain references of tests/small_kernels_ref.py against independent CPU code, so that a wrong reference cannot bless a
wrong kernel in tests/test_small_kernels_gpu.py: torch.softmax in float64, F.max_pool2d ceil-mode, F.interpolate
(align_corners=True) in float64, oracle.postprocess, oracle.ops.nms and numpy.float16.  The derived error bounds are checked from
both sides: a float32 numpy evaluation of the same expression stays inside them, and they stay small."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_kernels_ref as R
from oracle import config as ocfg
from oracle import ops as oops
from oracle import postprocess as opost


def _logit_rows(rng, rows, cols):
    x = rng.normal(0, 3, (rows, cols)).astype(np.float32)
    x[0] = 1.25                                     # equal logits
    if rows > 1:
        x[1] = np.linspace(-80, 80, cols)           # spread over +-80
    if rows > 2:
        x[2] = -200.0
        x[2, cols // 2] = 30.0                      # one dominating logit
    return x


@pytest.mark.parametrize("cols", [1, 2, 4, 7, 112])
def test_softmax_rows_is_torch_softmax_in_float64(cols):
    x = _logit_rows(np.random.default_rng(cols), 9, cols)
    want = torch.softmax(torch.from_numpy(x).double(), 1).numpy()
    got = R.softmax_rows(x)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=1e-300)
    assert np.abs(got.sum(1) - 1).max() < 1e-14


@pytest.mark.parametrize("cols", [1, 2, 7, 112])
def test_softmax_bound_holds_a_float32_evaluation_and_stays_small(cols):
    """numpy's float32 exp is itself within an ulp, so the kernels' expression evaluated in float32 on the CPU must sit inside
    the derived bound; and the bound must stay near float32 precision -- it is no tolerance that a wrong group could hide in."""
    x = _logit_rows(np.random.default_rng(cols + 50), 64, cols)
    d = x - x.max(1, keepdims=True)
    e = np.exp(d, dtype=np.float32)
    s = np.zeros(len(x), np.float32)
    for c in range(cols):
        s = s + e[:, c]
    got = e / s[:, None]
    ref, bound = R.softmax_rows(x), R.softmax_bound(x)
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    big = ref > 1e-30
    assert (bound[big] / ref[big]).max() <= (160 + cols + 3) * 2.0 ** -23 * 1.001


@pytest.mark.parametrize("G", [1, 2, 7, 28])
def test_kpts_tail_is_the_oracle_heads_expression(G):
    """oracle/net.py kpts_head after the class conv: sum over H, view (n, 6, G), softmax of channels 0-3 as 4 G bins, 4, 5."""
    rng = np.random.default_rng(G)
    lg = rng.normal(0, 1, (3, G, G, 6)) + 10.0 * np.arange(6) / G
    t = torch.from_numpy(lg).permute(0, 3, 1, 2)                     # (n, 6, h, w) as the reference network holds it
    allp = t.sum(2)
    want_k = F.softmax(allp[:, :4, :].contiguous().view(-1, 4 * G), 1).numpy()
    want_l = F.softmax(allp[:, 4, :].contiguous().view(-1, G), 1).numpy()
    want_r = F.softmax(allp[:, 5, :].contiguous().view(-1, G), 1).numpy()
    k, l, r, col = R.kpts_tail(lg)
    np.testing.assert_allclose(k, want_k, rtol=1e-12)
    np.testing.assert_allclose(l, want_l, rtol=1e-12)
    np.testing.assert_allclose(r, want_r, rtol=1e-12)
    np.testing.assert_allclose(col, allp.numpy(), rtol=1e-13)


def test_split16_is_numpy_float16_twice_in_the_documented_layout():
    x = np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.996,
                  6e-8, 2.0 ** -24, 2.0 ** -25, 1e-8, -3.1415927, 1000.123, 5e-5, -65504.0], np.float32).reshape(1, 16)
    hi, lo = R.split16_halves(x)
    assert hi.dtype == np.float16 and lo.dtype == np.float16
    assert hi[0, 3] == np.float16(1.0) and hi[0, 4] == np.float16(1.0) + np.float16(2.0 ** -10)      # tie to even / just above
    assert hi[0, 5] == np.float16(1.0 + 2.0 ** -9)                                                   # tie to even, upwards
    assert hi[0, 7] == np.float16(65504.0) and np.isfinite(lo[0, 7])
    assert np.signbit(hi[0, 1]) and hi[0, 1] == 0
    assert hi[0, 11] == 0 and lo[0, 11] == 0                                                         # 1e-8: below half the smallest subnormal
    raw = R.split16_pack(x)
    assert raw.dtype == np.float32 and raw.shape == x.shape
    b = raw.view(np.float16).reshape(2, 2, 8)                         # two groups of 32 bytes: [8 hi][8 lo] each
    assert np.array_equal(b[:, 0, :].view(np.uint16), hi.reshape(2, 8).view(np.uint16))
    assert np.array_equal(b[:, 1, :].view(np.uint16), lo.reshape(2, 8).view(np.uint16))
    back = R.split16_unpack(raw)
    assert np.array_equal(back, hi.astype(np.float32) + lo.astype(np.float32))
    assert (np.abs(back.astype(np.float64) - x) <= R.split16_step(x)).all()
    # beyond the format: 65520 rounds to inf and reads back as NaN (inf + -inf)
    bad = np.full((1, 8), 65520.0, np.float32)
    assert np.isinf(R.split16_halves(bad)[0]).all() and np.isnan(R.split16_unpack(R.split16_pack(bad))).all()


@pytest.mark.parametrize("H,W", [(3, 3), (4, 4), (5, 5), (4, 7), (7, 4), (6, 9), (75, 131)])
def test_maxpool_is_torch_ceil_mode(H, W):
    rng = np.random.default_rng(H * 10 + W)
    x = (rng.normal(0, 1, (2, H, W, 8)) - 5.0).astype(np.float32)            # all negative
    want = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 3, 2, 0, ceil_mode=True)
    assert (R.ceil_pool_out(H), R.ceil_pool_out(W)) == tuple(want.shape[2:])
    assert np.array_equal(R.maxpool3x3s2_ceil(x), want.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("TH,TW,H,W", [(1, 1, 3, 5), (1, 4, 2, 7), (3, 1, 5, 1), (3, 4, 3, 4), (3, 4, 5, 7), (7, 5, 19, 11),
                                       (2, 2, 1, 1), (19, 63, 38, 125)])
def test_upsample_add_is_interpolate_align_corners_in_float64(TH, TW, H, W):
    """F.interpolate in float64 computes the source position in float64; the reference (like ATen's float path and the kernel)
    in float32.  A position r * i carries two float32 roundings (<= 2^-23 relative, so <= 2^-23 * TH rows or TW columns), and
    the interpolant moves by at most 2 max|top| per unit of position in each direction -- across a truncation boundary too, it
    is continuous; 1 - lambda adds one more rounding of the weights.  Hence 2^-21 * (TH + TW) * max|top|."""
    rng = np.random.default_rng(TH * 100 + H)
    top = rng.normal(0, 2, (2, TH, TW, 8)).astype(np.float32)
    lat = rng.normal(0, 2, (2, H, W, 8)).astype(np.float32)
    up = F.interpolate(torch.from_numpy(top).double().permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=True)
    want = up.permute(0, 2, 3, 1).numpy() + lat.astype(np.float64)
    got, mag = R.upsample_add(top, lat)
    assert got.dtype == np.float64
    assert np.abs(got - want).max() <= 2.0 ** -21 * (TH + TW) * np.abs(top).max()
    assert (mag >= np.abs(got) * (1 - 1e-12)).all()
    if (TH, TW) == (H, W):
        assert np.array_equal(got, top.astype(np.float64) + lat)
    # the kernel's expression in float32 sits inside the derived bound
    t = torch.from_numpy(top)
    h0, h1, a0, a1 = R._taps(TH, H)
    w0, w1, b0, b1 = R._taps(TW, W)
    f = lambda a: torch.from_numpy(a.astype(np.float32))
    a0, a1, b0, b1 = f(a0)[None, :, None, None], f(a1)[None, :, None, None], f(b0)[None, None, :, None], f(b1)[None, None, :, None]
    y32 = (a0 * (b0 * t[:, h0][:, :, w0] + b1 * t[:, h0][:, :, w1]) + a1 * (b0 * t[:, h1][:, :, w0] + b1 * t[:, h1][:, :, w1])) \
        + torch.from_numpy(lat)
    assert (np.abs(y32.numpy().astype(np.float64) - got) <= R.upsample_add_bound(mag)).all()


@pytest.mark.parametrize("TH,TW,H,W", [(1, 1, 3, 5), (1, 4, 2, 7), (3, 1, 5, 1), (3, 4, 3, 4), (3, 4, 5, 7), (7, 5, 19, 11), (2, 2, 1, 1)])
def test_upsample_add_f32_restatement_lies_within_the_bound_of_float64(TH, TW, H, W):
    """The float32 restatement the GPU test compares bits with is itself tied to the float64 reference: inside upsample_add_bound
    on the GPU test's shapes; the identity size is top + lateral exactly."""
    for B in (1, 3):
        for C in (8, 24):
            rng = np.random.default_rng(TH * 1000 + H * 10 + B + C)
            top = rng.normal(0, 30, (B, TH, TW, C)).astype(np.float32)
            lat = rng.normal(0, 30, (B, H, W, C)).astype(np.float32)
            y32 = R.upsample_add_f32(top, lat)
            ref, mag = R.upsample_add(top, lat)
            assert y32.dtype == np.float32 and y32.shape == ref.shape
            assert (np.abs(y32.astype(np.float64) - ref) <= R.upsample_add_bound(mag)).all()
            if (TH, TW) == (H, W):
                assert np.array_equal(y32, top + lat)


def test_subsample_and_transposes_are_slicing_and_permute():
    x = torch.arange(2 * 5 * 7 * 4, dtype=torch.float32).view(2, 5, 7, 4)
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 1, 2).permute(0, 2, 3, 1)
    assert np.array_equal(R.subsample2(x.numpy()), want.numpy())
    assert np.array_equal(R.nhwc_to_nchw(x.numpy()), x.permute(0, 3, 1, 2).contiguous().numpy())
    assert np.array_equal(R.nchw_to_nhwc(x.numpy()), x.permute(0, 2, 3, 1).contiguous().numpy())
    assert R.nchw_to_nhwc(x.numpy()).flags['C_CONTIGUOUS']


@pytest.mark.parametrize("B,h,w", [(1, 1, 1), (2, 2, 3), (2, 5, 7)])
def test_rpn_score_is_the_oracles_reshape_softmax(B, h, w):
    """oracle/net.py rpn_head: F.softmax(score.view(b, 2, 3h, w), 1).view(b, 6, h, w), then the NHWC flatten in pairs."""
    rng = np.random.default_rng(h * w)
    head = (rng.normal(0, 3, (B, h * w, 24))).astype(np.float32)
    nchw = torch.from_numpy(head).double().view(B, h, w, 24).permute(0, 3, 1, 2)
    score, delta = nchw[:, :6].contiguous(), nchw[:, 6:].contiguous()
    prob = F.softmax(score.view(B, 2, 3 * h, w), 1).view(B, 6, h, w)
    want_p = prob.permute(0, 2, 3, 1).contiguous().view(B, -1, 2).numpy()
    want_d = delta.permute(0, 2, 3, 1).contiguous().view(B, -1, 6).numpy()
    p, d, bound = R.rpn_score(head)
    np.testing.assert_allclose(p, want_p, rtol=1e-13)
    assert d.dtype == np.float32 and np.array_equal(d.astype(np.float64), want_d)
    assert bound.shape == p.shape and (bound > 0).all()


def _decode_inputs(rng, n, n_cls, G):
    x1 = rng.uniform(0, 500, n); y1 = rng.uniform(0, 150, n)
    rl = np.stack([np.zeros(n), x1, y1, x1 + rng.uniform(0, 200, n), y1 + rng.uniform(0, 80, n)], 1).astype(np.float32)
    rr = rl.copy()
    rr[:, [1, 3]] -= rng.uniform(0, 30, (n, 1)).astype(np.float32)
    return (rl, rr, rng.normal(0, 1, (n, 6 * n_cls)).astype(np.float32), rng.normal(0, 1, (n, 5 * n_cls)).astype(np.float32),
            rng.uniform(0, 1, (n, 4 * G)).astype(np.float32), rng.uniform(0, 1, (n, G)).astype(np.float32),
            rng.uniform(0, 1, (n, G)).astype(np.float32), np.array([192.0, 640.0, 1.6], np.float32))


def test_decode_reference_is_the_oracle_and_restores_its_grid():
    rng = np.random.default_rng(0)
    args = _decode_inputs(rng, 17, 2, ocfg.KPTS_GRID)
    t = torch.from_numpy
    out = {'cls_prob': torch.zeros(1, 17, 2), 'rois_left': t(args[0])[None], 'rois_right': t(args[1])[None], 'bbox_pred': t(args[2])[None],
           'dim_orien_pred': t(args[3])[None], 'kpts_prob': t(args[4]), 'left_border_prob': t(args[5]), 'right_border_prob': t(args[6])}
    want = opost.decode_detections(out, t(args[7]).view(1, 3))
    got = R.decode_detections(*args, n_cls=2, G=ocfg.KPTS_GRID)
    for k in got:
        assert np.array_equal(got[k], want[k].numpy()), k
    R.decode_detections(*_decode_inputs(rng, 5, 4, 7), n_cls=4, G=7)
    assert ocfg.KPTS_GRID == 28


def test_the_oracles_argmax_takes_the_first_of_equal_maxima():
    """The decode takes torch.max(...)[1] on the CPU: with two or three equal maxima, and with an all-zero row (the lazy
    keypoint path), it returns the FIRST index -- which is what argmax_first in csrc/heads.hip implements (strict >)."""
    G = 7
    rl, rr, bp, dp, kp, lp, rp, info = _decode_inputs(np.random.default_rng(1), 4, 1, G)
    kp[:] *= 0.5; lp[:] *= 0.5; rp[:] *= 0.5
    kp[0, [9, 20]] = 0.75; lp[0, [2, 5]] = 0.75; rp[0, [1, 6]] = 0.75
    kp[1, [3, 10, 27]] = 0.875; lp[1, [0, 3, 4]] = 0.875; rp[1, [4, 5, 6]] = 0.875
    kp[2] = 0; lp[2] = 0; rp[2] = 0
    assert torch.max(torch.from_numpy(kp), 1)[1].tolist()[:3] == [9, 3, 0]
    assert R.argmax_first(kp).tolist()[:3] == [9, 3, 0] and R.argmax_first(lp).tolist()[:3] == [2, 0, 0]
    k = R.decode_detections(rl, rr, bp, dp, kp, lp, rp, info, 1, G)['kpts']
    w = rl[:, 3] - rl[:, 1] + 1.0
    assert k[:3, 1].tolist() == [np.float32(9) / np.float32(7), np.float32(3) / np.float32(7), 0.0]
    assert k[:3, 2].tolist() == [0.75, 0.875, 0.0]
    want_lb = ((np.array([2, 0, 0], np.float32) * w[:3] / np.float32(G) + rl[:3, 1]) / info[2]).astype(np.float32)
    want_rb = ((np.array([1, 4, 0], np.float32) * w[:3] / np.float32(G) + rl[:3, 1]) / info[2]).astype(np.float32)
    assert np.array_equal(k[:3, 3], want_lb) and np.array_equal(k[:3, 4], want_rb)


def _rand_dets(rng, n, w=1987.0, h=600.0):
    nc = max(1, n // 12)
    cx = rng.uniform(0, w, nc); cy = rng.uniform(0, h, nc); s = rng.uniform(16, 300, nc)
    idx = rng.integers(0, nc, n)
    x = cx[idx] + rng.normal(0, 0.15, n) * s[idx]; y = cy[idx] + rng.normal(0, 0.15, n) * s[idx]
    bw = s[idx] * rng.uniform(0.7, 1.4, n); bh = s[idx] * rng.uniform(0.5, 1.2, n)
    b = np.stack([x - bw / 2, y - bh / 2, x + bw / 2, y + bh / 2], 1)
    return np.clip(b, 0, [w - 1, h - 1, w - 1, h - 1]).astype(np.float32)


@pytest.mark.parametrize("n,n_cls,j", [(1, 2, 1), (2, 2, 1), (300, 4, 3), (300, 4, 1)])
@pytest.mark.parametrize("pattern", ["quantised", "equal", "none", "at_threshold"])
def test_class_nms_reference_is_the_oracles_filter_sort_nms(n, n_cls, j, pattern):
    """Against oracle.postprocess.class_detections (demo.py:231-251 restated with torch.sort(stable=True) and oracle.ops.nms),
    and against the pure-Python greedy NMS behind it."""
    rng = np.random.default_rng(n + j)
    scores = rng.uniform(0, 1, (n, n_cls)).astype(np.float32)
    boxes = np.concatenate([_rand_dets(rng, n) for _ in range(n_cls)], 1)
    if pattern == "quantised":
        scores[:, j] = np.round(scores[:, j], 2)
    elif pattern == "equal":
        scores[:, j] = 0.5
    elif pattern == "none":
        scores[:, j] = 0.01
    else:
        scores[:, j] = np.float32(0.05)              # equal to the threshold: excluded by the strict comparison
        scores[n // 2, j] = 0.9
    det = {'scores': torch.from_numpy(scores), 'boxes_left': torch.from_numpy(boxes), 'boxes_right': torch.from_numpy(boxes),
           'dim_orien': torch.zeros(n, 5 * n_cls), 'kpts': torch.zeros(n, 5)}
    want = opost.class_detections(det, j=j, thresh=0.05, nms_thresh=0.3)
    chain = want['inds'][want['order']].numpy()[want['keep']] if want['inds'].numel() else np.zeros(0, np.int64)
    keep_idx, num = R.class_nms(scores, boxes, j, 0.05, 0.3)
    assert num == len(chain) and np.array_equal(keep_idx[:num], chain) and (keep_idx[num:] == -1).all()
    keep_py, num_py = R.class_nms(scores, boxes, j, 0.05, 0.3, nms=oops.nms_py)
    assert num_py == num and np.array_equal(keep_py, keep_idx)
    if pattern == "none":
        assert num == 0
    if pattern == "at_threshold":
        assert num == 1 and keep_idx[0] == n // 2
    # record layout against the oracle's gathers
    kp = rng.normal(0, 1, (n, 5)).astype(np.float32)
    do = rng.normal(0, 1, (n, 5 * n_cls)).astype(np.float32)
    det['kpts'], det['dim_orien'] = torch.from_numpy(kp), torch.from_numpy(do)
    want = opost.class_detections(det, j=j, thresh=0.05, nms_thresh=0.3)
    rec = R.pack_detections(scores, boxes, boxes, do, kp, keep_idx, num, j, 24, flag=3.0)
    assert rec.shape == (n + 1, 24) and rec[0, 0] == num and rec[0, 1] == 3.0 and not rec[0, 2:].any() and not rec[1 + num:].any()
    if num:
        assert np.array_equal(rec[1:1 + num, 1:5], want['dets_left'][:, :4].numpy()) and np.array_equal(rec[1:1 + num, 0], want['dets_left'][:, 4].numpy())
        assert np.array_equal(rec[1:1 + num, 5:9], want['dets_right'][:, :4].numpy())
        assert np.array_equal(rec[1:1 + num, 9:14], want['dim_orien'].numpy()) and np.array_equal(rec[1:1 + num, 14:19], want['kpts'].numpy())
        assert np.array_equal(rec[1:1 + num, 19], keep_idx[:num].astype(np.float32)) and not rec[:, 20:].any()
