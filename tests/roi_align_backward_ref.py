"""Restatements behind the ROIAlign backward tests (numpy / torch only; no product code).

* `roi_align_backward_np`: the DEFINED ARITHMETIC of `roi_align_backward_cuda` (include/srcnn_hip.h): every contribution with the
  reference kernel's float / double promotions, added in float32 in ascending (roi, ph, pw) order starting from 0.  With
  `stats=True` it also returns, from a float64 run alongside, what the derived error bounds need: per element the number of
  contributions k and the sum of |contribution|, the slack a lattice coordinate moved by floating-point contraction allows,
  and the pixels that have a contributing coordinate within that movement of an integer or of the map border.
* `pool2x2_s1_backward_np`: the adjoint of the 2x2 / stride 1 average or maximum in the defined order.
* `roi_align_torch64`: an independent float64 ROIAlign lattice built from differentiable torch ops, so that autograd (not a
  restated formula) supplies the gradient the restatement is pinned against.
* `pyramid_levels`: the level routing in float64 with the distance to the nearest rounding boundary.
"""
import numpy as np
import torch

F = np.float32
U = 2.0 ** -24                       # unit roundoff of float32


def gamma(m):
    """Higham's gamma_m = m u / (1 - m u): the relative error bound of m consecutive float32 roundings."""
    m = np.asarray(m, np.float64)
    return m * U / (1.0 - m * U)


def _ulp(v, eps=0.0):
    """spacing of float32 at |v|, or at |v| + eps: covers both of two values that lie within eps of each other"""
    return float(np.spacing(F(abs(float(v)) + eps)))


def _bin_size(start, end, a):
    """(bin size, how far a build with contraction can move it).  roi_align_kernel.cu:115-118 with C++'s promotions (`1.` is a
    double).  Such a build fuses `coordinate * scale - start` into one rounding (the reference's own kernel built for gfx950 does:
    v_fma_f32 followed by a float add of 1): before rounding the difference moves by at most ulp(end) / 2; every later float
    result (the difference, + 1, / (a - 1)) re-rounds a slightly different input, which adds at most one ulp of that result."""
    d = F(end - start)
    size = max(F(np.float64(d) + 1.), F(0))
    b = F(np.float64(size) / (np.float64(a) - 1.))
    e = 0.5 * _ulp(end)
    e = e + _ulp(d, e)
    e = e + _ulp(size, e)
    e = e / (a - 1.) if a > 1 else 0.0
    e = e + _ulp(b, e)
    return b, e


def roi_geometry(roi, scale, ah, aw):
    """batch index, start_w, start_h, bin_w, bin_h, and the contraction movement of the two bin sizes"""
    s = F(scale)
    sw, sh, ew, eh = F(roi[1]) * s, F(roi[2]) * s, F(roi[3]) * s, F(roi[4]) * s
    bw, dbw = _bin_size(sw, ew, aw)
    bh, dbh = _bin_size(sh, eh, ah)
    return int(roi[0]), sw, sh, bw, bh, dbw, dbh


def lattice_axis(i, bin_size, start, dbin, size):
    """one axis of a lattice point: (inside the map, first tap, weight of the second tap, coordinate, contraction slack, the
    first tap the point would have if a contraction carried it across the map border next to it -- or None)."""
    p = F(F(i) * bin_size)
    v = F(p + start)
    ok = not (v < 0 or v >= size)
    first = int(min(np.floor(v), F(size - 2))) if ok else 0
    ratio = F(v - F(first))
    # A build with contraction forms i * bin + start in one rounding, from a bin size that may itself have moved by dbin: before
    # the last rounding the two coordinates differ by at most i * dbin + ulp(p) / 2 (the un-contracted product's rounding), after
    # it by at most one ulp more.
    e = i * dbin + 0.5 * _ulp(p)
    slack = e + _ulp(v, e)
    across = None
    if abs(float(v)) <= slack:
        across = 0
    elif abs(float(v) - size) <= slack:
        across = size - 2
    return ok, first, ratio, v, slack, across


def roi_align_backward_np(top, rois, shape, ah, aw, scale, stats=False):
    """top (n, C, ah, aw) float32, rois (n, 5), shape (B, C, H, W) -> float32 gradient (B, C, H, W)
    [, k (B, H, W), sum |contribution| (B, C, H, W) float64, coordinate slack (B, C, H, W) float64, fragile (B, H, W) bool]."""
    B, C, H, W = shape
    top = np.asarray(top, F)
    acc = np.zeros((B, H, W, C), F)
    g_all = np.ascontiguousarray(top.transpose(0, 2, 3, 1))
    if stats:
        k = np.zeros((B, H, W), np.int64)
        sabs = np.zeros((B, H, W, C), np.float64)
        slack = np.zeros((B, H, W, C), np.float64)
        fragile = np.zeros((B, H, W), bool)
    for n in range(len(rois)):
        b, sw, sh, bw, bh, dbw, dbh = roi_geometry(rois[n], scale, ah, aw)
        if not 0 <= b < B:
            continue
        cols = [lattice_axis(pw, bw, sw, dbw, W) for pw in range(aw)]
        rows = [lattice_axis(ph, bh, sh, dbh, H) for ph in range(ah)]
        if stats:
            # a point a contraction could carry across the map border: the four elements it then gains or loses
            for okh, hs, _, _, _, ah_ in rows:
                for okw, ws, _, _, _, aw_ in cols:
                    if (ah_ is not None or aw_ is not None) and (okh or ah_ is not None) and (okw or aw_ is not None):
                        y0, x0 = hs if ah_ is None else ah_, ws if aw_ is None else aw_
                        fragile[b, max(y0, 0):y0 + 2, max(x0, 0):x0 + 2] = True
        for ph in range(ah):
            okh, hs, hr, h, dh, _ = rows[ph]
            if not okh:
                continue
            hr1 = 1. - np.float64(hr)
            for pw in range(aw):
                okw, ws, wr, w, dw, _ = cols[pw]
                if not okw:
                    continue
                g = g_all[n, ph, pw]
                wl = F(F(1) - wr)
                up = g.astype(np.float64) * hr1
                down = g * hr                                        # float32 x float32
                acc[b, hs, ws] += (up * np.float64(wl)).astype(F)
                acc[b, hs, ws + 1] += (up * np.float64(wr)).astype(F)
                acc[b, hs + 1, ws] += down * wl
                acc[b, hs + 1, ws + 1] += down * wr
                if stats:
                    a = np.abs(g.astype(np.float64))
                    near = abs(float(h) - round(float(h))) <= dh or abs(float(w) - round(float(w))) <= dw
                    for dy, wy in ((0, 1. - float(hr)), (1, float(hr))):
                        for dx, wx in ((0, 1. - float(wr)), (1, float(wr))):
                            k[b, hs + dy, ws + dx] += 1
                            sabs[b, hs + dy, ws + dx] += a * abs(wy * wx)
                            slack[b, hs + dy, ws + dx] += a * (dh * abs(wx) + dw * abs(wy) + dh * dw)
                            if near:
                                fragile[b, hs + dy, ws + dx] = True
    out = np.ascontiguousarray(acc.transpose(0, 3, 1, 2))
    if not stats:
        return out
    return out, k, sabs.transpose(0, 3, 1, 2), slack.transpose(0, 3, 1, 2), fragile


def backward_bound(k, sabs):
    """|restatement or product - exact| per element: one contribution is at most 3 float32 roundings from its exact value
    (1 - w_ratio, g * h_ratio, the final product / cast; the double products add ~2^-53), the ordered float32 sum of k terms
    k - 1 more: gamma_(k + 3) x sum |contribution| (one spare rounding for the double operations)."""
    return gamma(k[:, None] + 3) * sabs


def pool2x2_s1_backward_np(gy, x, take_max):
    """gy (planes, h-1, w-1), x (planes, h, w) -> (planes, h, w) in the defined order (include/srcnn_hip.h)."""
    gy = np.asarray(gy)
    P, oh, ow = gy.shape
    h, w = oh + 1, ow + 1
    out = np.zeros((P, h, w), gy.dtype)
    seen = np.zeros((P, h, w), bool)
    if take_max:
        win = np.stack([x[:, :-1, :-1], x[:, :-1, 1:], x[:, 1:, :-1], x[:, 1:, 1:]], 0)      # row-major window order
        arg = np.zeros((P, oh, ow), np.int64)
        m = win[0].copy()
        for t in range(1, 4):
            take = (win[t] > m) | np.isnan(win[t])
            m = np.where(take, win[t], m)
            arg = np.where(take, t, arg)
    for q in range(4):                                              # outputs (i-1, j-1), (i-1, j), (i, j-1), (i, j) of lattice point (i, j)
        di, dj = 1 - (q >> 1), 1 - (q & 1)                          # the output's window element that is the lattice point
        sl = (slice(None), slice(di, di + oh), slice(dj, dj + ow))
        if take_max:
            sel = arg == di * 2 + dj
        else:
            sel = np.ones((P, oh, ow), bool)
        cur, s = out[sl], seen[sl]
        out[sl] = np.where(sel, np.where(s, cur + gy, gy), cur)
        seen[sl] = s | sel
    return out if take_max else out * gy.dtype.type(0.25)


def roi_align_torch64(features, rois, ah, aw, scale):
    """features (B, C, H, W) float64 (may require grad), rois (n, 5) -> lattice (n, C, ah, aw) float64.  The lattice
    coordinates are formed in float32 tensors as the kernels form them (so that both sides sample the same points); the
    weights and the blend are exact float64 and differentiable."""
    B, C, H, W = features.shape
    r = torch.as_tensor(np.asarray(rois, F))
    s = torch.tensor(F(scale))
    sw, sh, ew, eh = r[:, 1] * s, r[:, 2] * s, r[:, 3] * s, r[:, 4] * s
    rw = torch.clamp(((ew - sw).double() + 1.).float(), min=0)
    rh = torch.clamp(((eh - sh).double() + 1.).float(), min=0)
    bw = (rw.double() / (float(aw) - 1.)).float()
    bh = (rh.double() / (float(ah) - 1.)).float()
    hh = torch.arange(ah, dtype=torch.float32)[None, :] * bh[:, None] + sh[:, None]          # (n, ah)
    ww = torch.arange(aw, dtype=torch.float32)[None, :] * bw[:, None] + sw[:, None]          # (n, aw)
    okh, okw = ~((hh < 0) | (hh >= H)), ~((ww < 0) | (ww >= W))
    hs = torch.minimum(torch.floor(hh), torch.tensor(float(H - 2))).clamp(min=0).long()
    ws = torch.minimum(torch.floor(ww), torch.tensor(float(W - 2))).clamp(min=0).long()
    hr, wr = hh.double() - hs.double(), ww.double() - ws.double()
    flat = features.reshape(B, C, H * W)[r[:, 0].long()]                                      # (n, C, H W)
    n = r.shape[0]

    def tap(dy, dx):
        idx = ((hs + dy)[:, :, None] * W + (ws + dx)[:, None, :]).reshape(n, 1, ah * aw).expand(n, C, ah * aw)
        return torch.gather(flat, 2, idx).reshape(n, C, ah, aw)

    wy = (1. - hr)[:, None, :, None], hr[:, None, :, None]
    wx = (1. - wr)[:, None, None, :], wr[:, None, None, :]
    v = tap(0, 0) * wy[0] * wx[0] + tap(0, 1) * wy[0] * wx[1] + tap(1, 0) * wy[1] * wx[0] + tap(1, 1) * wy[1] * wx[1]
    return v * (okh[:, None, :, None] & okw[:, None, None, :]).double()


def pyramid_levels(rois):
    """(level 0..3 = P2..P5 per roi, distance of the un-rounded level from the nearest rounding boundary): stereo_rcnn.py:113-119
    in float64.  A test uses rois whose distance is far above float32 rounding, so that every implementation agrees."""
    r = np.asarray(rois, np.float64)
    lv = np.log(np.sqrt((r[:, 4] - r[:, 2] + 1.) * (r[:, 3] - r[:, 1] + 1.)) / 224.) + 4.
    rounded = np.copysign(np.floor(np.abs(lv) + 0.5), lv)
    margin = np.abs(np.abs(lv - np.floor(lv)) - 0.5)
    return (np.clip(rounded, 2, 5) - 2).astype(np.int64), margin


def crowded_case(seed=7):
    """512 rois, 256 channels, a 38 x 125 map, lattice 8; 128 rois share one small box: single elements take thousands of contributions."""
    g = np.random.default_rng(seed)
    n, shape, a, scale = 512, (1, 256, 38, 125), 8, 1 / 16.
    x1, y1 = g.uniform(-20, 1900, n), g.uniform(-20, 560, n)
    rois = np.stack([np.zeros(n), x1, y1, x1 + g.uniform(1, 400, n), y1 + g.uniform(1, 200, n)], 1).astype(F)
    rois[100:228, 1:] = [700.3, 200.7, 730.1, 228.4]                 # 128 rois share one box of about 2 x 2 map pixels
    top = g.standard_normal((n, shape[1], a, a)).astype(F)
    return top, rois, shape, a, scale


def many_rois_case(seed=13):
    """2100 rois (more than two of the kernel's 1024-roi chunks) on a 2 x 4 x 19 x 63 map, lattice 8: the running sum of an element
    is carried from chunk to chunk."""
    g = np.random.default_rng(seed)
    n, shape, a, scale = 2100, (2, 4, 19, 63), 8, 1 / 32.
    x1, y1 = g.uniform(-20, 1900, n), g.uniform(-20, 560, n)
    rois = np.stack([g.integers(0, 2, n), x1, y1, x1 + g.uniform(1, 600, n), y1 + g.uniform(1, 300, n)], 1).astype(F)
    top = g.standard_normal((n, shape[1], a, a)).astype(F)
    return top, rois, shape, a, scale
