"""Stage-level references for csrc/dense_align.hip (TEST INFRASTRUCTURE ONLY; numpy only).

One function per stage of the pipeline, each a plain restatement of the operation, so that a stage can be compared on its own:
  upsample2x_f32 / upsample2x_f64   `upsample2x_kernel` (F.upsample, bilinear, align_corners=True)
  lattice_f64                       `sample_kernel`: slice arithmetic, box vertices, nearest-vertex plane group, ray
                                    intersection, in-box test -- with the DECISION MARGIN of every lattice pixel
  taps_f64                          `grid_taps` / `sample_plane`: border-clamped bilinear taps
  tap_coords                        the pixel coordinate a hypothesis reads (`unnorm` of `left_sample_kernel` / `cost_kernel`)
  cost_f64                          `cost_kernel`: SAD over an object's valid pixels for one depth hypothesis
It follows oracle/dense_align.py and dense_align.hip; float64 throughout except where a function says float32.

DOMAIN: box and border coordinates are non-negative.  The kernel clamps slice bounds with max(.., 0) where Python slicing would
count a negative bound from the END of the axis; the two agree only for non-negative bounds, and `lattice_f64` asserts that.

What is an INPUT and therefore taken in the format the device is given it: the float32 boxes / borders / poses, and the float32
product `box * scale` (dense_align.py:261-262 multiplies float32 tensors; the slice arithmetic that follows is in doubles on
those float32 values, here as there -- an integer truncation admits no tolerance).
"""
import math

import numpy as np

PLANE_GROUP = [[0, 3, 4], [2, 3, 4], [1, 2, 4], [0, 1, 4], [0, 3, 5], [2, 3, 5], [1, 2, 5], [0, 1, 5]]   # box_3d.py:88-96
PLANE_TRI = [[0, 3, 4], [2, 3, 6], [1, 2, 5], [0, 1, 4], [0, 1, 2], [4, 5, 6]]                           # box_3d.py:47-52
DOUBLE_EPS = 0.01


# ------------------------------------------------------------------ upsample
def _axis_f32(n):
    f = np.float32
    r = f(n - 1) / f(2 * n - 1)                              # one float32 division
    pr = r * np.arange(2 * n).astype(f)                      # rh * y: a float32 product
    i0 = pr.astype(np.int32)                                 # truncation
    step = (i0 < n - 1).astype(np.int32)
    l1 = pr - i0.astype(f)
    l0 = f(1) - l1
    assert pr.dtype == f and l1.dtype == f and l0.dtype == f
    return i0, step, l0, l1


def _axis_f64(n):
    pr = (float(n - 1) / float(2 * n - 1)) * np.arange(2 * n).astype(np.float64)
    i0 = pr.astype(np.int64)
    step = (i0 < n - 1).astype(np.int64)
    l1 = pr - i0
    return i0, step, 1.0 - l1, l1


def _upsample(img, axis):
    C, H, W = img.shape
    h1, h1p, h0l, h1l = axis(H)
    w1, w1p, w0l, w1l = axis(W)
    h0l, h1l = h0l[None, :, None], h1l[None, :, None]
    w0l, w1l = w0l[None, None, :], w1l[None, None, :]
    p00 = img[:, h1][:, :, w1]
    p01 = img[:, h1][:, :, w1 + w1p]
    p10 = img[:, h1 + h1p][:, :, w1]
    p11 = img[:, h1 + h1p][:, :, w1 + w1p]
    # the blend of upsample2x_at, parenthesised as there; every numpy operation on same-typed arrays rounds once (no FMA)
    return h0l * (w0l * p00 + w1l * p01) + h1l * (w0l * p10 + w1l * p11)


def upsample2x_f32(img):
    """(C, H, W) float32 -> (C, 2H, 2W) float32: `upsample2x_at` operation by operation in float32."""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.float32
    out = _upsample(img, _axis_f32)
    assert out.dtype == np.float32
    return out


def upsample2x_f64(img):
    """The same interpolation with float64 weights and a float64 blend."""
    return _upsample(np.asarray(img, np.float64), _axis_f64)


def upsample_bound(H, W, src_absmax):
    """Bound on |upsample2x_f32 - upsample2x_f64|, u = 2^-24.  A weight comes from `rh * y`, a float32 product below H (W): the
    quotient rh carries a relative u and the product another, so the weight is off by e < 2 u H = H 2^-23 (W 2^-23).  A weight
    error e moves a blend (1 - l) a + l b by e |b - a|, and neighbouring source values differ by at most max|src| = M in the
    images this is used on (non-negative or smooth ones; the tests assert it where it is not evident), so both axes together
    move the value by (H + W) 2^-23 M.  The blend itself (`1 - l`, four products, three sums) adds a few u M: 8 u M.  Where the
    truncation of `rh * y` lands on the other side of an integer the weight pair swaps continuously (l = 1 - e on the lower
    cell is l = e on the upper), so nothing is excepted.  Total: ((2 (H + W)) + 8) 2^-24 M."""
    return ((2.0 * (H + W)) + 8.0) * 2.0 ** -24 * float(src_absmax)


# ------------------------------------------------------------------ lattice
def lattice_slices(scale, H2, W2, box, border):
    """dense_align.py:42-45 on one object: (r0, r1, hstep, c0, c1, wstep) with Python's slice clamping applied.
    box (4) / border (2) float32, original-image pixels; scale = im_info[0,2] (the doubling is done here)."""
    sc = np.float32(float(scale) * 2)
    b = [float(np.float32(v) * sc) for v in box]
    bl, br = [float(np.float32(v) * sc) for v in border]
    assert min(b) >= 0 and bl >= 0 and br >= 0, "domain: non-negative box and border coordinates (module docstring)"
    wstep = max(int((br - bl) / 56.0), 1)
    hstep = max(int((b[3] - b[1]) / 56.0), 1)
    r0, r1 = int((b[1] + b[3]) / 2.0 + 0.5), int(b[3] - (b[3] - b[1]) * 0.1 + 0.5)
    c0, c1 = int(bl + 0.5), int(br + 0.5)
    return min(r0, H2), min(r1, H2), hstep, min(c0, W2), min(c1, W2), wstep


def box_geometry_f64(pose):
    """Box3d (box_3d.py:12-60) in float64 on the float32 pose: T, R, Po, Pc, planes (6, 4), nearest vertex and the gap between
    the nearest and the second nearest vertex distance (a float32 evaluation may pick another vertex only if that gap is tiny)."""
    p = [float(np.float32(v)) for v in pose]
    T = np.array(p[0:3])
    sx, sy, sz, th = p[3], p[4], p[5], p[6]
    c, s = math.cos(th), math.sin(th)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    hx, hz = sx / 2, sz / 2
    Po = np.array([[-hx, 0, -hz], [-hx, 0, hz], [hx, 0, hz], [hx, 0, -hz],
                   [-hx, -sy, -hz], [-hx, -sy, hz], [hx, -sy, hz], [hx, -sy, -hz]])
    Pc = Po @ R.T + T
    planes = []
    for a, b_, c_ in PLANE_TRI:
        n = np.cross(Pc[b_] - Pc[a], Pc[c_] - Pc[a])
        planes.append([n[0], n[1], n[2], -float(n @ Pc[a])])
    d = np.sqrt((Pc ** 2).sum(1))
    nearest = int(np.argmin(d))                         # first minimum == strict '<' scan
    gap = float(np.sort(d)[1] - np.sort(d)[0])
    return T, R, Po, Pc, np.array(planes), nearest, gap


def lattice_f64(calib, scale, H2, W2, box, border, pose):
    """One object's sample lattice (dense_align.py:13-69, box_3d.py:62-106) in float64.
    Returns a dict: u, v (int64, the WHOLE lattice in row-major order), mask (bool: the ray hits the box), dz (float64: z of
    the hit in camera coordinates minus the box centre's -- the kernel's `ic2`; 0 where mask is false), plane (which of the three
    tested faces was hit, -1 = none), margin (float64: the smallest distance of any object-frame coordinate that was TESTED for
    this pixel to its lo / hi threshold, metres), nr, nc, hstep, wstep, nearest_gap."""
    scale2 = float(scale) * 2
    f, cx, cy = calib.p2[0, 0] * scale2, calib.p2[0, 2] * scale2, calib.p2[1, 2] * scale2
    r0, r1, hstep, c0, c1, wstep = lattice_slices(scale, H2, W2, box, border)
    rows, cols = np.arange(H2)[r0:r1:hstep], np.arange(W2)[c0:c1:wstep]
    nr, nc = len(rows), len(cols)
    T, R, Po, Pc, planes, nearest, gap = box_geometry_f64(pose)
    out = {'nr': nr, 'nc': nc, 'hstep': hstep, 'wstep': wstep, 'nearest_gap': gap, 'r0': r0, 'r1': r1, 'c0': c0, 'c1': c1}
    if nr == 0 or nc == 0:
        z = np.zeros(0)
        out.update(u=z.astype(np.int64), v=z.astype(np.int64), mask=z.astype(bool), dz=z, plane=z.astype(np.int64), margin=z)
        return out
    u = np.tile(cols, nr).astype(np.int64)
    v = np.repeat(rows, nc).astype(np.int64)
    homo = np.stack(((u - cx) / f, (v - cy) / f, np.ones(len(u))), 1)
    lo, hi = Po[4] - DOUBLE_EPS, Po[2] + DOUBLE_EPS
    mask = np.zeros(len(u), bool)
    dz = np.zeros(len(u))
    plane = np.full(len(u), -1, np.int64)
    margin = np.full(len(u), np.inf)
    for i in range(3):
        pl = planes[PLANE_GROUP[nearest][i]]
        with np.errstate(divide='ignore', invalid='ignore'):
            # a ray parallel to the face (v == cy against the top / bottom face: the products are exact zeros in float32 as
            # here) gives t = inf and inf / nan coordinates: every comparison is false, in any precision -- no margin to take
            t = -pl[3] / (homo @ pl[0:3])
            ic = homo * t[:, None] - T
            io = ic @ R                                  # rows of R^T applied: io_k = sum_j R[j][k] ic_j
            inside = ((io >= lo) & (io <= hi)).all(1)
            m = np.minimum(np.abs(io - lo), np.abs(io - hi))
        m = np.where(np.isfinite(m), m, np.inf).min(1)
        todo = ~mask                                     # the first valid plane wins (box_3d.py:79-82)
        margin[todo] = np.minimum(margin[todo], m[todo])
        hit = todo & inside
        dz[hit] = ic[hit, 2]
        plane[hit] = i
        mask |= hit
    out.update(u=u, v=v, mask=mask, dz=dz, plane=plane, margin=margin)
    return out


# ------------------------------------------------------------------ taps and cost
def tap_coords(u, v, H2, W2, dtype=np.float64):
    """`unnorm`: lattice coordinate -> normalised grid -> pixel, as F.grid_sample(align_corners=True) un-normalises it
    (dense_align.py:194-202,219).  dtype=float32 restates the kernel's operations one by one."""
    t = dtype
    hw, hh = t((W2 - 1) / 2.0), t((H2 - 1) / 2.0)
    u, v = np.asarray(u).astype(t), np.asarray(v).astype(t)
    px = (((u - hw) / hw + t(1)) / t(2)) * t(W2 - 1)
    py = (((v - hh) / hh + t(1)) / t(2)) * t(H2 - 1)
    assert px.dtype == t and py.dtype == t
    return px, py


def right_u(u, dz, depth, fb, dtype=np.float64):
    """The right image's column of a lattice pixel under one depth hypothesis (dense_align.py:211-219): u - gdd with
    gdd = 1 / (dz / fb + 1 / (fb / depth)).  dtype=float32 restates `cost_kernel`'s operations one by one."""
    t = dtype
    fb, depth = t(fb), t(depth)
    dis_inv = t(1) / ((t(1) / depth) * fb)
    gdd = t(1) / (np.asarray(dz).astype(t) / fb + dis_inv)
    out = np.asarray(u).astype(t) - gdd
    assert out.dtype == t
    return out


def taps_f64(img, px, py):
    """Border-clamped bilinear taps (F.grid_sample, padding_mode='border'): img (C, H, W), px / py (N) pixel coordinates ->
    (N, C) float64.  A neighbour outside the image has weight 0 after the clamp; it is read at the clamped index."""
    img = np.asarray(img, np.float64)
    C, H, W = img.shape
    ix = np.clip(np.asarray(px, np.float64), 0.0, W - 1.0)
    iy = np.clip(np.asarray(py, np.float64), 0.0, H - 1.0)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    ax, ay = ix - x0, iy - y0
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    out = (img[:, y0, x0] * ((1 - ax) * (1 - ay)) + img[:, y0, x1] * (ax * (1 - ay))
           + img[:, y1, x0] * ((1 - ax) * ay) + img[:, y1, x1] * (ax * ay))
    return out.T


def cost_f64(img_right, left_val, px, py):
    """SAD (L1, dense_align.py:231) over an object's valid pixels for one hypothesis: left_val (N, 3) the left taps, px / py (N)
    where the right image is read."""
    if len(np.asarray(px)) == 0:
        return 0.0
    return float(np.abs(np.asarray(left_val, np.float64) - taps_f64(img_right, px, py)).sum())


def order_bound(count):
    """tests/test_dense_align_gpu.py `_order_bound`, relative to the cost: two float32 evaluations of a sum of 3 * count
    non-negative terms differ by at most 2 gamma_n sum|x|, the terms themselves by a few u each."""
    return (2.0 * 3.0 * np.asarray(count, np.float64) + 16.0) * 2.0 ** -24
