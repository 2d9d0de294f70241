"""Pure numpy / Python-integer restatement of the result visualisation (include/srcnn_hip.h, "result visualisation"), written
against that specification: segment construction from a detection record, the rasterisation rule as an explicit per-segment
PIXEL WALK (the kernel uses the closed-form membership test `covers`, restated here as well, so the two forms check each other),
the lidar plane and the panel layout.  Python integers do not overflow, so the 64-bit path of the kernel is checked against exact
arithmetic.

`Trace.pretrunc` collects every float64 value that is truncated to an integer on the way (projected corners, bird's-eye
coordinates, lidar cells): the device's sin / cos / division may differ from numpy's in the last bit, so a GPU test asserts
`min_integer_margin(trace) >= 1e-6` on its inputs before it compares pictures exactly."""
import math

import numpy as np

REC_COLS = 32
LIMIT = float(2 ** 30)
RED, GREEN = (204, 0, 0), (0, 200, 0)
BOXES, WIREFRAMES, BEV_BOXES = 1, 2, 4
WIRE_EDGES = ((0, 1), (1, 2), (2, 3), (0, 3), (4, 5), (5, 6), (6, 7), (7, 4), (4, 0), (5, 1), (6, 2), (7, 3))
BEV_EDGES = ((0, 1), (1, 2), (2, 3), (0, 3), (1, 4), (2, 4))


def bev_geometry(H):
    """(res, x_max, y_max, x_off, y_off) for width = 2 H, float64 as the reference computes them."""
    width = 2 * int(H)
    res = 70.0 / width
    return res, int(40 / res), int(70 / res), int(math.floor(-20 / res)), int(math.floor(70 / res)) - 1


class Trace(object):
    def __init__(self):
        self.pretrunc = []          # float64 values about to be truncated
        self.segments = {'left': [], 'right': [], 'bev': []}        # (p0, p1, thickness, rgb) in draw order


def min_integer_margin(trace):
    """Smallest distance of a traced pre-truncation value (inside the clamp) from an integer at which its truncation changes;
    inf if there is none.  Truncation is toward zero, so every value in (-1, 1) gives 0 and zero itself is no such boundary: a
    value there is measured against -1 and 1 (a corner at z = 1e-9 has the bird's-eye coordinate -z / res = -6e-10)."""
    best = float('inf')
    for v in trace.pretrunc:
        if not math.isfinite(v) or abs(v) >= LIMIT:
            continue
        best = min(best, 1.0 - abs(v) if abs(v) < 1.0 else abs(v - round(v)))
    return best


def clamp_trunc(v, trace=None):
    v = float(v)
    if trace is not None:
        trace.pretrunc.append(v)
    if not v > -LIMIT:          # NaN too
        v = -LIMIT
    if not v < LIMIT:
        v = LIMIT
    return int(v)               # toward zero


# --------------------------------------------------------------------------- the rasterisation rule, two forms
def _sign(v):
    return (v > 0) - (v < 0)


def walk_segment(p0, p1, t, width, height):
    """Every pixel of the stamped segment inside [0, width) x [0, height), by walking i = 0..a along the major axis (the range
    of i is first cut to the steps whose stamp can reach the canvas: a far end point may lie 2^30 pixels away)."""
    (x0, y0), (x1, y1) = (int(p0[0]), int(p0[1])), (int(p1[0]), int(p1[1]))
    adx, ady, sx, sy = abs(x1 - x0), abs(y1 - y0), _sign(x1 - x0), _sign(y1 - y0)
    lo, hi = -(t // 2), (t - 1) // 2
    x_major = adx >= ady
    a, b = (adx, ady) if x_major else (ady, adx)
    m0, sm, size = (x0, sx, width) if x_major else (y0, sy, height)
    # steps i with -hi <= m0 + sm i <= size - 1 - lo
    i_lo, i_hi = 0, a
    if sm > 0:
        i_lo, i_hi = max(i_lo, -hi - m0), min(i_hi, size - 1 - lo - m0)
    elif sm < 0:
        i_lo, i_hi = max(i_lo, m0 - (size - 1 - lo)), min(i_hi, m0 + hi)
    out = set()
    for i in range(i_lo, i_hi + 1):
        step = (2 * i * b + a) // (2 * a) if a else 0
        if x_major:
            x, y = x0 + sx * i, y0 + sy * step
        else:
            x, y = x0 + sx * step, y0 + sy * i
        for dy in range(lo, hi + 1):
            for dx in range(lo, hi + 1):
                if 0 <= x + dx < width and 0 <= y + dy < height:
                    out.add((x + dx, y + dy))
    return out


def covers(p0, p1, t, px, py):
    """The closed-form membership test of the same rule (what a pixel of the gather kernel asks)."""
    (x0, y0), (x1, y1) = (int(p0[0]), int(p0[1])), (int(p1[0]), int(p1[1]))
    dx, dy = x1 - x0, y1 - y0
    lo, hi = -(t // 2), (t - 1) // 2
    if abs(dx) >= abs(dy):
        m0, n0, dm, dn, pm, pn = x0, y0, dx, dy, px, py
    else:
        m0, n0, dm, dn, pm, pn = y0, x0, dy, dx, py, px
    am, an = abs(dm), abs(dn)
    for d in range(lo, hi + 1):
        mi = pm - d
        i = mi - m0 if dm >= 0 else m0 - mi
        if i < 0 or i > am:
            continue
        step = (2 * i * an + am) // (2 * am) if am else 0
        ni = n0 + step if dn >= 0 else n0 - step
        if lo <= pn - ni <= hi:
            return True
    return False


def draw_segment(canvas, p0, p1, t, rgb):
    h, w = canvas.shape[:2]
    for x, y in walk_segment(p0, p1, t, w, h):
        canvas[y, x] = rgb


# --------------------------------------------------------------------------- record -> segments
def corners_3d(pos, dim, theta):
    """The eight box corners, float64, each operation rounded once in this order."""
    w, h, l = float(dim[0]), float(dim[1]), float(dim[2])
    x, y, z = float(pos[0]), float(pos[1]), float(pos[2])
    c, s = math.cos(float(theta)), math.sin(float(theta))
    out = []
    for i in range(8):
        va = -w if i & 3 in (0, 1) else w
        vd = -l if i & 3 in (0, 3) else l
        vb = 0.0 if i < 4 else -h * 2.0
        out.append((x + (c * va + s * vd) / 2.0, y + vb / 2.0, z + (-s * va + c * vd) / 2.0))
    return out, (c, s)


def segments_from_record(rec, p2, vis_thresh, H, layers=7, bev=True):
    rec = np.asarray(rec, np.float32)
    assert rec.ndim == 2 and rec.shape[1] == REC_COLS
    p2 = np.asarray(p2, np.float64).reshape(3, 4)
    n = rec.shape[0] - 1
    res, x_max, y_max, x_off, y_off = bev_geometry(H)
    tr = Trace()
    cf = float(rec[0, 0])
    count = (int(cf) if cf < n else n) if cf > 0 else 0
    thresh = np.float32(vis_thresh)
    for r in range(count):
        row = rec[1 + r]
        if not row[0] > thresh:
            continue
        if r < 100 and layers & BOXES:
            for eye, key in ((0, 'left'), (1, 'right')):
                b = row[1 + 4 * eye: 5 + 4 * eye]
                x1, y1, x2, y2 = [clamp_trunc(np.round(np.float32(v))) for v in b]          # float32 round-half-even
                for p0, p1 in (((x1, y1), (x2, y1)), ((x2, y1), (x2, y2)), ((x2, y2), (x1, y2)), ((x1, y2), (x1, y1))):
                    tr.segments[key].append((p0, p1, 1, RED))
    wire, bevs = [], []
    for r in range(count):
        row = rec[1 + r]
        if not (row[0] > thresh and row[25] > 0):
            continue
        pos, dim, theta = row[27:30].astype(np.float64), row[9:12].astype(np.float64), float(row[30])
        cs, (c, s) = corners_3d(pos, dim, theta)
        if layers & WIREFRAMES and not any(p[2] < 0 for p in cs):
            px = []
            for X, Y, Z in cs:
                u = p2[0, 0] * X + p2[0, 1] * Y + p2[0, 2] * Z
                v = p2[1, 0] * X + p2[1, 1] * Y + p2[1, 2] * Z
                w = p2[2, 0] * X + p2[2, 1] * Y + p2[2, 2] * Z
                with np.errstate(all='ignore'):
                    px.append((clamp_trunc(np.float64(u) / np.float64(w), tr), clamp_trunc(np.float64(v) / np.float64(w), tr)))
            for i, j in WIRE_EDGES:
                wire.append((px[i], px[j], 1, GREEN))
        if layers & BEV_BOXES and bev:
            tip = float(dim[2]) * 2.0 / 3.0
            pts = [(p[0], p[2]) for p in cs[:4]] + [(float(pos[0]) + s * tip, float(pos[2]) + c * tip)]
            bp = [(clamp_trunc(X / res, tr) - x_off, clamp_trunc(-Z / res, tr) + y_off) for X, Z in pts]
            for i, j in BEV_EDGES:
                bevs.append((bp[i], bp[j], 2, GREEN))
    tr.segments['left'] += wire
    tr.segments['bev'] += bevs
    return tr


# --------------------------------------------------------------------------- lidar plane
def lidar_plane(points, velo_to_cam2, H, trace=None):
    """(y_max, x_max) uint8: 255, 100 where a kept point falls."""
    res, x_max, y_max, x_off, y_off = bev_geometry(H)
    m = np.asarray(velo_to_cam2, np.float64)[:3].reshape(3, 4)
    plane = np.full((y_max, x_max), 255, np.uint8)
    for p in np.asarray(points, np.float32).reshape(-1, 4):
        x, y, z = float(p[0]), float(p[1]), float(p[2])
        with np.errstate(invalid='ignore'):              # NaN / inf coordinates: dropped by the filter below
            X = m[0, 0] * x + m[0, 1] * y + m[0, 2] * z + m[0, 3]
            Z = m[2, 0] * x + m[2, 1] * y + m[2, 2] * z + m[2, 3]
        if not (0.0 < Z < 70.0 and -20.0 < X < 20.0):
            continue
        if trace is not None:
            trace.pretrunc += [X / res, -Z / res]
        xi, yi = int(X / res) - x_off, int(-Z / res) + y_off
        xi, yi = min(xi, x_max - 1), min(yi, y_max - 1)
        if xi < 0 or yi < 0:
            continue
        plane[yi, xi] = 100
    return plane


# --------------------------------------------------------------------------- the panel
def render(left, right, rec, p2, vis_thresh=0.7, plane=None, layers=7, bev=True):
    """(panel, trace): the uint8 RGB (2 H, W + x_max, 3) panel and what was drawn."""
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    H, W = left.shape[:2]
    res, x_max, y_max, x_off, y_off = bev_geometry(H)
    if bev and y_max != 2 * H:
        raise ValueError("int(70 / res) is not 2 H")
    tr = segments_from_record(rec, p2, vis_thresh, H, layers, bev)
    l, r = left.copy(), right.copy()
    for key, canvas in (('left', l), ('right', r)):
        for p0, p1, t, rgb in tr.segments[key]:
            draw_segment(canvas, p0, p1, t, rgb)
    panel = np.concatenate((l, r), axis=0)
    if bev:
        b = np.full((y_max, x_max), 255, np.uint8) if plane is None else np.asarray(plane, np.uint8)
        b = np.repeat(b[:, :, None], 3, axis=2)
        for p0, p1, t, rgb in tr.segments['bev']:
            draw_segment(b, p0, p1, t, rgb)
        panel = np.concatenate((panel, b), axis=1)
    return panel, tr
