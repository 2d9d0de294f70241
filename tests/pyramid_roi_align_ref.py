"""References behind the direct tests of the fused pyramid ROIAlign forward, `srcnn_pyramid_roi_align` (numpy / torch on the CPU;
nothing here imports the product package).  tests/test_pyramid_roi_align_ref_cpu.py pins everything below before a GPU sees it.

* `exact_reference`: the expected float32 output, bit for bit.  Built from the pieces that are pinned against the reference's
  own kernel: `oracle.ops.roi_align_avg` per level, scale = map_height / im_height as a Python double narrowed to float32 (what
  srcnn_pyramid_roi_align does), and an EXPLICIT level per roi, so that a caller can ask for "this roi at level l".
* `float64_reference`: an independent float64 evaluation (`roi_align_backward_ref.roi_align_torch64`: float32 lattice
  coordinates, exact float64 blend; then a float64 2x2 / stride-1 mean) with a derived per-element bound (`BOUND_C`).
* level routing: the window `TIE_WINDOW` inside which a correct float32 evaluation may land on either side of a rounding
  boundary, a deterministic search that plants float32 rois inside it, and `device_level_set`, the levels a correct float32
  evaluation can return for a roi.
* `build_case` / `TABLE`: the rois, maps and kernel configurations of tests/test_pyramid_roi_align_gpu.py.

Channels are independent in ROIAlign (every channel of the oracle and of the kernels goes through the same arithmetic on its own
values), so the references are computed once on CMAX channels and a test with C channels reads the first C of them.
"""
import functools
import math

import numpy as np
import torch

import roi_align_backward_ref as RB
import small_kernels_ref as SK

F = np.float32
U = 2.0 ** -24                      # unit roundoff of float32
F32, SPLIT16 = 0, 1                 # SRCNN_FMT_*

IM_H, IM_W = 400, 640               # the smallest image on which all four levels occur (thresholds 50 / 136 / 369 image pixels)
MAP_HW = [(100, 160), (50, 80), (25, 40), (13, 20)]      # 13, not 400 / 32: the scale rule is map_height / im_height
BATCH = 2
CMAX = 512

# ---------------------------------------------------------------------------------------------------------------- level routing
# pyramid_level (csrc/roi_align_geom.h) evaluates  lv = logf(sqrtf(bh * bw) / 224) + 4  in float32, bh = y2 - y1 + 1,
# bw = x2 - x1 + 1, and rounds it half away from zero.  TIE_WINDOW bounds |lv_float32 - lv_exact| for any correct float32
# evaluation, in units of u = 2^-24 (every float32 operation is within u relative of its exact result; sqrtf, the division and
# logf are given a full ulp = 2u, which is what ROCm documents for logf and more than the correctly rounded sqrtf and division
# need):
#   bh, bw        two operations each (the difference, + 1): the first error is scaled by d / (d + 1) < 1, so <= 2u each;
#   bh * bw       the product of the two plus its own rounding:                      2u + 2u + u  = 5u     (relative)
#   sqrtf         halves the relative error of its argument, adds one ulp:           2.5u + 2u    = 4.5u
#   / 224         one ulp:                                                           4.5u + 2u    = 6.5u
#   logf          a relative error e of the argument is an ABSOLUTE error e of the logarithm: 6.5u; the routing boundaries lie
#                 at log values -1.5, -0.5 and 0.5, all below 2 in magnitude, where one ulp is at most 2^-23 = 2u:   8.5u
#   + 4           the results 2.5, 3.5, 4.5 are below 8, where half an ulp is at most 2^-22 = 4u:                    12.5u
# (the float64 evaluation the margin comes from is exact to 1e-15 on this scale).  12.5 u = 7.5e-7, below 1e-5.
TIE_WINDOW = 12.5 * U
assert TIE_WINDOW < 1e-5
BOUNDARIES = (2, 3, 4)              # lv = k + 0.5 <=> sqrt(h w) = 224 e^(k - 3.5); levels k - 2 (below) and k - 1 (above), 0 = P2
RANDOM_MARGIN = 1e-3                # every random roi is at least this far from a boundary
NEAR_MARGIN = (1e-4, 1e-3)          # "near but decided"


def boundary_area(k):
    return (224.0 * math.exp(k - 3.5)) ** 2


def _half_away_level(lv):
    """float32 lv -> level 0..3 the way pyramid_level finishes (NaN -> 0: fmaxf(NaN, 2) = 2)."""
    if np.isnan(lv) or np.isinf(lv):
        return 0 if not lv > 0 else 3
    r = math.copysign(math.floor(abs(float(lv)) + 0.5), float(lv))      # (|lv| + 0.5 is exact in float32 for |lv| < 8 near k + 0.5)
    return int(min(max(r, 2.0), 5.0)) - 2


def device_lv_interval(roi):
    """(lowest, highest) un-rounded float32 level a CORRECT float32 evaluation of pyramid_level can produce for one float32 roi:
    the subtraction, the additions, the product, sqrtf and the division are correctly rounded (IEEE; the library is built
    without contraction and with the compiler's default correctly rounded float32 sqrt / divide), so numpy float32 reproduces
    them exactly; logf may return any float32 within one ulp of the exact logarithm of its float32 argument (ROCm's documented
    accuracy), and the final + 4 is monotone in it.  (nan, nan) for a negative area, (-inf, -inf) for a zero one."""
    r = np.asarray(roi, F)
    with np.errstate(invalid='ignore'):
        bh = F(F(r[4] - r[2]) + F(1))
        bw = F(F(r[3] - r[1]) + F(1))
        q = F(np.sqrt(F(bh * bw)) / F(224))
    if np.isnan(q):
        return F(np.nan), F(np.nan)
    if q == 0:
        return F(-np.inf), F(-np.inf)
    y = math.log(float(q))
    e = float(np.spacing(F(abs(y))))
    lo = np.nextafter(F(y - e), F(-np.inf))                          # outward: never narrower than the admissible interval
    hi = np.nextafter(F(y + e), F(np.inf))
    return F(lo + F(4)), F(hi + F(4))


def device_level_set(roi):
    """The levels a correct float32 evaluation can return (device_lv_interval, then the monotone half-away rounding and the
    clamp).  A roi whose interval is the single point k + 0.5 is a tie in float32 itself: half away from zero sends it UP; half
    to even (rintf) would send 2.5 and 4.5 down."""
    lo, hi = device_lv_interval(roi)
    return set(range(_half_away_level(lo), _half_away_level(hi) + 1))


def plant_ties(k, b, x1, y1, h0, count=2, span=4096):
    """Deterministic search for float32 rois [b, x1, y1, x2, y2] whose float64 level lies within TIE_WINDOW of k + 0.5: walk y2
    over `span` consecutive float32 values from y1 + h0 - 1; for each, the x2 that makes the area (y2 - y1 + 1)(x2 - x1 + 1)
    hit 224^2 e^(2k - 7), rounded to float32, and its two float32 neighbours.  (Integer coordinates do not get close enough:
    the area must be right to a few 1e-7 relative.)  Returns the `count` closest, at most one per y2; for k = 4 the candidates
    whose un-rounded float32 level is exactly 4.5 for every admissible evaluation (device_lv_interval) come
    first."""
    y2 = F(y1 + h0 - 1)
    ys = (y2 + np.arange(span, dtype=np.float64) * float(np.spacing(y2))).astype(F)
    h = ys.astype(np.float64) - float(F(y1)) + 1.0
    x2 = (float(F(x1)) + boundary_area(k) / h - 1.0).astype(F)
    cands = []
    for x in (np.nextafter(x2, F(-np.inf)), x2, np.nextafter(x2, F(np.inf))):
        rois = np.stack([np.full(span, b, F), np.full(span, x1, F), np.full(span, y1, F), x, ys], 1).astype(F)
        cands.append((RB.pyramid_levels(rois)[1], rois))
    m = np.stack([c[0] for c in cands])                             # (3, span)
    pick = m.argmin(0)
    best = m.min(0)
    rois = np.stack([cands[pick[j]][1][j] for j in range(span)])
    order = np.argsort(best, kind='stable')
    if k == 4:
        sure = [j for j in order[:64] if best[j] < TIE_WINDOW and device_lv_interval(rois[j]) == (F(4.5), F(4.5))]
        order = np.array(sure + [j for j in order if j not in set(sure)])
    return rois[order[:count]]


def near_boundary(k, b, side, x1, y1, h0, target=4e-4):
    """A roi whose level is `target` (inside NEAR_MARGIN) below (side = -1) or above (+1) k + 0.5: decided for every
    implementation (the margin is more than a hundred TIE_WINDOWs), but only just."""
    h = float(F(y1 + h0 - 1)) - float(F(y1)) + 1.0
    w = boundary_area(k) * math.exp(2.0 * side * target) / h
    return np.array([b, x1, y1, F(x1 + w - 1.0), F(y1 + h0 - 1)], F)


# ---------------------------------------------------------------------------------------------------------------- the case
def _random_rois(g, per_level):
    """`per_level` rois of every level on alternating batch images, each at least RANDOM_MARGIN from a rounding boundary
    (re-drawn otherwise), fractional coordinates, inside the image."""
    edges = [8.0] + [math.sqrt(boundary_area(k)) for k in BOUNDARIES] + [480.0]
    out = []
    for l in range(4):
        got = 0
        while got < per_level:
            s = math.exp(g.uniform(math.log(edges[l] * 1.01), math.log(edges[l + 1] * 0.99)))
            lo, hi = max(0.4, (s / (IM_H - 1.0)) ** 2 * 1.02), min(2.5, ((IM_W - 1.0) / s) ** 2 * 0.98)
            ar = g.uniform(lo, hi)
            h, w = s / math.sqrt(ar), s * math.sqrt(ar)
            x1, y1 = g.uniform(0, IM_W - w), g.uniform(0, IM_H - h)
            roi = np.array([got % BATCH, x1, y1, x1 + w - 1.0, y1 + h - 1.0], F)
            lv, m = RB.pyramid_levels(roi[None])
            if m[0] < RANDOM_MARGIN or lv[0] != l:
                continue
            out.append(roi)
            got += 1
    return out


@functools.lru_cache(maxsize=None)
def build_case(seed=20):
    """The rois and maps of the GPU tests.  Returns a dict:
      maps    four (BATCH, h, w, CMAX) float32 NHWC maps (standard normal);
      rois    (n, 5) float32;  kind (n,) of 'random' | 'tie' | 'near' | 'edge';  name (n,) a word per roi;
      level   (n,) the expected level 0..3: the float64 level (of a tie too), and P2 for the roi of negative area;
      alt     (n,) the other admissible level of a tie, -1 elsewhere;  tie_k (n,) the boundary of a tie, 0 elsewhere;
      margin  (n,) float64 distance of the un-rounded level from the nearest k + 0.5;
      decided (n,) bool: every implementation, the oracle's torch float32 routing included, must agree on the level.
    Everything is read-only and shared."""
    g = np.random.default_rng(seed)
    rois, kind, name = [], [], []

    def add(r, k, nm):
        rois.append(np.asarray(r, F)); kind.append(k); name.append(nm)

    for r in _random_rois(g, 12):
        add(r, 'random', 'random')
    # planted ties and near-boundary rois: (k, image, x1, y1, height) -- widths follow from the boundary's area
    spots = {2: [(0, 8.25, 16.5, 40.0), (1, 301.5, 120.75, 61.0)],
             3: [(0, 20.5, 40.25, 110.0), (1, 250.125, 200.5, 150.0)],
             4: [(0, 12.5, 10.25, 301.0), (1, 90.75, 30.5, 340.0)]}
    for k in BOUNDARIES:
        for b, x1, y1, h0 in spots[k]:
            add(plant_ties(k, b, x1, y1, h0, count=1)[0], 'tie', 'tie%d' % k)
    for k in BOUNDARIES:
        for side, (b, x1, y1, h0) in zip((-1, 1), spots[k]):
            add(near_boundary(k, 1 - b, side, x1 + 3.0, y1 + 2.0, h0 * 0.9), 'near', 'near%d%s' % (k, '-+'[side > 0]))
            add(near_boundary(k, b, -side, x1 + 1.5, y1 + 5.0, h0 * 1.05, target=1.5e-4), 'near', 'near%d%s' % (k, '-+'[side < 0]))
    add([1, 0, 0, 0, 0], 'edge', 'zero')                                 # the all-zero padded proposal
    add([0, 200, 100, 150, 180], 'edge', 'negative-area')               # x2 < x1: the width clamps to 0; the area is negative
    add([1, 200, 180, 150, 100], 'edge', 'reversed')                    # x2 < x1 and y2 < y1: both clamp, the area is positive
    add([0, 37, 21, 37, 21], 'edge', 'one-pixel')
    add([1, 600.5, 350.25, 700, 450], 'edge', 'right-bottom')           # partly outside on the right and at the bottom
    add([1, -30.5, -20.25, 60, 45], 'edge', 'negative-start')           # partly outside, negative start
    add([0, 700, 450, 800, 520], 'edge', 'outside')                     # wholly outside: exactly 0
    # level 2 (25 x 40, scale 1 / 16 exactly): start_h = 11, roi_h = 24 - 11 + 1 = 14, bin_h = 2 (A = 7) or 1 (A = 14): the last
    # lattice row is 11 + 14 = 25 == height exactly and must be dropped, the one before it is inside
    add([0, 100, 176, 299, 384], 'edge', 'last-row-on-height')
    rois = np.stack(rois)
    kind, name = np.array(kind), np.array(name)
    with np.errstate(invalid='ignore'):
        level, margin = RB.pyramid_levels(rois)
    level = level.copy()
    level[name == 'negative-area'] = 0      # sqrt of a negative area: lv is NaN, and fminf(fmaxf(NaN, 2), 5) = 2, P2.  (The
    margin[name == 'negative-area'] = 1.0   # reference drops such a roi from every level; its proposals never have x2 < x1.)
    tie_k = np.array([int(nm[3:]) if kd == 'tie' else 0 for nm, kd in zip(name, kind)])
    alt = np.where(kind == 'tie', 2 * tie_k - 3 - level, -1)            # the other one of (k - 2, k - 1)
    decided = (kind != 'tie') & (name != 'negative-area')
    maps = [g.standard_normal((BATCH, h, w, CMAX)).astype(F) for h, w in MAP_HW]
    for a in maps + [rois, level, margin, alt, tie_k, decided]:
        a.setflags(write=False)
    return dict(maps=maps, rois=rois, kind=kind, name=name, level=level, alt=alt, tie_k=tie_k, margin=margin, decided=decided)


@functools.lru_cache(maxsize=None)
def map_bytes(fmt):
    """What is uploaded: the float32 maps themselves, or their SPLIT16 bytes (small_kernels_ref.split16_pack) typed as float32.
    The bytes are the split OF THE VALUE THEY HOLD (packed once more after unpacking: where lo came out as exactly half a step
    of hi, the first split is not the canonical one of hi + lo), so that pack(unpack(bytes)) == bytes."""
    maps = build_case()['maps']
    out = maps if fmt == F32 else [SK.split16_pack(SK.split16_unpack(SK.split16_pack(m))) for m in maps]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def map_values(fmt):
    """The values the kernel sees: float32(hi) + float32(lo) of the SPLIT16 bytes (split16_unpack), or the float32 maps."""
    out = map_bytes(fmt) if fmt == F32 else [SK.split16_unpack(m) for m in map_bytes(fmt)]
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- exact
def level_scale(l, im_height=IM_H, map_hw=MAP_HW):
    """srcnn_pyramid_roi_align: (float)((double)map_height / (double)im_height)"""
    return float(F(map_hw[l][0] / float(im_height)))


def exact_reference(maps, rois, A, im_height, levels):
    """maps: four (B, h, w, C) float32 NHWC (the values the kernel sees), rois (n, 5), levels (n,) in 0..3 -> (n, A, A, C) float32:
    oracle.ops.roi_align_avg of every roi on the map of ITS level at that level's scale."""
    from oracle import ops as oops
    rois = np.asarray(rois, F)
    levels = np.asarray(levels)
    out = np.zeros((rois.shape[0], A, A, maps[0].shape[3]), F)
    for l in range(4):
        idx = np.nonzero(levels == l)[0]
        if idx.size == 0:
            continue
        feat = np.ascontiguousarray(np.asarray(maps[l], F).transpose(0, 3, 1, 2))
        scale = maps[l].shape[1] / float(im_height)                    # a Python double; the oracle narrows it to float32
        out[idx] = oops.roi_align_avg(feat, rois[idx], A, A, scale).transpose(0, 2, 3, 1)
    return out


@functools.lru_cache(maxsize=None)
def expected(mfmt, A, alt=False):
    """Exact reference of the whole case on CMAX channels at the expected levels; alt=True: the planted ties (in case order) at
    their OTHER admissible level."""
    c = build_case()
    if alt:
        t = c['kind'] == 'tie'
        out = exact_reference(map_values(mfmt), c['rois'][t], A, IM_H, c['alt'][t])
    else:
        out = exact_reference(map_values(mfmt), c['rois'], A, IM_H, c['level'])
    out.setflags(write=False)
    return out


def as_bits(x, ofmt):
    """float32 (..., C) -> what the output buffer must hold, as int32: the float32 bits, or the SPLIT16 bytes."""
    x = np.ascontiguousarray(x, F)
    return (x if ofmt == F32 else SK.split16_pack(x)).view(np.int32)


def split16_unpack64(raw):
    """int32- or float32-typed SPLIT16 bytes (..., C) -> hi + lo in float64 (exact; small_kernels_ref.split16_unpack adds in
    float32, which can round)."""
    raw = np.ascontiguousarray(raw)
    C = raw.shape[-1]
    h = raw.reshape(-1, C // 8, 8).view(np.float16).reshape(-1, C // 8, 2, 8).astype(np.float64)
    return (h[:, :, 0, :] + h[:, :, 1, :]).reshape(raw.shape)


# ---------------------------------------------------------------------------------------------------------------- float64
# The derived bound.  One output element is 0.25 x the float32 sum of four lattice points; a lattice point is
#     v = (float)( ul hr1 wr1 + ur hr1 wr + (double)dl_h wr1 + (double)dr_hw ),   dl_h = dl * h_ratio,  dr_hw = dr * h_ratio * w_ratio
# with dl_h and dr_hw formed in float32 and everything else in double (csrc/roi_align.hip, lattice_point8).  The float64
# reference uses the same float32 coordinates and hence the same weights exactly (h - hstart is exact in float32), so the two
# differ only by the kernel's roundings.  Count them along the worst path from a tap value to the output:
#     dr_hw: two float32 products (dl_h: one)                        2
#     the narrowing of the double blend to float32                   1
#     s = top_prev; s += top; s += bot_prev; s += bot                3   (the first operand passes through all three additions)
#     x 0.25                                                         0   (exact: a power of two, no underflow at these magnitudes)
# That is 6 roundings of relative size u on every |weight x value| term; one spare unit covers the double-precision operations
# (~2^-53 each) and the second-order products: |kernel - float64| <= gamma_7 x S, S = 0.25 sum over the 4 lattice points and
# their 4 taps of |weight x value| -- and likewise for the exact reference, which has the same operations.  A SPLIT16 output
# adds the format's own step at the value (small_kernels_ref.split16_step).
BOUND_C = 7


def lattice64(values, roi, a, scale, absolute=False):
    """One roi on one (B, h, w, C) map -> (a, a, C) float64 lattice in the float32 coordinates of the kernels
    (roi_align_backward_ref.roi_geometry / lattice_axis).  absolute=True: sum of |weight| |value| instead of weight x value (a
    weight is negative where the first tap is clamped to size - 2 and the ratio exceeds 1)."""
    B, H, W, C = values.shape
    b, sw, sh, bw, bh, _, _ = RB.roi_geometry(roi, scale, a, a)
    rows = [RB.lattice_axis(i, bh, sh, 0.0, H)[:3] for i in range(a)]
    cols = [RB.lattice_axis(i, bw, sw, 0.0, W)[:3] for i in range(a)]
    ok = np.array([r[0] for r in rows])[:, None] & np.array([c[0] for c in cols])[None, :]
    hs, ws = np.array([r[1] for r in rows]), np.array([c[1] for c in cols])
    hr = np.array([float(r[2]) for r in rows])[:, None, None]
    wr = np.array([float(c[2]) for c in cols])[None, :, None]
    wy, wx = (1.0 - hr, hr), (1.0 - wr, wr)
    out = np.zeros((a, a, C), np.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            v = values[b][(hs + dy)[:, None], (ws + dx)[None, :]].astype(np.float64)
            out += np.abs(wy[dy] * wx[dx]) * np.abs(v) if absolute else wy[dy] * wx[dx] * v
    return out * ok[:, :, None]


def _mean2x2(x):
    """(..., a, a, C) float64 -> (..., a - 1, a - 1, C): 2x2 / stride-1 mean"""
    return 0.25 * (x[..., :-1, :-1, :] + x[..., :-1, 1:, :] + x[..., 1:, :-1, :] + x[..., 1:, 1:, :])


def float64_reference(maps, rois, A, im_height, levels, chunk=2):
    """-> (value (n, A, A, C) float64, bound (n, A, A, C) float64): roi_align_torch64 per level (rois of one image at a time,
    `chunk` at a time: it copies the whole map per roi) followed by the float64 2x2 mean; bound = gamma_BOUND_C x S."""
    rois = np.asarray(rois, F)
    n, C = rois.shape[0], maps[0].shape[3]
    val = np.zeros((n, A, A, C), np.float64)
    mag = np.zeros((n, A, A, C), np.float64)
    for l in range(4):
        scale = level_scale(l, im_height, [m.shape[1:3] for m in maps])
        for b in range(maps[l].shape[0]):
            idx = np.nonzero((np.asarray(levels) == l) & (rois[:, 0] == b))[0]
            if idx.size == 0:
                continue
            feat = torch.from_numpy(np.ascontiguousarray(maps[l][b:b + 1].transpose(0, 3, 1, 2))).double()
            for s in range(0, idx.size, chunk):
                sel = idx[s:s + chunk]
                r = rois[sel].copy()
                r[:, 0] = 0
                lat = RB.roi_align_torch64(feat, r, A + 1, A + 1, scale).numpy()            # (k, C, a, a)
                val[sel] = _mean2x2(lat.transpose(0, 2, 3, 1))
        for i in np.nonzero(np.asarray(levels) == l)[0]:
            mag[i] = _mean2x2(lattice64(maps[l], rois[i], A + 1, scale, absolute=True))
    return val, float(RB.gamma(BOUND_C)) * mag


@functools.lru_cache(maxsize=None)
def expected64(mfmt, A, alt=False):
    """float64_reference of the whole case on CMAX channels (alt=True: the planted ties at their other admissible level)."""
    c = build_case()
    if alt:
        t = c['kind'] == 'tie'
        out = float64_reference(map_values(mfmt), c['rois'][t], A, IM_H, c['alt'][t])
    else:
        out = float64_reference(map_values(mfmt), c['rois'], A, IM_H, c['level'])
    for a in out:
        a.setflags(write=False)
    return out


def within_bound(got_bits, ofmt, ref, bound):
    """got_bits (..., C) int32 output bits; ref, bound float64 of the same shape -> (ok per element, error, allowed)."""
    if ofmt == F32:
        got = np.ascontiguousarray(got_bits).view(F).astype(np.float64)
        allowed = bound
    else:
        got = split16_unpack64(got_bits)
        allowed = bound + SK.split16_step(np.abs(ref) + bound)
    err = np.abs(got - ref)
    return err <= allowed, err, allowed


# ---------------------------------------------------------------------------------------------------------------- the table
# Which kernel a call reaches, read off the dispatch in srcnn_pyramid_roi_align: the roi form (pyramid_roi_align8_roi_kernel) when
# cstride and coffset are multiples of 8 and C <= 256; else the row-pair form (pyramid_roi_align8_kernel) when they are
# multiples of 8; else the per-channel kernel (pyramid_roi_align_kernel).  SRCNN_ROI_ALIGN_FORM=0 (read once per process) sends
# the first group to the row-pair form too, in blocks of 64 / (C / 8) output rows.
def _table():
    t = []

    def add(form, C, A, mfmt, ofmt, cstride, coffset):
        t.append(dict(form=form, C=C, A=A, mfmt=mfmt, ofmt=ofmt, cstride=cstride, coffset=coffset,
                      id='%s-C%d-A%d-%s-%s-%d+%d' % (form, C, A, 'fs'[mfmt], 'fs'[ofmt], cstride, coffset)))

    add('roi', 256, 14, SPLIT16, SPLIT16, 256, 0)                       # the shipped keypoint head
    for A in (7, 14):
        add('roi', 256, A, F32, F32, 512, 256)
        for C in (64, 192):
            add('roi', C, A, SPLIT16, F32, C, 0)                        # idle upper channel groups
        for C in (320, 512):
            for mfmt in (F32, SPLIT16):
                for ofmt in (F32, SPLIT16):
                    add('rowpair', C, A, mfmt, ofmt, C, 0)
        for C in (64, 256):
            for mfmt in (SPLIT16, F32):
                add('perchannel', C, A, mfmt, F32, 2 * C + 4, C + 4)
    return t


TABLE = _table()
BOX_HEAD = dict(form='roi', C=256, A=7, mfmt=SPLIT16, ofmt=SPLIT16, cstride=512, coffsets=(0, 256))   # two calls, one buffer
FORM0 = [dict(form='rowpair', C=C, A=A, mfmt=f, ofmt=f, cstride=C, coffset=0, id='form0-C%d-A%d-%s' % (C, A, 'fs'[f]))
         for C in (64, 128, 256) for A in (7, 14) for f in (F32, SPLIT16)]       # the child process with SRCNN_ROI_ALIGN_FORM=0
