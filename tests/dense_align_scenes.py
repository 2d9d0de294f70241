"""Constructed scenes of the dense-alignment stage tests (tests/test_dense_align_ref_cpu.py validates them on the CPU,
tests/test_dense_align_stages_gpu.py runs them on the device) and the float64 evaluation of a whole scene.

Image: fixture.make_inputs(seed, 60, 200, target_short=96) -> 96 x 320 network input, scale 1.6, upsampled 192 x 640.
Calibration: f = 116 px, cx = 100, cy = 30 (original pixels), P2[0,3] - P3[0,3] = 0.54 f; cars at z = 3..25 m.
Every object is (pose, box, border): the 2-D box and the borders are inputs of their own (not the projection of the pose), which
is what lets a scene put a lattice exactly where an edge case lies.  The constants were found by random search over poses with
dense_align_ref.lattice_f64 ALONE, keeping those that meet the scene conditions (decision margin, unique nearest vertex, the
wanted count); no device result went into them.
"""
import numpy as np

import dense_align_ref as ref

H, W, SCALE, SEED = 96, 320, 1.6, 4
H2, W2 = 2 * H, 2 * W
MARGIN = 1e-3            # metres: no lattice pixel's membership may hinge on less


def calib():
    from oracle import dense_align as oda
    return oda.Calib([116.0, 0, 100.0, 5.0, 0, 116.0, 30.0, 0, 0, 0, 1, 0],
                     [116.0, 0, 100.0, -57.64, 0, 116.0, 30.0, 0, 0, 0, 1, 0])


# name: (pose x y z w h l theta, box x0 y0 x1 y1, border left right); original-image pixels
OBJECTS = {
    # --- lattice totals (valid pixels): 1, 63, 64, 65, 255, 256, 257 and several 256-pixel rounds
    'n1':    ([-10.25, 1.15, 22.5, 1.44, 1.47, 3.61, 2.62], [42.375, 32.5, 52.4375, 33.125], [48.125, 48.4375]),
    'n63':   ([2.92, 0.64, 12.67, 1.55, 1.66, 4.06, -2.4], [109.6875, 23.375, 141.3125, 30.875], [124.6875, 126.9375]),   # borders narrower than the box
    'n64':   ([-10.25, 1.15, 22.5, 1.44, 1.47, 3.61, 2.62], [42.375, 28.875, 52.4375, 35.4375], [47.125, 49.75]),
    'n65':   ([2.47, 1.08, 23.43, 1.73, 1.49, 4.0, -0.68], [102.5625, 29.25, 122.75, 33.125], [108.8125, 112.75]),
    'n255':  ([-8.34, 0.97, 23.17, 1.41, 1.52, 3.52, 1.57], [47.875, 28.0, 68.0, 32.3125], [50.0, 65.8125]),
    'n256':  ([9.14, 0.95, 21.13, 1.72, 1.43, 3.86, 0.14], [142.875, 27.9375, 159.0625, 34.375], [142.9375, 153.0]),       # 8 misses, second-plane hits
    'n257':  ([-1.88, 0.81, 5.8, 1.54, 1.52, 3.82, -0.55], [41.625, 42.5625, 94.3125, 46.5], [37.4375, 91.9375]),         # 33 misses below an oblique edge, wstep 3
    'big':   ([-1.06, 1.18, 6.56, 1.69, 1.63, 4.0, 2.42], [53.375, 25.8125, 118.5, 58.5625], [57.1875, 108.875]),         # 3243 of 3486: 14 rounds, yaw, two planes, wstep 2
    # --- edges
    'left':  ([-1.59, 0.76, 3.6, 1.6, 1.59, 4.4, -0.12], [0.0, 17.0, 50.8125, 54.75], [0.0, 29.9375]),                    # z ~ 3 m at column 0: right taps clamp at x = 0
    'right': ([3.56, 0.83, 6.75, 1.54, 1.41, 3.97, 0.11], [166.0625, 10.0625, 199.0, 49.625], [169.75, 201.0]),           # c1 clamps to W2
    'bottom': ([-0.38, 0.86, 4.29, 1.56, 1.56, 4.22, -0.3], [82.375, 33.9375, 128.3125, 68.375], [81.125, 119.3125]),     # r1 clamps to H2
    'hstep': ([0.75, 1.09, 3.75, 1.73, 1.57, 4.13, 0.48], [78.5, 6.6875, 121.6875, 55.75], [79.875, 104.75]),             # hstep 2
    'nr0':   ([2.47, 1.08, 23.43, 1.73, 1.49, 4.0, -0.68], [102.5625, 31.0, 122.75, 31.0], [108.8125, 112.75]),           # flat box
    'nc0':   ([2.47, 1.08, 23.43, 1.73, 1.49, 4.0, -0.68], [102.5625, 29.25, 122.75, 33.125], [112.75, 108.8125]),        # bl >= br
    'miss':  ([12.0, 1.08, 10.0, 1.73, 1.49, 4.0, 0.8], [40.0, 29.25, 60.0, 40.0], [42.0, 58.0]),                         # the pose is nowhere near its box
}

SCENES = {
    'totals': ['n1', 'n63', 'n64', 'n65', 'n255', 'n256', 'n257', 'big'],
    # the 'n64' row between 'right' and 'bottom' is switched off by the valid mask on the device (MASKED)
    'edges': ['left', 'nr0', 'right', 'n64', 'bottom', 'nc0', 'hstep', 'miss', 'n63'],
    'overflow': ['n255', 'n257', 'n65'],
    'allmiss': ['miss', 'nr0'],
}
MASKED = {'edges': [3]}
SMALL = ['n1', 'n63', 'nr0', 'n64', 'n65', 'miss', 'n255']      # the many-object batches cycle through these


def many(R):
    return [SMALL[i % len(SMALL)] for i in range(R)]


def arrays(names):
    """float32 (poses (R,7), boxes (R,4), keypoints (R,5)) of a list of object names."""
    poses = np.array([OBJECTS[n][0] for n in names], np.float32)
    boxes = np.array([OBJECTS[n][1] for n in names], np.float32)
    kp = np.zeros((len(names), 5), np.float32)
    kp[:, 3:5] = np.array([OBJECTS[n][2] for n in names], np.float32)
    return poses, boxes, kp


_lattices = {}


def lattice(name):
    """The reference lattice of one object (computed once, shared, never modified)."""
    if name not in _lattices:
        pose, box, border = OBJECTS[name]
        L = ref.lattice_f64(calib(), SCALE, H2, W2, np.float32(box), np.float32(border), np.float32(pose))
        for v in L.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _lattices[name] = L
    return _lattices[name]


def fb():
    """f * baseline in upsampled pixels x metres, as srcnn_dense_align / dense_align.py:259-260 form it (doubles)."""
    c = calib()
    scale2 = SCALE * 2
    f = c.p2[0, 0] * scale2
    return f * ((c.p2[0, 3] - c.p3[0, 3]) * scale2 / f)


def costs_f64(up_right, left_val, u, v, dz, depths, coord_dtype=np.float64):
    """One object's cost under every hypothesis of `depths`: SAD in float64 of left_val (N, 3) against the right image's taps.
    coord_dtype=float32 forms the tap COORDINATE with the kernel's float32 operations (the coordinate is then an input of the
    taps and the sum, which is what the summation-order bound is about); float64 forms it in float64."""
    px0, py = ref.tap_coords(u, v, H2, W2, coord_dtype)
    hw = coord_dtype((W2 - 1) / 2.0)
    out = []
    for d in depths:
        ur = ref.right_u(u, dz, d, fb(), coord_dtype)
        px = (((ur - hw) / hw + coord_dtype(1)) / coord_dtype(2)) * coord_dtype(W2 - 1)
        out.append(ref.cost_f64(up_right, left_val, px, py))
    return np.array(out)


def first_argmin(c):
    return int(np.argmin(np.asarray(c)))


def near_tie(costs, count):
    """None, or a description of why the first minimum of `costs` is a near-tie by the summation-order bound: some other
    hypothesis lies within the bound of it without being EXACTLY equal and later (equal hypotheses -- those clamped to 1.5 m, or
    whose every right tap clamps at column 0 -- are deliberate: there the first minimum is the rule)."""
    c = np.asarray(costs, np.float64)
    a = first_argmin(c)
    bound = float(ref.order_bound(count)) * c[a]
    for j in range(len(c)):
        if j != a and c[j] - c[a] <= 2 * bound and not (c[j] == c[a] and j > a):
            return "hypothesis %d (%.9g) against the minimum %d (%.9g), bound %.3g" % (j, c[j], a, c[a], bound)
    return None
