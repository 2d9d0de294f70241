"""CPU: tests/overlay_ref.py against itself and against hand-drawn pictures -- the rasterisation rule's pixel walk and its
closed-form membership test agree, the bird's-eye geometry keeps y_max == 2 H for the sizes the GPU tests and KITTI use, and
three small pictures are what the rule says by hand.  These tests pin the REFERENCE the GPU tests compare with; apart from
`engine.bev_geometry` they touch no product code and are no coverage of the kernel (tests/test_overlay_gpu.py is)."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_ref as ref           # noqa: E402


@pytest.mark.parametrize('t', [1, 2])
def test_walk_and_membership_agree_on_a_9x9_grid(t):
    """Every segment with both end points in a 9 x 9 grid, seen on an 8 x 8 canvas that cuts the grid's first column and row
    (so stamps and clipping are both exercised)."""
    pts = list(itertools.product(range(-1, 8), range(-1, 8)))
    W = H = 8                                            # canvas [0, 8): grid column/row -1 lies outside
    n = 0
    for p0 in pts:
        for p1 in pts:
            walked = ref.walk_segment(p0, p1, t, W, H)
            member = {(x, y) for y in range(H) for x in range(W) if ref.covers(p0, p1, t, x, y)}
            assert walked == member, (p0, p1, t)
            n += 1
    assert n == 81 * 81


def test_walk_and_membership_agree_far_outside():
    """End points 2^30 away: the walk cuts its range, the membership test is exact in Python integers."""
    far = 2 ** 30
    for p0, p1 in (((3, 4), (far, far // 3)), ((-far, 5), (far, 2)), ((2, -far), (5, far)), ((far, far), (far, far)),
                   ((-far, -far), (far, far - 7))):
        for t in (1, 2):
            walked = ref.walk_segment(p0, p1, t, 16, 12)
            member = {(x, y) for y in range(12) for x in range(16) if ref.covers(p0, p1, t, x, y)}
            assert walked == member, (p0, p1, t)


@pytest.mark.parametrize('H', [8, 20, 375, 600])
def test_bev_height_is_twice_the_image_height(H):
    res, x_max, y_max, x_off, y_off = ref.bev_geometry(H)
    assert y_max == 2 * H                                # the ValueError guard of engine.render_overlay is not hit
    assert x_max in (2 * H * 4 // 7, 2 * H * 4 // 7 - 1) and x_off < 0 <= y_off
    from stereo_rcnn_amd import engine
    assert engine.bev_geometry(H) == (res, x_max, y_max, x_off, y_off)


def _picture(rows):
    return np.array([[c == '#' for c in r] for r in rows])


def _drawn(p0, p1, t):
    c = np.zeros((8, 8, 3), np.uint8)
    ref.draw_segment(c, p0, p1, t, (1, 2, 3))
    assert set(map(tuple, c[c.any(2)])) <= {(1, 2, 3)}
    return c.any(2)


def test_hand_checked_rectangle():
    c = np.zeros((8, 8, 3), np.uint8)
    for p0, p1 in (((1, 2), (6, 2)), ((6, 2), (6, 5)), ((6, 5), (1, 5)), ((1, 5), (1, 2))):
        ref.draw_segment(c, p0, p1, 1, (204, 0, 0))
    assert (c.any(2) == _picture(['........',
                                  '........',
                                  '.######.',
                                  '.#....#.',
                                  '.#....#.',
                                  '.######.',
                                  '........',
                                  '........'])).all()


def test_hand_checked_diagonal():
    # (0, 0) -> (7, 3): x-major, y = (2 i 3 + 7) // 14 = 0 0 1 1 2 2 3 3 for i = 0..7
    assert (_drawn((0, 0), (7, 3), 1) == _picture(['##......',
                                                   '..##....',
                                                   '....##..',
                                                   '......##',
                                                   '........',
                                                   '........',
                                                   '........',
                                                   '........'])).all()
    # the reverse direction walks from the other end: y = 3 - (6 i + 7) // 14 at x = 7 - i
    assert (_drawn((7, 3), (0, 0), 1) == _picture(['##......',
                                                   '..##....',
                                                   '....##..',
                                                   '......##',
                                                   '........',
                                                   '........',
                                                   '........',
                                                   '........'])).all()


def test_hand_checked_thick_line():
    # thickness 2 stamps offsets {-1, 0}: the vertical line x = 3, y = 2..5 also covers x = 2 and y = 1
    assert (_drawn((3, 2), (3, 5), 2) == _picture(['........',
                                                   '..##....',
                                                   '..##....',
                                                   '..##....',
                                                   '..##....',
                                                   '..##....',
                                                   '........',
                                                   '........'])).all()
    # a zero-length segment is its stamp; at the corner the stamp is clipped
    assert (_drawn((0, 0), (0, 0), 2) == _picture(['#.......'] + ['........'] * 7)).all()
    assert _drawn((5, 5), (5, 5), 1).sum() == 1


def test_reference_panel_layout_and_draw_order():
    H, W = 8, 10
    left = np.full((H, W, 3), 10, np.uint8)
    right = np.full((H, W, 3), 20, np.uint8)
    rec = np.zeros((3, ref.REC_COLS), np.float32)
    rec[0, 0] = 2
    rec[1, 0], rec[1, 1:5], rec[1, 5:9] = 0.9, (1, 1, 5, 5), (0, 1, 4, 5)
    rec[2, 0], rec[2, 1:5], rec[2, 5:9] = 0.5, (2, 2, 6, 6), (2, 2, 6, 6)            # below the threshold: not drawn
    panel, tr = ref.render(left, right, rec, np.eye(3, 4), 0.7)
    res, x_max, y_max, _, _ = ref.bev_geometry(H)
    assert panel.shape == (2 * H, W + x_max, 3) and y_max == 2 * H
    assert (panel[:, W:] == 255).all()
    assert tuple(panel[1, 1]) == ref.RED and tuple(panel[H + 1, 0]) == ref.RED and tuple(panel[0, 0]) == (10, 10, 10)
    assert len(tr.segments['left']) == 4 and len(tr.segments['right']) == 4 and not tr.segments['bev']
    assert (panel[:H, :W] != 10).any(2).sum() == 16 and (panel[H:, :W] != 20).any(2).sum() == 16
