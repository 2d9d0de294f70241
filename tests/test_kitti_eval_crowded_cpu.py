"""CPU: what test_kitti_eval_crowded_gpu.py relies on, held without a GPU -- the exact-rational BEV intersection against
analytic cases and against the float reference, the float reference's measured distance from it (the source of
tolerances.KITTI_BEV_EXACT), the crowded split's preconditions, and the planted frames' literals against the reference."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_ref as ref                                    # noqa: E402
import kitti_synth as ks                                        # noqa: E402
import tolerances                                               # noqa: E402


def _box(x=0.0, y=1.0, z=10.0, h=1.0, w=1.0, l=1.0, ry=0.0):
    return {'x': x, 'y': y, 'z': z, 'h': h, 'w': w, 'l': l, 'ry': ry}


def _exact(a, b):
    return ref.bev_intersection_exact(ref.footprint(a), ref.footprint(b))


def test_exact_intersection_analytic_cases():
    a = _box(l=3.9, w=1.6, h=1.5, ry=0.3)
    assert ref.ground_overlap(a, a, ref.bev_intersection_exact) == pytest.approx(1.0, abs=1e-14)
    sq, turned = _box(), _box(ry=math.pi / 4)
    assert _exact(sq, turned) == pytest.approx(2 * (math.sqrt(2) - 1), abs=1e-14)       # the regular octagon
    assert _exact(turned, sq) == pytest.approx(2 * (math.sqrt(2) - 1), abs=1e-14)
    assert ref.ground_overlap(_box(w=2, l=2), _box(x=1, w=2, l=2), ref.bev_intersection_exact) == 1 / 3
    assert ref.box3d_overlap(_box(h=2, y=1.0), _box(h=2, y=2.0), ref.bev_intersection_exact) == 1 / 3
    assert _exact(_box(), _box(x=5)) == 0.0
    assert _exact(_box(), _box(x=1)) == 0.0 and _exact(_box(), _box(x=1, z=11)) == 0.0   # a shared edge, a shared corner
    assert _exact(_box(w=2, l=2), _box(w=1, l=1)) == 1.0 and _exact(_box(w=1, l=1), _box(w=2, l=2)) == 1.0   # contained
    assert _exact(_box(l=0.0), _box()) == 0.0 and _exact(_box(), _box(w=0.0)) == 0.0     # zero extent
    assert _exact(_box(l=2), _box(l=2, ry=math.pi)) == pytest.approx(2.0, abs=1e-14)     # half a turn: the other orientation
    # the rotation sense: +ry and -ry of an off-axis pair differ, of an on-axis pair they do not
    b = _box(l=4, w=1.5)
    exact = lambda d, g: ref.ground_overlap(d, g, ref.bev_intersection_exact)                    # noqa: E731
    assert abs(exact(b, _box(x=1, l=4, w=1.5, ry=0.4)) - exact(b, _box(x=1, l=4, w=1.5, ry=-0.4))) < 1e-14
    c, d = _box(x=1.0, z=10.5, l=4, w=1.5, ry=0.4), _box(x=1.0, z=10.5, l=4, w=1.5, ry=-0.4)
    assert abs(exact(b, c) - exact(b, d)) > 1e-3
    assert abs(exact(b, c) - ref.ground_overlap(b, c)) < 1e-12 and abs(exact(b, d) - ref.ground_overlap(b, d)) < 1e-12
    assert ref.ground_and_box3d_overlap(a, _box(x=0.5, l=3.9, w=1.6, ry=0.1)) == \
        (ref.ground_overlap(a, _box(x=0.5, l=3.9, w=1.6, ry=0.1)), ref.box3d_overlap(a, _box(x=0.5, l=3.9, w=1.6, ry=0.1)))


def test_exact_intersection_against_the_float_reference_in_general_position():
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(1500):
        a = _box(x=float(rng.uniform(-15, 15)), z=float(rng.uniform(5, 60)), l=3.9, w=1.6, ry=float(rng.uniform(-3.2, 3.2)))
        b = _box(x=a['x'] + float(rng.normal(0, 1)), z=a['z'] + float(rng.normal(0, 1)), l=4.2, w=1.7, ry=float(rng.uniform(-3.2, 3.2)))
        worst = max(worst, abs(_exact(a, b) - ref.bev_intersection(ref.footprint(a), ref.footprint(b))))
    assert 0.0 < worst <= 1e-12


def test_float_reference_on_boxes_end_to_end():
    """Two boxes one length apart along their axis: their side edges lie end to end on one line.  The float reference once
    took a 'crossing' of two such edges anywhere along them (an IoU of up to 0.14 where the truth is below 1e-11)."""
    g = _box(x=-1.1894696476150592, z=43.5615396832051, l=1.6805611106880545, w=0.5857695234576358, ry=1.3085278116119659)
    d = dict(g, x=-0.7537469403518012, z=41.938446534586326)
    assert ref.ground_overlap(d, g, ref.bev_intersection_exact) < 1e-11
    assert abs(ref.ground_overlap(d, g) - ref.ground_overlap(d, g, ref.bev_intersection_exact)) < 1e-11


def test_float_reference_distance_from_exact_sets_the_device_tolerance():
    """tolerances.KITTI_BEV_EXACT is four times the float reference's own distance from exact arithmetic over the sweep."""
    worst = {'near': 0.0, 'far': 0.0}
    n = 0
    for band, g, d, kinds in ks.bev_sweep():
        o = ks.exact_overlaps(g, d, also_float=True)
        worst[band] = max(worst[band], float(np.abs(o[:2] - o[2:]).max()))
        n += len(kinds)
        assert set(kinds) <= set(ks.SWEEP_KINDS)
    assert n >= 20000
    print('float reference vs exact:', worst)
    for band, w in worst.items():                 # an upper bound: the maxima are rounding noise and move with the host's sin / cos
        assert 0.0 < w <= 1.05 * tolerances.KITTI_BEV_REFERENCE_MEASURED[band], (band, w)
        assert tolerances.KITTI_BEV_EXACT[band] == pytest.approx(4 * tolerances.KITTI_BEV_REFERENCE_MEASURED[band], rel=0.02)


def test_crowded_split_preconditions():
    gts, dets = ks.crowded_split()
    assert [len(d) for d in dets] == list(ks.CROWDED_SIZES) + [200]
    for g, n_dc in zip(gts, ks.CROWDED_DONTCARE):
        t = np.char.lower(g['type'].astype(str))
        assert int((t == 'dontcare').sum()) == n_dc and 8 <= int((t != 'dontcare').sum()) <= 12
    scores = np.concatenate([d['score'] for d in dets[:-1]])          # the generated frames
    assert (scores < 0).any() and scores.min() > -1.0 and np.isin(scores, [0.5, 0.75, 0.9]).mean() > 0.3
    cache = {}
    want = ref.evaluate(gts, dets, cache=cache)
    margin, positive = ks.threshold_margin(cache)
    assert margin > 1e-9 and positive > 5000, (margin, positive)
    car = want['Car']['0.70, 0.70, 0.70']['bbox']['hard']
    assert len(car['thresholds']) >= 10 and sum(car['fp']) > 0 and sum(car['fn']) > 0
    # the traced copy of the loop counts what the reference counts, and finds every situation -- each in a form in which the
    # wrong choice changes the counts -- in the split, and in the planted frame alone (the random frames hold only some)
    n = [0]

    def same(st, want_st):
        assert (st['tp'], st['fn'], st['v']) == (want_st['tp'], want_st['fn'], want_st['v'])
        n[0] += 1
    seen = ks.census(gts, dets, cache, check=same)
    assert n[0] > 1000 and all(seen[s] > 0 for s in ks.SITUATIONS), seen
    planted = ks.census(gts[-1:], dets[-1:], {m: cache[m][-1:] for m in cache})
    assert all(planted[s] > 0 for s in ks.SITUATIONS), planted
    # don't-care boxes: the matrix is not empty, and some detections lie in two regions at once
    in_dc = [np.array(dcov) > 0.7 for _, dcov in cache[ref.IMAGE] if len(dcov)]
    assert sum(int(m.sum()) for m in in_dc) > 300 and any((m.sum(axis=0) >= 2).any() for m in in_dc)


def test_planted_literals_hold_in_the_reference():
    ks.expect_tie_frame(ref.evaluate([ks.tie_frame()[0]], [ks.tie_frame()[1]]))
    for n in ks.PLANTED_N:
        ks.expect_identical(ref.evaluate(*ks.identical_detections(n)), n)
    for n in ks.PLANTED_N[:3]:
        for p in ks.BEST_AT:
            if p < n:
                ks.expect_best_score(ref.evaluate(*ks.best_score_at(n, p)))
    ks.expect_best_score(ref.evaluate(*ks.best_score_at(4096, 128)))
    for k in (2, 65, 70):
        ks.expect_stacked(ref.evaluate(*ks.identical_detections(130, n_gt=k)), 130, k)
    ks.expect_valid_behind_ignored(ref.evaluate(*ks.ignored_candidates(True)))
    ks.expect_all_ignored(ref.evaluate(*ks.ignored_candidates(False)))
    for n_regions in (1, 2):
        ks.expect_inside_dontcare(ref.evaluate(*ks.inside_dontcare(n_regions)))
