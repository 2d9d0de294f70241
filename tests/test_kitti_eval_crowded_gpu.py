"""MI355X: kitti_match_kernel and kitti_overlaps_kernel where a frame holds more than 64 detections -- several 64-wide chunks
per lane, assigned bits above bit 0, ties between lanes and chunks -- against the devkit transcription (tests/kitti_eval_ref.py)
exactly, against literals on planted frames, and the BEV / 3-D overlaps against exact rational arithmetic on near-degenerate
boxes (tests/kitti_synth.py makes all inputs; test_kitti_eval_crowded_cpu.py holds their preconditions without a GPU).

Measured: the reference side of this module (Python loops and rational arithmetic) takes 20 s, the device side (every
ke.evaluate / ke.overlaps call together) 0.3 s.  Device BEV / 3-D IoU against exact arithmetic over the sweep: 2.7e-12 (z <= 80 m) and 9.7e-12 (z ~ 500 m) against the 6.6e-11 and 7.2e-11 of KITTI_BEV_EXACT in tests/tolerances.py.
"""
import json
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_ref as ref                                    # noqa: E402
import kitti_synth as ks                                        # noqa: E402
import tolerances                                               # noqa: E402
from stereo_rcnn_amd import kitti_eval as ke                    # noqa: E402

pytestmark = pytest.mark.gpu

SPENT = {'reference': 0.0, 'device': 0.0}


def _timed(side, f, *a, **k):
    t = time.perf_counter()
    out = f(*a, **k)
    SPENT[side] += time.perf_counter() - t
    return out


@pytest.fixture(scope='module', autouse=True)
def _report_time():
    yield
    print('\ntest_kitti_eval_crowded_gpu: reference side %.1f s, device side %.1f s' % (SPENT['reference'], SPENT['device']))


@pytest.fixture(scope='module')
def split():
    return ks.crowded_split()


@pytest.fixture(scope='module')
def reference(split):
    cache = {}
    return _timed('reference', ref.evaluate, *split, cache=cache), cache


@pytest.fixture(scope='module')
def device_result(split):
    return _timed('device', ke.evaluate, *split)


def test_crowded_split_parity_with_reference(split, reference, device_result):
    gts, dets = split
    want, cache = reference
    assert [len(d) for d in dets[:len(ks.CROWDED_SIZES)]] == list(ks.CROWDED_SIZES)
    # no overlap lies within 1e-9 of a minimum overlap: rounding cannot decide a comparison
    margin, positive = ks.threshold_margin(cache)
    assert margin > 1e-9 and positive > 5000, (margin, positive)
    assert list(want) == ['Car', 'Pedestrian', 'Cyclist']
    assert ks.assert_same_result(device_result, want) > 300
    # the split reaches a long threshold sweep with false positives, misses and don't-care suppression in one configuration
    car = want['Car']['0.70, 0.70, 0.70']['bbox']['hard']
    assert len(car['thresholds']) >= 10 and sum(car['fp']) > 0 and sum(car['fn']) > 0
    bare = [g[np.char.lower(g['type'].astype(str)) != 'dontcare'] for g in gts]
    no_dc = _timed('reference', ref.evaluate, bare, dets, classes=('Car',))['Car']['0.70, 0.70, 0.70']['bbox']['hard']
    assert no_dc['thresholds'] == car['thresholds'] and sum(no_dc['fp']) > sum(car['fp'])
    # ... and every situation the chunked reduction has to get right, found through the reference's loop
    seen = _timed('reference', ks.census, gts, dets, cache)
    assert all(seen[s] > 0 for s in ks.SITUATIONS), seen


def test_each_crowded_frame_alone(split, reference):
    """A split of one frame: an error in a frame cannot be cancelled by another in the sums."""
    gts, dets = split
    _, cache = reference
    n = 0
    for f, (g, d) in enumerate(zip(gts, dets)):
        if len(d) < 65:
            continue
        want = _timed('reference', ref.evaluate, [g], [d], cache={m: [cache[m][f]] for m in cache})
        ks.assert_same_result(_timed('device', ke.evaluate, [g], [d]), want, where='frame %d (%d detections)' % (f, len(d)))
        n += 1
    assert n == sum(s >= 65 for s in ks.CROWDED_SIZES) + 1


def test_crowded_overlaps(split, reference):
    """The 2-D and the don't-care overlaps are `+ - * / min max` on the same doubles in the reference's order: bit-equal.  BEV
    and 3-D against exact arithmetic at the sweep's near-band tolerance."""
    gts, dets = split
    _, cache = reference
    got = _timed('device', ke.overlaps, gts, dets)
    tol = tolerances.KITTI_BEV_EXACT['near']
    n_dc = 0
    for f, (g, d, e) in enumerate(zip(gts, dets, got)):
        keep = np.char.lower(g['type'].astype(str)) != 'dontcare'
        ov, dcov = cache[ref.IMAGE][f]
        want = np.array([row for row, k in zip(ov, keep) if k]).reshape(e['bbox'].shape)
        assert np.array_equal(e['bbox'], want), f
        assert e['dontcare'].shape == (int((~keep).sum()), len(d))
        assert np.array_equal(e['dontcare'], np.array(dcov).reshape(e['dontcare'].shape)), f
        n_dc += int((e['dontcare'] > 0).sum())
        bev, box3d = _timed('reference', ks.exact_overlaps, g[keep], d)
        assert np.isfinite(e['bev']).all() and np.isfinite(e['3d']).all()
        assert tolerances.observe('kitti_crowded_bev_vs_exact', np.abs(e['bev'] - bev).max(initial=0.0)) <= tol, f
        assert tolerances.observe('kitti_crowded_3d_vs_exact', np.abs(e['3d'] - box3d).max(initial=0.0)) <= tol, f
    assert n_dc > 300                                            # the don't-care matrix is compared where it is not zero


def test_two_crowded_runs_are_bit_identical(split, device_result):
    again = _timed('device', ke.evaluate, *split)
    assert json.dumps(again, sort_keys=True) == json.dumps(device_result, sort_keys=True)


# ---------------------------------------------------------------- planted frames: the answers are literals

def _both(gts, dets):
    got = _timed('device', ke.evaluate, gts, dets)
    ks.assert_same_result(got, _timed('reference', ref.evaluate, gts, dets))
    assert list(got) == ['Car']
    return got


def test_tie_frame_where_every_tie_has_a_consequence():
    ks.expect_tie_frame(_both([ks.tie_frame()[0]], [ks.tie_frame()[1]]))


@pytest.mark.parametrize('n', ks.PLANTED_N)
def test_identical_detections_on_one_ground_truth(n):
    ks.expect_identical(_both(*ks.identical_detections(n)), n)


@pytest.mark.parametrize('n,p', [(n, p) for n in ks.PLANTED_N for p in ks.BEST_AT if p < n])
def test_best_score_at_an_index(n, p):
    ks.expect_best_score(_both(*ks.best_score_at(n, p)))


@pytest.mark.parametrize('k', (2, 65, 70))
def test_stacked_ground_truths_take_different_detections(k):
    ks.expect_stacked(_both(*ks.identical_detections(130, n_gt=k)), 130, k)


def test_a_valid_candidate_behind_seventy_ignored_ones():
    ks.expect_valid_behind_ignored(_both(*ks.ignored_candidates(True)))


def test_all_candidates_ignored():
    ks.expect_all_ignored(_both(*ks.ignored_candidates(False)))


@pytest.mark.parametrize('n_regions', (1, 2))
def test_detections_inside_dontcare_regions(n_regions):
    ks.expect_inside_dontcare(_both(*ks.inside_dontcare(n_regions)))


# ---------------------------------------------------------------- BEV / 3-D overlaps against exact arithmetic

def test_near_degenerate_overlaps_against_exact_arithmetic():
    """20 000 pairs a perturbation of 1e-16 .. 1e-3 apart (kitti_synth.bev_sweep), 200 x 200 per frame, every entry compared."""
    sweep = ks.bev_sweep()
    assert sum(len(k) for _, _, _, k in sweep) >= 20000
    gts, dets = [s[1] for s in sweep], [s[2] for s in sweep]
    got = _timed('device', ke.overlaps, gts, dets)
    back = _timed('device', ke.overlaps, *zip(*[ks.swapped(g, d) for g, d in zip(gts, dets)]))
    worst = {}
    for (band, g, d, kinds), e, b in zip(sweep, got, back):
        tol = tolerances.KITTI_BEV_EXACT[band]
        bev, box3d = _timed('reference', ks.exact_overlaps, g, d)
        for name, want in (('bev', bev), ('3d', box3d)):
            a = e[name]
            assert a.shape == (ks.SWEEP_PER_FRAME, ks.SWEEP_PER_FRAME) and np.isfinite(a).all()
            assert a.min() >= 0.0 and a.max() <= 1.0 + tol
            dev = tolerances.observe('kitti_%s_vs_exact_%s' % (name, band), np.abs(a - want).max())
            sym = tolerances.observe('kitti_%s_symmetry_%s' % (name, band), np.abs(a - b[name].T).max())
            worst[name, band] = max(worst.get((name, band), 0.0), dev)
            assert dev <= tol, (name, band, dev, tol)
            assert sym <= 2 * tol, (name, band, sym)
        same = np.array([k == 'same' for k in kinds])
        assert same.any() and np.abs(np.diag(e['bev'])[same] - 1.0).max() <= tol and np.abs(np.diag(e['3d'])[same] - 1.0).max() <= tol
    print('\ndevice vs exact: ' + ', '.join('%s %s %.2e' % (k + (v,)) for k, v in sorted(worst.items())))
