"""CPU: the KITTI evaluation's host side (parsing, cleanData, getThresholds, AP sums), the reference helper's geometry on
analytic cases, the reduced pass-2 choice against the devkit's sequential loop, and the library's argument checks of the
new entry points (no launch needed)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_ref as ref                                    # noqa: E402
from stereo_rcnn_amd import kitti_eval as ke                    # noqa: E402


def _label(type_, trunc=0.0, occ=0, alpha=0.0, box=(100, 100, 200, 150), dims=(1.5, 1.6, 3.9), loc=(1.0, 1.7, 20.0), ry=0.0):
    return (type_, trunc, occ, alpha) + tuple(box) + tuple(dims) + tuple(loc) + (ry,)


def _arr(rows, dtype=ke.LABEL_DTYPE):
    return np.array(rows, dtype=dtype)


def test_label_and_result_parsing_round_trip(tmp_path):
    p = tmp_path / '000001.txt'
    p.write_text('Car 0.00 0 -1.58 587.01 173.33 614.12 200.12 1.65 1.67 3.64 -0.65 1.71 46.70 -1.59\n'
                 'DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10\n'
                 'Person_sitting 0.3 2 0.1 1 2 3 4 5 6 7 8 9 10 0.5\n\n')
    a = ke.read_label(str(p))
    assert a.dtype == ke.LABEL_DTYPE and len(a) == 3
    assert list(a['type']) == ['Car', 'DontCare', 'Person_sitting']
    assert a['occluded'].tolist() == [0, -1, 2] and a['truncated'][2] == 0.3
    assert a['x1'][0] == 587.01 and a['z'][0] == 46.70 and a['ry'][0] == -1.59 and a['x'][1] == -1000
    (tmp_path / 'empty.txt').write_text('')
    assert len(ke.read_label(str(tmp_path / 'empty.txt'))) == 0

    # a result file written by the product's own writer
    from stereo_rcnn_amd.model.utils import kitti_utils
    calib = kitti_utils.FrameCalibrationData()
    calib.t_cam2_cam0 = np.array([0.06, 0.0, 0.0])
    res = tmp_path / 'res'
    kitti_utils.write_detection_results(str(res), '000001', calib, [10.5, 20.25, 110.0, 80.0], [2.0, 1.5, 30.0],
                                        [1.6, 1.5, 4.0], 0.3, 0.875)
    kitti_utils.write_detection_results(str(res), '000001', calib, [1, 2, 3, 4], [0.0, 1.0, 10.0], [1.0, 2.0, 3.0], 1.0, 0.5)
    r = ke.read_result(str(res / 'data' / '000001.txt'))
    assert r.dtype == ke.RESULT_DTYPE and len(r) == 2
    assert r['type'][0] == 'Car' and r['truncated'][0] == -1 and r['occluded'][0] == -1
    assert (r['x1'][0], r['y1'][0], r['x2'][0], r['y2'][0]) == (10.5, 20.25, 110.0, 80.0)
    assert (r['h'][0], r['w'][0], r['l'][0]) == (1.5, 1.6, 4.0)                  # the writer's dim order
    assert abs(r['x'][0] - 1.94) < 1e-9 and r['z'][0] == 30.0                  # x moved to cam0
    assert abs(r['ry'][0] - (0.3 - 1.57)) < 1e-6 and r['score'][0] == 0.875 and r['score'][1] == 0.5
    assert abs(r['alpha'][0] - (0.3 - math.pi / 2 + math.atan2(-2.0, 30.0))) < 1e-6


def test_load_split_listed_frames_and_missing_results(tmp_path):
    lab, res = tmp_path / 'label', tmp_path / 'res'
    (res / 'data').mkdir(parents=True)
    lab.mkdir()
    for i in ('000000', '000001', '000002'):
        (lab / (i + '.txt')).write_text('Car 0 0 0 1 1 50 60 1.5 1.6 3.9 1 1.7 20 0\n')
    (res / 'data' / '000000.txt').write_text('car -1 -1 0 1 1 50 60 1.5 1.6 3.9 1 1.7 20 0 0.9\n')
    (res / 'data' / '000002.txt').write_text('')
    ids, gts, dets = ke.load_split(str(lab), str(res), ['000000', '000001', '000002'])
    assert ids == ['000000', '000001', '000002'] and [len(d) for d in dets] == [1, 0, 0] and [len(g) for g in gts] == [1, 1, 1]
    ids, _, dets = ke.load_split(str(lab), str(res))                  # no list: the result files that exist
    assert ids == ['000000', '000002']
    ids, _, dets = ke.load_split(str(lab), str(res / 'data'))         # a bare result directory is accepted
    assert ids == ['000000', '000002'] and len(dets[0]) == 1


def test_clean_data_flags_every_branch():
    gt = _arr([_label('Car'),                                           # 0: car, easy
               _label('Van'),                                           # 1: neighbour -> 1
               _label('Car', box=(0, 100, 50, 140)),                    # 2: exactly 40 px: fails easy (<=), moderate ok
               _label('Car', box=(0, 100, 50, 125)),                    # 3: exactly 25 px: fails every difficulty
               _label('Car', trunc=0.15),                               # 4: truncation exactly 0.15: easy ok
               _label('Car', trunc=0.16, occ=1),                        # 5: moderate
               _label('Pedestrian'),                                    # 6: other class -> -1 for car
               _label('Person_sitting'),                                # 7: neighbour of pedestrian
               _label('car', occ=3),                                    # 8: case-insensitive; occlusion 3 fails all
               _label('DontCare', trunc=-1, occ=-1)])                   # 9: -1
    det = _arr([_label('Car') + (0.9,), _label('Car', box=(0, 0, 10, 24.9)) + (0.8,), _label('Pedestrian') + (0.7,),
                _label('CAR', box=(0, 0, 10, 40)) + (0.6,)], ke.RESULT_DTYPE)
    want_gt = {('Car', 0): [0, 1, 1, 1, 0, 1, -1, -1, 1, -1], ('Car', 1): [0, 1, 0, 1, 0, 0, -1, -1, 1, -1],
               ('Car', 2): [0, 1, 0, 1, 0, 0, -1, -1, 1, -1], ('Pedestrian', 0): [-1, -1, -1, -1, -1, -1, 0, 1, -1, -1]}
    want_det = {('Car', 0): [0, 1, -1, 0], ('Car', 1): [0, 1, -1, 0], ('Car', 2): [0, 1, -1, 0], ('Pedestrian', 0): [-1, 1, 0, -1]}
    types = np.char.lower(gt['type'].astype(str))
    dtypes = np.char.lower(det['type'].astype(str))
    for (cls, d), want in want_gt.items():
        ig, idt, n = ke.clean_flags(types, gt['truncated'], gt['occluded'], np.abs(gt['y1'] - gt['y2']), dtypes,
                                    det['y2'] - det['y1'], cls, d)
        assert ig.tolist() == want, (cls, d)
        assert idt.tolist() == want_det[(cls, d)], (cls, d)
        assert n == want.count(0)
        rg, rd, dc, rn = ref.clean_data(list(gt), list(det), cls, d)
        assert rg == want and rd == want_det[(cls, d)] and rn == n and len(dc) == 1


def test_get_thresholds_hand_cases():
    for f in (ke.get_thresholds, ref.get_thresholds):
        assert len(f([0.5] * 40, 40)) == 40
        t = f([i / 100.0 for i in range(100)], 100)
        assert len(t) == 41 and t[-1] == 0.0 and t[0] == 0.99          # the last score is always kept
        t = f([i / 10.0 for i in range(10)], 100)
        assert len(t) == 5 and t[-1] == 0.0
    v = list(np.random.default_rng(3).random(37).round(3))
    assert ke.get_thresholds(v, 50) == ref.get_thresholds(v, 50)


def test_average_precision_sums():
    p = [1.0] * 41
    e = ke.average_precision(p, 10)
    assert e['R11'] == pytest.approx(100.0) and e['R40'] == pytest.approx(100.0) and e['n_gt'] == 10
    p = [0.0] * 41
    p[20] = 0.5                                                        # the suffix maximum lifts p[0..19] to 0.5
    e = ke.average_precision(p, 3)
    assert e['precision'][:21] == [0.5] * 21 and e['precision'][21:] == [0.0] * 20
    assert e['R11'] == pytest.approx(100.0 / 11 * 0.5 * 6) and e['R40'] == pytest.approx(100.0 / 40 * 0.5 * 20)
    assert e['R11'] == ref.ap_r11(p) and e['R40'] == ref.ap_r40(p)
    p = [0.9, 0.3, 0.8] + [0.1] * 38
    e = ke.average_precision(p, 5)
    assert e['precision'][:3] == [0.9, 0.8, 0.8] and e['R40'] == ref.ap_r40(p) and e['R11'] == ref.ap_r11(p)
    e = ke.average_precision([0.0] * 41, 0)
    assert e['R11'] is None and e['R40'] is None and e['n_gt'] == 0


def _box(x=0.0, y=1.0, z=10.0, h=1.0, w=1.0, l=1.0, ry=0.0):
    return {'x': x, 'y': y, 'z': z, 'h': h, 'w': w, 'l': l, 'ry': ry}


def test_reference_geometry_analytic_cases():
    a = _box(l=3.9, w=1.6, h=1.5, ry=0.3)
    assert ref.ground_overlap(a, a) == pytest.approx(1.0, abs=1e-12)
    assert ref.box3d_overlap(a, a) == pytest.approx(1.0, abs=1e-12)
    sq, turned = _box(), _box(ry=math.pi / 4)
    inter = 2 * (math.sqrt(2) - 1)                                   # the regular octagon
    assert ref.bev_intersection(ref.footprint(sq), ref.footprint(turned)) == pytest.approx(inter, abs=1e-12)
    assert ref.ground_overlap(sq, turned) == pytest.approx(inter / (2 - inter), abs=1e-12)
    assert inter / (2 - inter) == pytest.approx(1 / math.sqrt(2), abs=1e-12)
    assert ref.ground_overlap(_box(w=2, l=2), _box(x=1, w=2, l=2)) == pytest.approx(1 / 3, abs=1e-12)
    assert ref.box3d_overlap(_box(h=2, y=1.0), _box(h=2, y=2.0)) == pytest.approx(1 / 3, abs=1e-12)   # y is the bottom face
    assert ref.ground_overlap(_box(), _box(x=5)) == 0.0 and ref.box3d_overlap(_box(), _box(y=10)) == 0.0
    # the rotation sense matters: +ry and -ry of an off-axis pair differ
    b = _box(l=4, w=1.5)
    assert abs(ref.ground_overlap(b, _box(x=1, l=4, w=1.5, ry=0.4)) - ref.ground_overlap(b, _box(x=1, l=4, w=1.5, ry=-0.4))) < 1e-12
    c = _box(x=1.0, z=10.5, l=4, w=1.5, ry=0.4)
    d = _box(x=1.0, z=10.5, l=4, w=1.5, ry=-0.4)
    assert abs(ref.ground_overlap(b, c) - ref.ground_overlap(b, d)) > 1e-3
    img = {'x1': 0, 'y1': 0, 'x2': 10, 'y2': 10}
    assert ref.image_overlap(img, {'x1': 5, 'y1': 0, 'x2': 15, 'y2': 10}) == pytest.approx(1 / 3)
    assert ref.image_overlap(img, {'x1': 5, 'y1': 0, 'x2': 15, 'y2': 10}, 0) == pytest.approx(0.5)


def test_reduced_pass2_choice_equals_the_sequential_loop():
    rng = np.random.default_rng(0)
    for trial in range(3000):
        n = int(rng.integers(0, 12))
        ov = rng.choice([0.0, 0.3, 0.5, 0.55, 0.7, 0.71, 0.9, 1.0], size=n)      # repeats: ties in overlap
        if trial % 3 == 0:
            ov = rng.random(n)
        ign = rng.choice([0, 1], size=n, p=[0.6, 0.4])
        cands = list(zip(ov.tolist(), ign.tolist()))
        for mo in (0.5, 0.7):
            assert ref.select_reduced(cands, mo) == ref.select_sequential(cands, mo), (cands, mo)


def test_overlap_options_and_table_format():
    assert ke.parse_overlaps(['car=0.7,0.5,0.5', 'CAR=0.7,0.7,0.7', 'cyclist=0.5,0.25,0.25']) == \
        {'Car': [(0.7, 0.5, 0.5), (0.7, 0.7, 0.7)], 'Cyclist': [(0.5, 0.25, 0.25)]}
    with pytest.raises(ValueError):
        ke.parse_overlaps(['truck=0.5,0.5,0.5'])
    e = ke.average_precision([1.0] * 41, 4)
    none = ke.average_precision([0.0] * 41, 0)
    res = {'Car': {'0.70, 0.70, 0.70': {m: {'easy': e, 'moderate': e, 'hard': none} for m in ('bbox', 'bev', '3d', 'aos')}}}
    txt = ke.format_table(res)
    assert txt.splitlines()[0] == 'Car AP@0.70, 0.70, 0.70:'
    assert 'bbox AP(R11): 100.0000, 100.0000,    n/a' in txt and 'aos  AP(R40):' in txt


@pytest.fixture(scope='module')
def lib():
    from stereo_rcnn_amd import _lib
    from stereo_rcnn_amd.csrc import build as hip_build
    hip_build.build(verbose=False)
    return _lib.lib()


def test_library_refuses_a_frame_over_the_detection_limit(lib):
    """Argument validation happens before any launch: a frame over SRCNN_KITTI_MAX_DET is an error, never a truncation."""
    from stereo_rcnn_amd import _lib
    assert lib.srcnn_version() >= 250
    s = _lib.KittiSplit()
    s.n_frames, s.max_det_per_frame = 1, ke.MAX_DET_PER_FRAME + 1
    m = _lib.KittiMatchDesc()
    m.n_cfg, m.n_slots, m.compute_fp = 1, 41, 1
    assert lib.srcnn_kitti_overlaps(ctypes.byref(s), None) == -1
    assert b'4096' in lib.srcnn_last_error()
    assert lib.srcnn_kitti_match(ctypes.byref(s), ctypes.byref(m), None) == -1
    s.max_det_per_frame = 3
    for f in ('det_off', 'gt_off', 'dc_off', 'pair_off', 'dcpair_off', 'ov_img', 'ov_bev', 'ov_3d', 'ov_dc'):
        setattr(s, f, 256)                                          # never dereferenced: the checks come first
    for f in ('cfg_flags', 'cfg_metric', 'cfg_min_overlap', 'cfg_n_thresh', 'thresholds', 'ign_gt', 'ign_det', 'gt_score',
              'tp', 'fp', 'fn', 'similarity'):
        setattr(m, f, 256)
    m.n_slots = 42                                                  # more than the 41 threshold slots
    assert lib.srcnn_kitti_match(ctypes.byref(s), ctypes.byref(m), None) == -1
    m.n_slots, m.compute_fp = 2, 0                                  # pass 1 has one slot
    assert lib.srcnn_kitti_match(ctypes.byref(s), ctypes.byref(m), None) == -1
    s.n_frames = 0                                                  # an empty split is a no-op
    assert lib.srcnn_kitti_overlaps(ctypes.byref(s), None) == 0


def test_run_kitti_forwards_the_split_arguments_then_evaluates_on_rank_0(monkeypatch, tmp_path):
    from stereo_rcnn_amd import run_kitti, test_net
    split = tmp_path / 'val.txt'
    split.write_text('000003\n000001\n')
    calls = []
    monkeypatch.setattr(test_net, 'main', lambda argv: calls.append(('split', list(argv))))
    monkeypatch.setattr(ke, 'evaluate_split', lambda *a, **k: calls.append(('eval', a[:3])) or 'table')
    argv = ['--kitti-root', 'K', '--split', str(split), '--label-dir=L', '--checkpoint', 'c.pth', '--result-dir', 'R',
            '--gather']
    monkeypatch.delenv('RANK', raising=False)
    assert run_kitti.main(argv) == 'table'
    assert calls == [('split', ['--kitti-root', 'K', '--split', str(split), '--checkpoint', 'c.pth', '--result-dir', 'R',
                                '--gather']),
                     ('eval', ('L', 'R', ['000003', '000001']))]
    calls.clear()
    monkeypatch.setenv('RANK', '1')                                 # other ranks run the split only
    assert run_kitti.main(['--label-dir', 'L'] + argv[:4] + argv[5:]) is None
    assert [c[0] for c in calls] == ['split']
