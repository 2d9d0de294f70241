"""MI355X: the KITTI evaluation's device kernels (csrc/kitti_eval.hip) against the loop-by-loop CPU transcription of the
devkit (tests/kitti_eval_ref.py) on seeded synthetic splits, the determinism of the result, the KITTI loop's --label-dir path
and the CLI, and the stated per-frame detection limit."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_ref as ref                                    # noqa: E402
from stereo_rcnn_amd import kitti_eval as ke                    # noqa: E402
from kitti_synth import _jitter, _round, _row, assert_same_result   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic_split(seed, n_frames=200, max_obj=6):
    """Labels mixing Car / Van / Pedestrian / Person_sitting / Cyclist / DontCare across the difficulty edges, and detections
    that are jittered copies, duplicates, drops, false positives, small boxes and boxes inside DontCare regions, with scores
    rounded so that ties occur."""
    rng = np.random.default_rng(seed)
    gts, dets = [], []
    types = ['Car', 'Car', 'Car', 'Van', 'Pedestrian', 'Pedestrian', 'Cyclist', 'Person_sitting']
    for f in range(n_frames):
        g = [_round(_row(rng, str(rng.choice(types)))) for _ in range(int(rng.integers(0, max_obj + 1)))]
        dcs = []
        if rng.random() < 0.4:
            r = _row(rng, 'Car')
            dcs.append(['DontCare', -1, -1, -10] + [round(v, 2) for v in r[4:8]] + [-1, -1, -1, -1000, -1000, -1000, -10])
        d = []
        for r in g:
            if rng.random() < 0.15:
                continue                                             # dropped
            t = {'Van': 'Car' if rng.random() < 0.5 else 'Van', 'Person_sitting': 'Pedestrian'}.get(r[0], r[0])
            d.append([t] + _jitter(rng, r)[1:])
            if rng.random() < 0.2:
                d.append([t] + _jitter(rng, r, 1.5)[1:])             # duplicate
        for _ in range(int(rng.integers(0, 3))):
            d.append(_row(rng, str(rng.choice(['Car', 'Pedestrian', 'Cyclist']))))    # pure false positives
        if rng.random() < 0.3:
            d.append(_row(rng, 'Car', height=float(rng.uniform(10, 24.9))))          # small
        for dc in dcs:
            if rng.random() < 0.7:                                   # inside a don't-care region
                x1, y1, x2, y2 = dc[4:8]
                bx = _row(rng, 'Car')
                bx[4:8] = [x1 + 0.2 * (x2 - x1), y1 + 0.1 * (y2 - y1), x2 - 0.1 * (x2 - x1), y2 - 0.2 * (y2 - y1)]
                d.append(bx)
        order = rng.permutation(len(d))
        d = [d[k] for k in order]
        rows = []
        for r in d:
            sc = float(rng.choice([0.5, 0.75, 0.9])) if rng.random() < 0.2 else round(float(rng.random()), 6)
            rows.append(tuple(_round([r[0], -1.0, -1] + list(r[3:]), 4)) + (sc,))
        gts.append(np.array([tuple(r) for r in g + dcs], dtype=ke.LABEL_DTYPE))
        dets.append(np.array(rows, dtype=ke.RESULT_DTYPE))
    return gts, dets


@pytest.fixture(scope='module')
def split():
    return synthetic_split(7)


@pytest.fixture(scope='module')
def device_result(split):
    return ke.evaluate(*split)


def _ref_overlaps(g, d):
    g = [r for r in g if str(r['type']).lower() != 'dontcare']
    return {'bbox': [[ref.image_overlap(x, y) for x in d] for y in g], 'bev': [[ref.ground_overlap(x, y) for x in d] for y in g],
            '3d': [[ref.box3d_overlap(x, y) for x in d] for y in g]}


def test_device_overlaps_match_reference():
    """~10k seeded det x gt pairs plus the degenerate cases: within 1e-12 of the vertex-set reference, never NaN."""
    rng = np.random.default_rng(11)
    gts, dets = [], []
    for f in range(100):
        g = [_row(rng, str(rng.choice(['Car', 'Pedestrian', 'Cyclist']))) for _ in range(10)]
        d = [_jitter(rng, r, float(rng.choice([0.5, 2.0, 6.0]))) for r in g]
        gts.append(np.array([tuple(r) for r in g], dtype=ke.LABEL_DTYPE))
        dets.append(np.array([tuple(r) + (0.5,) for r in d], dtype=ke.RESULT_DTYPE))
    base = ['Car', 0.0, 0, 0.0, 100.0, 100.0, 200.0, 160.0, 1.5, 2.0, 4.0, 0.0, 1.5, 20.0, 0.0]

    def b(**kw):
        r = list(base)
        for k, v in kw.items():
            r[{'x1': 4, 'y1': 5, 'x2': 6, 'y2': 7, 'h': 8, 'w': 9, 'l': 10, 'x': 11, 'y': 12, 'z': 13, 'ry': 14}[k]] = v
        return r
    pairs = [(b(), b()),                                                 # identical
             (b(), b(w=1.0, l=2.0, h=1.0)),                              # contained
             (b(), b(x=4.0)),                                            # shared edge, no area
             (b(), b(x=2.0)),                                            # collinear edges, half overlap
             (b(ry=math.pi / 2), b(ry=-math.pi / 2)),                    # +-pi/2
             (b(ry=math.pi / 2), b(ry=0.0)),
             (b(), b(x=30.0, x1=500.0, x2=600.0)),                       # no contact
             (b(l=0.0), b()), (b(), b(w=0.0)), (b(l=0.0, w=0.0), b(l=0.0, w=0.0)),   # zero extent
             (b(h=0.0), b(h=0.0)), (b(x2=100.0), b()),                   # zero height, zero-width 2-D box
             (b(ry=0.3), b(ry=0.3 + math.pi)),                           # the same footprint turned half a turn
             (b(x=1.0, z=20.5, ry=0.4), b(x=1.0, z=20.5, ry=-0.4))]
    for d, g in pairs:
        gts.append(np.array([tuple(g)], dtype=ke.LABEL_DTYPE))
        dets.append(np.array([tuple(d) + (0.5,)], dtype=ke.RESULT_DTYPE))
    got = ke.overlaps(gts, dets)
    n, worst = 0, 0.0
    for g, d, e in zip(gts, dets, got):
        want = _ref_overlaps(g, d)
        for m in ('bbox', 'bev', '3d'):
            a = e[m]
            assert np.isfinite(a).all()
            diff = np.abs(a - np.array(want[m]).reshape(a.shape))
            worst = max(worst, float(diff.max()) if diff.size else 0.0)
            n += a.size
    assert n >= 3 * 10000 and worst <= 1e-12, worst
    deg = got[100:]
    assert deg[0]['bev'][0, 0] == pytest.approx(1.0, abs=1e-12) and deg[0]['3d'][0, 0] == pytest.approx(1.0, abs=1e-12)
    assert deg[1]['bev'][0, 0] == pytest.approx(2.0 / 8.0, abs=1e-12)
    assert deg[2]['bev'][0, 0] == pytest.approx(0.0, abs=1e-12) and deg[3]['bev'][0, 0] == pytest.approx(1 / 3, abs=1e-12)
    assert deg[4]['bev'][0, 0] == pytest.approx(1.0, abs=1e-12) and deg[6]['bev'][0, 0] == 0.0 and deg[6]['bbox'][0, 0] == 0.0
    assert all(deg[k]['bev'][0, 0] == 0.0 for k in (7, 8, 9)) and deg[10]['3d'][0, 0] == 0.0


def test_split_parity_with_reference(split, device_result):
    gts, dets = split
    # no overlap lies within 1e-9 of a minimum overlap: rounding cannot decide a comparison
    mins = sorted({v for sets in ke.DEFAULT_OVERLAPS.values() for t in sets for v in t})
    for g, d in zip(gts, dets):
        ov = _ref_overlaps(g, d)
        dc = [[ref.image_overlap(x, y, 0) for x in d] for y in g if str(y['type']).lower() == 'dontcare']
        vals = np.array([v for m in ov.values() for row in m for v in row] + [v for row in dc for v in row])
        if vals.size:
            assert min(np.abs(vals - t).min() for t in mins) > 1e-9
    want = ref.evaluate(gts, dets)
    got = device_result
    assert list(got) == list(want) == ['Car', 'Pedestrian', 'Cyclist']
    n_thr = 0
    for c in want:
        assert list(got[c]) == list(want[c])
        for key in want[c]:
            for m in ('bbox', 'bev', '3d', 'aos'):
                for diff in ref.DIFFICULTIES:
                    w, e = want[c][key][m][diff], got[c][key][m][diff]
                    assert e['n_gt'] == w['n_gt'], (c, key, m, diff)
                    if m == 'aos':
                        assert (e['R11'] is None) == (w['R11'] is None)
                        if w['R11'] is not None:
                            assert abs(e['R11'] - w['R11']) <= 1e-12 and abs(e['R40'] - w['R40']) <= 1e-12
                        assert np.abs(np.array(e['precision']) - np.array(w['precision'])).max() <= 1e-12
                        continue
                    assert e['thresholds'] == w['thresholds'], (c, key, m, diff)
                    assert (e['tp'], e['fp'], e['fn']) == (w['tp'], w['fp'], w['fn']), (c, key, m, diff)
                    assert e['precision'] == w['precision'] and e['R11'] == w['R11'] and e['R40'] == w['R40']
                    n_thr += len(w['thresholds'])
    assert n_thr > 500                                                   # the split exercises the threshold sweep
    car = got['Car']['0.70, 0.70, 0.70']['bbox']['moderate']
    assert 0 < car['R40'] < 100 and sum(car['fp']) > 0


def test_two_runs_are_bit_identical(split, device_result):
    again = ke.evaluate(*split)
    assert json.dumps(again, sort_keys=True) == json.dumps(device_result, sort_keys=True)


def _write_kitti_tree(root, gts, ids):
    """label_2/, calib/ (P0 == P2: no cam0 shift) of a synthetic split."""
    p2 = np.array([721.5377, 0, 609.5593, 0.0, 0, 721.5377, 172.854, 0.0, 0, 0, 1, 0.0])
    rowtxt = lambda name, mat: name + ': ' + ' '.join('%.12e' % v for v in np.ravel(mat))
    for d in ('label_2', 'calib'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for i, g in zip(ids, gts):
        with open(os.path.join(root, 'label_2', i + '.txt'), 'w') as fh:
            for r in g:
                fh.write('%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n' % tuple(r))
        with open(os.path.join(root, 'calib', i + '.txt'), 'w') as fh:
            fh.write('\n'.join([rowtxt('P0', p2), rowtxt('P1', p2), rowtxt('P2', p2), rowtxt('P3', p2),
                                rowtxt('R0_rect', np.eye(3)), rowtxt('Tr_velo_to_cam', np.eye(3, 4))]) + '\n')


def test_ground_truth_as_detections_through_the_kitti_loop_and_cli(tmp_path, monkeypatch):
    """Car ground truth written back as detections through test_net.run_split's writer, driven by run_kitti, gives AP = 100
    wherever there is ground truth; a listed frame whose result file is missing loses exactly its ground truths; the CLI prints the table and
    writes the same dict as evaluate()."""
    from stereo_rcnn_amd import test_net
    gts, _ = synthetic_split(5, n_frames=200)
    for g in gts:                                   # every other car made easy: n_gt > 40 at every difficulty, so that the
        car = np.flatnonzero(g['type'] == 'Car')[::2]   # 41 recall points can all be reached (n_gt <= 40 caps AP below 100)
        g['truncated'][car], g['occluded'][car] = 0.0, 0
        g['y2'][car] = np.maximum(g['y2'][car], g['y1'][car] + 45.0)
    ids = ['%06d' % i for i in range(len(gts))]
    root, res = str(tmp_path / 'training'), str(tmp_path / 'res')
    _write_kitti_tree(root, gts, ids)
    by_id = dict(zip(ids, gts))

    def detect(frames):
        for k, _ in enumerate(frames):
            objs = []
            for r in by_id[ids[k]]:
                if r['type'] != 'Car':
                    continue
                objs.append({'score': 0.5 + 0.001 * len(objs), 'box_left': [r['x1'], r['y1'], r['x2'], r['y2']],
                             'xyz': [r['x'], r['y'], r['z']], 'dim': [r['w'], r['h'], r['l']], 'theta': r['ry'] + 1.57,
                             'aligned': True})
            yield objs
    split_txt = str(tmp_path / 'val.txt')
    with open(split_txt, 'w') as fh:
        fh.write('\n'.join(ids) + '\n')
    written = []

    def split_driver(argv):                         # test_net.main with the detector replaced: run_split and its writer
        a = dict(zip(argv[::2], argv[1::2]))
        assert len(argv) == 8 and a['--checkpoint'] == 'model.pth' and '--label-dir' not in a
        written.append(test_net.run_split(None, a['--kitti-root'], test_net.read_split(a['--split']), a['--result-dir'], None,
                                          read_image=lambda p: np.zeros((4, 4, 3), np.uint8), detect_stream=detect))
    monkeypatch.setattr(test_net, 'main', split_driver)
    from stereo_rcnn_amd import run_kitti
    full = run_kitti.main(['--kitti-root', root, '--label-dir', os.path.join(root, 'label_2'), '--split', split_txt,
                           '--checkpoint', 'model.pth', '--result-dir', res])
    frames, n_obj, _ = written[0]
    assert frames == len(ids) and n_obj == sum(int((g['type'] == 'Car').sum()) for g in gts)
    assert list(full) == ['Car']
    for key, by_metric in full['Car'].items():
        for m in ('bbox', 'bev', '3d'):
            for diff in ke.DIFFICULTIES:
                e = by_metric[m][diff]
                assert e['n_gt'] > 40 and len(e['thresholds']) == 41 and e['R11'] == pytest.approx(100.0, abs=1e-9) and e['R40'] == pytest.approx(100.0, abs=1e-9)
    assert json.load(open(os.path.join(res, 'ap.json'))) == full

    # drop the result file of the frame with the most moderate cars: recall falls by exactly its ground truths
    flags = lambda g, d: ke.clean_flags(np.char.lower(g['type'].astype(str)), g['truncated'], g['occluded'],
                                        np.abs(g['y1'] - g['y2']), np.zeros(0, 'U1'), np.zeros(0), 'Car', d)[2]
    k = max(range(len(ids)), key=lambda i: flags(gts[i], 1))
    lost = [flags(gts[k], d) for d in range(3)]
    assert lost[1] > 0
    os.remove(os.path.join(res, 'data', ids[k] + '.txt'))
    _, g2, d2 = ke.load_split(os.path.join(root, 'label_2'), res, ids)
    part = ke.evaluate(g2, d2)
    for d, diff in enumerate(ke.DIFFICULTIES):
        e = part['Car']['0.70, 0.70, 0.70']['3d'][diff]
        n = e['n_gt']
        assert e['tp'][-1] == n - lost[d] and e['fn'][-1] == lost[d] and e['fp'][-1] == 0

    out_json = str(tmp_path / 'cli.json')
    proc = subprocess.run([sys.executable, '-m', 'stereo_rcnn_amd.kitti_eval', '--label-dir', os.path.join(root, 'label_2'),
                           '--result-dir', res, '--split', split_txt, '--json', out_json], cwd=ROOT, capture_output=True,
                          text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    assert 'Car AP@0.70, 0.70, 0.70:' in proc.stdout and 'Car AP@0.70, 0.50, 0.50:' in proc.stdout
    assert '%d frames:' % len(ids) in proc.stdout
    assert json.load(open(out_json)) == json.loads(json.dumps(part))


def test_frame_over_the_detection_limit_is_an_error():
    rng = np.random.default_rng(1)
    g = np.array([tuple(_row(rng, 'Car'))], dtype=ke.LABEL_DTYPE)
    big = np.array([tuple(_row(rng, 'Car')) + (0.5,)] * (ke.MAX_DET_PER_FRAME + 1), dtype=ke.RESULT_DTYPE)
    ok = np.array([tuple(_row(rng, 'Car')) + (0.5,)] * ke.MAX_DET_PER_FRAME, dtype=ke.RESULT_DTYPE)
    res = ke.evaluate([g, g], [ok[:3], ok])                              # exactly at the limit: evaluated, and right
    assert_same_result(res, ref.evaluate([g, g], [ok[:3], ok]))          # (no detection lies on g: no threshold anywhere)
    on = np.array([tuple(g[0]) + (0.5,)] * ke.MAX_DET_PER_FRAME, dtype=ke.RESULT_DTYPE)      # ... and with every one on it
    assert assert_same_result(ke.evaluate([g, g], [on[:3], on]), ref.evaluate([g, g], [on[:3], on])) > 0
    with pytest.raises(RuntimeError, match='4096'):
        ke.evaluate([g, g], [ok[:3], big])
