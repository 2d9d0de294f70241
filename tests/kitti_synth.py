"""Seeded inputs of the KITTI evaluation tests (no test in here; imported by the CPU and the GPU modules alike):

  * the row makers of the synthetic splits (_row, _round, _jitter);
  * crowded_split: frames whose detection counts straddle the 64-wide chunks of kitti_match_kernel, full of ties, exact
    duplicates, ignored candidates and don't-care boxes, plus one hand-built frame (tie_frame) that holds every tie / ignore
    situation the chunked reduction has to get right;
  * census: a copy of the reference's greedy loop that also records each ground truth's candidates, to *find* those
    situations in a split (test_kitti_eval_crowded_cpu.py holds the copy to the reference's counts);
  * the planted frames whose answers are literals, and assert_same_result, the entry-for-entry comparison;
  * bev_sweep: near-degenerate (gt, det) box pairs for the BEV / 3-D overlaps, and exact_overlaps, their exact yardstick.
"""
import collections
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_ref as ref                                    # noqa: E402
from stereo_rcnn_amd import kitti_eval as ke                    # noqa: E402

DIMS = {'Car': (1.5, 1.6, 3.9), 'Van': (2.2, 1.9, 5.0), 'Pedestrian': (1.75, 0.6, 0.8), 'Person_sitting': (1.2, 0.6, 0.9),
        'Cyclist': (1.7, 0.6, 1.8)}


def _row(rng, type_, height=None):
    h2 = float(rng.choice([25.0, 40.0])) if height is None and rng.random() < 0.15 else (height or float(rng.uniform(15, 150)))
    x1, y1 = float(rng.uniform(0, 1100)), float(rng.uniform(100, 220))
    w2 = h2 * float(rng.uniform(0.4, 2.2))
    h, w, l = (d * float(rng.uniform(0.9, 1.1)) for d in DIMS[type_])
    return [type_, float(rng.choice([0.0, 0.1, 0.15, 0.2, 0.3, 0.45, 0.5, 0.7])), int(rng.integers(0, 4)),
            float(rng.uniform(-math.pi, math.pi)), x1, y1, x1 + w2, y1 + h2, h, w, l,
            float(rng.uniform(-15, 15)), float(rng.uniform(1.0, 2.5)), float(rng.uniform(5, 60)), float(rng.uniform(-math.pi, math.pi))]


def _round(r, nd=2):
    return [r[0], round(r[1], 2), r[2]] + [round(v, nd) for v in r[3:]]


def _jitter(rng, r, s=1.0):
    r = list(r)
    for k in range(4, 8):
        r[k] += float(rng.normal(0, 2.0 * s))
    r[7] = max(r[7], r[5] + 1.0)
    r[6] = max(r[6], r[4] + 1.0)
    for k in (8, 9, 10):
        r[k] *= float(rng.uniform(1 - 0.08 * s, 1 + 0.08 * s))
    r[11] += float(rng.normal(0, 0.25 * s))
    r[12] += float(rng.normal(0, 0.1 * s))
    r[13] += float(rng.normal(0, 0.5 * s))
    r[14] += float(rng.normal(0, 0.15 * s))
    r[3] += float(rng.normal(0, 0.3))
    return r


def labels(rows):
    return np.array([tuple(r) for r in rows], dtype=ke.LABEL_DTYPE)


def results(rows):
    """rows: label-format lists with the score appended."""
    return np.array([tuple([r[0], -1.0, -1] + list(r[3:])) for r in rows], dtype=ke.RESULT_DTYPE)


def _dontcare(box):
    return ['DontCare', -1, -1, -10] + [float(v) for v in box] + [-1, -1, -1, -1000, -1000, -1000, -10]


# ---------------------------------------------------------------- the crowded split

CROWDED_SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 200, 513, 1000)
CROWDED_DONTCARE = (0, 1, 3, 0, 1, 3, 0, 1, 3, 1, 3)            # don't-care regions of the frame of that size
CROWDED_SEED = 5
NEIGHBOUR = {'Car': 'Van', 'Pedestrian': 'Person_sitting'}


def _crowded_frame(rng, n_det, n_dc):
    types = ['Car', 'Car', 'Car', 'Van', 'Pedestrian', 'Pedestrian', 'Cyclist', 'Person_sitting']
    n_obj = int(rng.integers(8, 13))
    g = []
    for k in range(n_obj):
        # two objects per frame just above a minimum height, so that a box under it still overlaps them by more than 0.7
        height = float(rng.uniform(27, 34)) if k == 0 else float(rng.uniform(42, 55)) if k == 1 else None
        g.append(_round(_row(rng, str(rng.choice(types)) if k > 1 else 'Car', height=height)))
    dcs = []
    for k in range(n_dc):
        if k == 1:                                               # the second region overlaps the first
            x1, y1, x2, y2 = dcs[0][4:8]
            box = [x1 + 0.4 * (x2 - x1), y1 - 20.0, x2 + 0.5 * (x2 - x1), y2 + 10.0]
        else:
            x1, y1 = float(rng.uniform(0, 900)), float(rng.uniform(230, 260))
            box = [x1, y1, x1 + float(rng.uniform(150, 250)), y1 + float(rng.uniform(60, 110))]
        dcs.append(_dontcare([round(v, 2) for v in box]))

    def inside(regions):                                         # a Car box within every region of `regions`
        x1, y1 = max(r[4] for r in regions), max(r[5] for r in regions)
        x2, y2 = min(r[6] for r in regions), min(r[7] for r in regions)
        bx = _row(rng, 'Car')
        u, v = sorted(rng.uniform(0.02, 0.98, 2)), sorted(rng.uniform(0.02, 0.98, 2))
        if (v[1] - v[0]) * (y2 - y1) < 41.0:                     # tall enough to be valid at every difficulty
            v = [0.02, 0.98]
        bx[4:8] = [x1 + u[0] * (x2 - x1), y1 + v[0] * (y2 - y1), x1 + u[1] * (x2 - x1) + 1.0, y1 + v[1] * (y2 - y1)]
        return bx

    n_dup = int(round(0.2 * n_det)) if n_det >= 3 else 0
    d = []
    while len(d) < n_det - n_dup:
        u = rng.random()
        r = g[int(rng.integers(0, n_obj))]
        det_type = {'Van': 'Car' if rng.random() < 0.5 else 'Van', 'Person_sitting': 'Pedestrian'}.get(r[0], r[0])
        if u < 0.40:                                             # jittered copy of a ground truth
            d.append([det_type] + _jitter(rng, r, float(rng.choice([0.15, 0.4, 1.0])))[1:])
        elif u < 0.50:                                           # neighbour-class row
            d.append([NEIGHBOUR.get(det_type, det_type)] + _jitter(rng, r, 0.4)[1:])
        elif u < 0.62:                                           # under a minimum height, still on the ground truth
            c = [det_type] + _jitter(rng, r, 0.15)[1:]
            gh = r[7] - r[5]
            c[7] = c[5] + (24.5 if gh < 40 or rng.random() < 0.3 else 39.5) - float(rng.uniform(0, 0.4))
            d.append(c)
        elif u < 0.77 and dcs:                                   # inside one don't-care region, or inside two at once
            d.append(inside(dcs[:2]) if len(dcs) > 1 and rng.random() < 0.4 else inside([dcs[int(rng.integers(0, len(dcs)))]]))
        else:                                                    # unrelated
            d.append(_row(rng, str(rng.choice(['Car', 'Pedestrian', 'Cyclist']))))
    rows = []
    for r in d:
        sc = float(rng.choice([0.5, 0.75, 0.9])) if rng.random() < 0.34 else round(float(rng.uniform(-0.04, 1.0)), 3)
        rows.append(_round([r[0], -1.0, -1] + list(r[3:]), 4) + [sc])
    for _ in range(n_dup):                                       # exact duplicates of earlier rows, often score and all
        r = list(rows[int(rng.integers(0, len(rows)))])
        if rng.random() > 0.7:
            r[-1] = round(float(rng.uniform(-0.04, 1.0)), 3)
        rows.append(r)
    rows = [rows[k] for k in rng.permutation(len(rows))]
    return labels(g + dcs), np.array([tuple(r) for r in rows], dtype=ke.RESULT_DTYPE)


def _car(k, height=60.0, score=None, **kw):
    """A Car that is easy at every difficulty (height > 40, not occluded, not truncated) in image column k / ground lane k."""
    r = ['Car', 0.0, 0, 0.1, 40.0 + 170.0 * k, 120.0, 140.0 + 170.0 * k, 120.0 + height, 1.5, 1.6, 3.9, -20.0 + 8.0 * k, 1.6, 30.0,
         0.2]
    for name, v in kw.items():
        r[{'alpha': 3, 'y2': 7, 'ry': 14}[name]] = v
    return r if score is None else r + [score]


def _filler(j, score=None):
    """A Car detection that overlaps no _car(k): a false positive wherever it is valid."""
    x1 = float((j * 37) % 1100)
    r = ['Car', 0.0, 0, -0.4, x1, 300.0, x1 + 70.0, 350.0, 1.5, 1.6, 3.9, -40.0 + 0.4 * (j % 200), 1.6, 75.0, -1.0]
    return r + [round(0.05 + 0.0001 * j, 4) if score is None else score]


def _flat(k, shift=0.0, height=60.0, score=None, low=False, px=10.0):
    """_car(k) with ry = 0, l = 4, w = 2, moved by `shift` steps: 10 px in the image and 0.5 m along x on the ground, so that
    every overlap is a ratio of small integers (one step apart: 0.818 in 2-D, 7 / 9 on the ground; three steps: 0.538 and 5 / 11)
    and equal shifts give bit-equal overlaps.  low: 24.5 px high, under every minimum height; on a 30 px ground truth such a box
    needs px = 4 (one step: 0.759, three steps: 0.654) to stay over 0.7 one step away."""
    r = _car(k, height=height, ry=0.0)
    r[4], r[6], r[9], r[10], r[11] = r[4] + px * shift, r[6] + px * shift, 2.0, 4.0, r[11] + 0.5 * shift
    if low:
        r[7] = 144.5
    return r if score is None else r + [score]


TIE_FRAME_THRESHOLDS = [0.9, 0.86, 0.82, 0.72, 0.7, 0.68, 0.66, 0.64, 0.62, 0.6]


def tie_frame():
    """200 detections and 15 ground truths in which every tie has a consequence: the equal rivals differ in their ignore flag
    or in what they leave for the next ground truth, so the wrong one changes the counts.  Index arithmetic is the point.
    V = a copy of the ground truth, I = the same box 24.5 px high (ignored_det == 1; it still overlaps: 0.82 in 2-D, the same
    3-D box).  g0..g5 and g12..g14 are 30 px high (valid at moderate and hard, ignored at easy), the others 60 px.
      pass 1, equal scores (pass 1 takes the first of them whatever its flag; an ignored winner leaves the ground truth no score):
        g0  V@6   I@70   0.90  other chunk of the same lane           -> score 0.90
        g1  I@7   V@135  0.88  the same, flags exchanged              -> no score; pass 2 takes 135
        g2  V@8   I@71   0.86  later chunk of a lower lane            -> score 0.86
        g3  I@10  V@73   0.84                                         -> no score; pass 2 takes 73
        g4  V@11  I@76   0.82  later chunk of a higher lane           -> score 0.82
        g5  I@13  V@79   0.80                                         -> no score; pass 2 takes 79
      pass 2, equal overlaps (p one step left of D1, q one step right, D2 two steps right: q overlaps D2 as well, p does not;
      D1 must take p, the first, or D2 is left with nothing and p becomes a false positive):
        g6, g7    p@14 (0.70)  q@78  (0.68)  other chunk of the same lane
        g8, g9    p@16 (0.66)  q@143 (0.64)  later chunk of a lower lane
        g10, g11  p@17 (0.62)  q@146 (0.60)  later chunk of a higher lane
      ignored candidates:
        g12       I@20, 21, 22 (0.71), V@150 (0.72): the valid one behind the ignored ones -> score 0.72, a true positive
        g13, g14  I@160 one step right of g13 (0.74), I@161, 162 one step left; g14 two steps right: g13 must take 160, the
                  first, which leaves g14 nothing (a miss); had it taken another, g14 would take 160 and not be missed
    Everything else is a valid false positive far away with a score under 0.08, below every threshold.
    The answer at moderate and hard (n_gt = 15; 15 scores or fewer are all kept by get_thresholds): thresholds
    TIE_FRAME_THRESHOLDS; tp 1 (g0), 3 (+g1, g2), 5 (+g3, g4), 7 (+g5, g12), then one more at each threshold (g6 .. g11) up to
    13; fp 0 throughout; fn = 15 - tp, less one from 0.72 on, where g13 holds an ignored detection and is neither.
    At easy (n_gt = 6: g6 .. g11; every 30 px box is ignored): thresholds 0.7 .. 0.6, tp 1 .. 6, fn 5 .. 0, fp 0."""
    g = [_car(k, height=30.0) for k in range(6)]
    g += [_flat(6), _flat(6, 2), _flat(7), _flat(7, 2), _flat(8), _flat(8, 2)]
    g += [_car(9, height=30.0), _flat(10, height=30.0), _flat(10, 2, height=30.0, px=4.0)]
    d = [_filler(j) for j in range(200)]
    for k, (v, i, sc) in enumerate(((6, 70, 0.90), (135, 7, 0.88), (8, 71, 0.86), (73, 10, 0.84), (11, 76, 0.82), (79, 13, 0.80))):
        d[v] = _car(k, height=30.0, score=sc)
        d[i] = _car(k, height=30.0, score=sc, y2=144.5)
    for k, (p, q, sp, sq) in zip((6, 7, 8), ((14, 78, 0.70, 0.68), (16, 143, 0.66, 0.64), (17, 146, 0.62, 0.60))):
        d[p], d[q] = _flat(k, -1, score=sp), _flat(k, 1, score=sq)
    for j in (20, 21, 22):
        d[j] = _car(9, height=30.0, score=0.71, y2=144.5)
    d[150] = _car(9, height=30.0, score=0.72)
    d[160] = _flat(10, 1, height=30.0, score=0.74, low=True, px=4.0)
    d[161] = d[162] = _flat(10, -1, height=30.0, score=0.74, low=True, px=4.0)
    return labels(g), results(d)


def expect_tie_frame(got):
    tp = [1, 3, 5, 7, 8, 9, 10, 11, 12, 13]
    fn = [14, 12, 10, 7, 6, 5, 4, 3, 2, 1]
    for key, m, d, e in entries(got, difficulties=('moderate', 'hard')):
        assert _counts(e) == (15, TIE_FRAME_THRESHOLDS, tp, [0] * 10, fn), (key, m, d, _counts(e))
    for key, m, d, e in entries(got, difficulties=('easy',)):
        assert _counts(e) == (6, TIE_FRAME_THRESHOLDS[4:], [1, 2, 3, 4, 5, 6], [0] * 6, [5, 4, 3, 2, 1, 0]), (key, m, d, _counts(e))


def crowded_split(seed=CROWDED_SEED):
    """(gt_frames, det_frames): one frame per CROWDED_SIZES entry, then tie_frame()."""
    rng = np.random.default_rng(seed)
    gts, dets = [], []
    for n_det, n_dc in zip(CROWDED_SIZES, CROWDED_DONTCARE):
        g, d = _crowded_frame(rng, n_det, n_dc)
        assert len(d) == n_det
        gts.append(g)
        dets.append(d)
    g, d = tie_frame()
    return gts + [g], dets + [d]


def min_overlaps():
    return sorted({v for sets in ke.DEFAULT_OVERLAPS.values() for t in sets for v in t})


def threshold_margin(cache):
    """(distance of the closest overlap to any minimum overlap, number of positive overlaps) over a ref.evaluate cache."""
    vals = []
    for metric in cache:
        for ov, dcov in cache[metric]:
            vals += [v for row in ov for v in row]
            if metric == ref.IMAGE:
                vals += [v for row in dcov for v in row]
    vals = np.array(vals)
    return min(float(np.abs(vals - t).min()) for t in min_overlaps()), int((vals > 0).sum())


# ---------------------------------------------------------------- finding the tie / ignore situations in a split

def trace_matches(det, ignored_gt, ignored_det, compute_fp, ov, min_overlap, thresh=0.0):
    """The ground-truth loop of ref.compute_statistics, copied, which also records for every ground truth the candidates the
    loop could have taken: ([(i, chosen index or -1, [(j, score, overlap, ignored_det)])], {'tp', 'fn', 'v'})."""
    NO = ref.NO_DETECTION
    stat = {'tp': 0, 'fn': 0, 'v': []}
    assigned_detection = [False] * len(det)
    trace = []
    for i in range(len(ignored_gt)):
        if ignored_gt[i] == -1:
            continue
        det_idx, valid_detection, max_iou, assigned_ignored_det = -1, NO, 0.0, False
        cands = []
        for j in range(len(det)):
            if ignored_det[j] == -1:
                continue
            if assigned_detection[j]:
                continue
            if compute_fp and det[j]['score'] < thresh:
                continue
            overlap = ov[i][j]
            if overlap > min_overlap:
                cands.append((j, float(det[j]['score']), overlap, ignored_det[j]))
            if not compute_fp and overlap > min_overlap and det[j]['score'] > valid_detection:
                det_idx = j
                valid_detection = det[j]['score']
            elif compute_fp and overlap > min_overlap and (overlap > max_iou or assigned_ignored_det) and ignored_det[j] == 0:
                max_iou = overlap
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = False
            elif compute_fp and overlap > min_overlap and valid_detection == NO and ignored_det[j] == 1:
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = True
        trace.append((i, det_idx, cands))
        if valid_detection == NO and ignored_gt[i] == 0:
            stat['fn'] += 1
        elif valid_detection != NO and (ignored_gt[i] == 1 or ignored_det[det_idx] == 1):
            assigned_detection[det_idx] = True
        elif valid_detection != NO:
            stat['tp'] += 1
            stat['v'].append(det[det_idx]['score'])
            assigned_detection[det_idx] = True
    return trace, stat


SITUATIONS = ('p1_tie_other_chunk_of_the_same_lane',        # winner 6, equal score at 70
              'p1_tie_later_chunk_of_a_lower_lane',         # winner 8, equal score at 71
              'p1_tie_later_chunk_of_a_higher_lane',        # winner 9, equal score at 74
              'p2_equal_overlaps_in_different_chunks',
              'p2_valid_at_64_or_more_behind_ignored_ones_below_64',
              'p2_all_ignored_and_the_first_at_64_or_more')


def classify(trace, compute_fp, ov, min_overlap):
    """The SITUATIONS that occur in one frame's trace.  A tie counts only if it matters which of the equals is taken: in pass 1
    the rival's ignore flag differs from the winner's (the ground truth gets a score or none); in pass 2, and among ignored
    candidates, the rival and the winner differ in being a candidate of some later ground truth."""
    seen = collections.Counter()

    def differ_later(i, a, b):
        return any((ov[k][a] > min_overlap) != (ov[k][b] > min_overlap) for k in range(i + 1, len(ov)))
    for i, w, cands in trace:
        if w < 0:
            continue
        by_j = {c[0]: c for c in cands}
        if not compute_fp:
            rivals = [j for j, sc, _, ign in cands if j != w and sc == by_j[w][1] and ign != by_j[w][3]]
            assert all(j > w for j in rivals)
            seen[SITUATIONS[0]] += any(j % 64 == w % 64 for j in rivals)
            seen[SITUATIONS[1]] += any(j // 64 > w // 64 and j % 64 < w % 64 for j in rivals)
            seen[SITUATIONS[2]] += any(j // 64 > w // 64 and j % 64 > w % 64 for j in rivals)
        elif by_j[w][3] == 0:
            seen[SITUATIONS[3]] += any(ign == 0 and j // 64 != w // 64 and o == by_j[w][2] and differ_later(i, j, w)
                                       for j, _, o, ign in cands if j != w)
            low = [c for c in cands if c[0] < 64]
            seen[SITUATIONS[4]] += w >= 64 and len(low) > 0 and all(c[3] == 1 for c in low)
        else:
            assert all(c[3] == 1 for c in cands) and w == min(c[0] for c in cands)
            seen[SITUATIONS[5]] += w >= 64 and any(differ_later(i, c[0], w) for c in cands if c[0] != w)
    return seen


def census(gts, dets, cache, check=None):
    """Counter of SITUATIONS over every class, overlap set, metric and difficulty: pass 1, and pass 2 at the lowest threshold.
    check(stat, reference stat) is called with every frame's traced and reference counts."""
    seen = collections.Counter()
    for cls in ref.CLASSES:
        for triple in ref.DEFAULT_OVERLAPS[cls]:
            for metric in (ref.IMAGE, ref.GROUND, ref.BOX3D):
                for diff in range(3):
                    flags = [ref.clean_data(g, d, cls, diff) for g, d in zip(gts, dets)]
                    v = []
                    for f, (ig, idt, dc, n) in enumerate(flags):
                        ov, dcov = cache[metric][f]
                        tr, st = trace_matches(dets[f], ig, idt, False, ov, triple[metric])
                        if check:
                            check(st, ref.compute_statistics(gts[f], dets[f], dc, ig, idt, False, ov, dcov, triple[metric],
                                                             metric, False))
                        seen += classify(tr, False, ov, triple[metric])
                        v += st['v']
                    n_gt = sum(fl[3] for fl in flags)
                    thr = ref.get_thresholds(v, n_gt) if n_gt else []
                    if not thr:
                        continue
                    for f, (ig, idt, dc, n) in enumerate(flags):
                        ov, dcov = cache[metric][f]
                        tr, st = trace_matches(dets[f], ig, idt, True, ov, triple[metric], thr[-1])
                        if check:
                            check(st, ref.compute_statistics(gts[f], dets[f], dc, ig, idt, True, ov, dcov, triple[metric],
                                                             metric, False, thr[-1]))
                        seen += classify(tr, True, ov, triple[metric])
    return seen


# ---------------------------------------------------------------- comparing two results

def assert_same_result(got, want, where=''):
    """Entry for entry: integers and floats equal, the AOS within 1e-12 (its cosine is the device's).  Returns the number of
    thresholds compared."""
    assert list(got) == list(want), where
    n_thr = 0
    for c in want:
        assert list(got[c]) == list(want[c])
        for key in want[c]:
            for m in ('bbox', 'bev', '3d', 'aos'):
                for diff in ref.DIFFICULTIES:
                    w, e = want[c][key][m][diff], got[c][key][m][diff]
                    at = (where, c, key, m, diff)
                    assert e['n_gt'] == w['n_gt'], at
                    if m == 'aos':
                        assert (e['R11'] is None) == (w['R11'] is None), at
                        if w['R11'] is not None:
                            assert abs(e['R11'] - w['R11']) <= 1e-12 and abs(e['R40'] - w['R40']) <= 1e-12, at
                        assert np.abs(np.array(e['precision']) - np.array(w['precision'])).max() <= 1e-12, at
                        continue
                    assert e['thresholds'] == w['thresholds'], at
                    assert (e['tp'], e['fp'], e['fn']) == (w['tp'], w['fp'], w['fn']), at + (e['tp'], e['fp'], e['fn'], w['tp'], w['fp'], w['fn'])
                    assert e['precision'] == w['precision'] and e['R11'] == w['R11'] and e['R40'] == w['R40'], at
                    n_thr += len(w['thresholds'])
    return n_thr


def entries(result, cls='Car', metrics=('bbox', 'bev', '3d'), difficulties=ref.DIFFICULTIES):
    """Every (key, metric, difficulty, entry) of one class of a result."""
    return [(key, m, d, result[cls][key][m][d]) for key in result[cls] for m in metrics for d in difficulties]


# ---------------------------------------------------------------- planted frames whose answers are literals

PLANTED_N = (64, 65, 130, 4096)
BEST_AT = (0, 63, 64, 127, 128, -1)
DELTA_ALPHA = 0.3
SIMILARITY = (1.0 + math.cos(0.1 - (0.1 + DELTA_ALPHA))) / 2.0       # of one matched pair of identical_detections


def identical_detections(n, n_gt=1):
    """n_gt identical easy Cars and n identical valid detections on them with one score (alpha turned by DELTA_ALPHA).
    The answer: every threshold is 0.5 and has tp = n_gt, fp = n - n_gt, fn = 0; AOS precision = n_gt * SIMILARITY / n."""
    return [labels([_car(0)] * n_gt)], [results([_car(0, score=0.5, alpha=0.1 + DELTA_ALPHA)] * n)]


def best_score_at(n, p):
    """One easy Car, n identical detections with distinct scores, the best (0.95) at index p (negative: from the end).
    The answer: thresholds [0.95], tp [1], fp [0], fn [0]."""
    rows = [_car(0, score=round(0.1 + 0.0001 * j, 4)) for j in range(n)]
    rows[p][-1] = 0.95
    return [labels([_car(0)])], [results(rows)]


def ignored_candidates(with_valid):
    """Ground truth A (30 px high: ignored at easy, valid at moderate and hard) and an ordinary easy B.
    with_valid: detections 0..69 lie on A and are under every minimum height (24.5 px: 2-D overlap 24.5 / 30, the same 3-D
    box), score 0.92; 70 is A itself with score 0.95; 71 is B with score 0.9.
    Without: a second ground truth A2 two steps right of A (_flat); detection 0 lies between them and overlaps both, 1..70 lie
    one step left of A and overlap A only, all 71 under the minimum height with score 0.92; 71 is B."""
    if with_valid:
        rows = [_car(0, height=30.0, score=0.92, y2=144.5) for _ in range(70)] + [_car(0, height=30.0, score=0.95)]
        return [labels([_car(0, height=30.0), _car(3)])], [results(rows + [_car(3, score=0.9)])]
    rows = [_flat(0, 1, height=30.0, score=0.92, low=True, px=4.0)]
    rows += [_flat(0, -1, height=30.0, score=0.92, low=True, px=4.0) for _ in range(70)]
    return [labels([_flat(0, height=30.0), _flat(0, 2, height=30.0, px=4.0), _car(3)])], [results(rows + [_car(3, score=0.9)])]


def inside_dontcare(n_regions, n=200):
    """One easy Car matched by its copy (score 0.9) and n valid Car detections (score 0.95) inside n_regions (1 or 2, the two
    overlapping) don't-care regions, on the ground far from the Car.
    The answer: thresholds [0.9], tp [1], fn [0]; fp [0] for bbox, [n] for bev and 3d."""
    dcs = [_dontcare([100.0, 250.0, 500.0, 370.0]), _dontcare([300.0, 240.0, 700.0, 360.0])][:n_regions]
    rows = [_car(0, score=0.9)]
    for j in range(n):
        x1 = 310.0 + (j % 20) * 5.0
        y1 = 255.0 + (j // 20) * 2.0
        rows.append(['Car', 0.0, 0, 0.0, x1, y1, x1 + 80.0, y1 + 70.0, 1.5, 1.6, 3.9, 10.0 + 0.01 * j, 1.6, 70.0, 0.5, 0.95])
    k = n // 2
    rows = rows[1:k] + rows[:1] + rows[k:]                      # the matched detection in the middle, in another chunk
    return [labels([_car(0)] + dcs)], [results(rows)]


def _counts(e):
    return e['n_gt'], e['thresholds'], e['tp'], e['fp'], e['fn']


def expect_identical(got, n):
    for key, m, d, e in entries(got):
        assert _counts(e) == (1, [0.5], [1], [n - 1], [0]), (key, m, d, _counts(e))
    for key, m, d, e in entries(got, metrics=('aos',)):
        assert abs(e['precision'][0] * n - SIMILARITY) <= 1e-12, (key, d)      # the similarity does not depend on n


def expect_best_score(got):
    for key, m, d, e in entries(got):
        assert _counts(e) == (1, [0.95], [1], [0], [0]), (key, m, d, _counts(e))


def expect_stacked(got, n, k):
    """K identical ground truths, n identical detections: the greedy walk assigns K different ones.  An assigned flag in the
    wrong place, or lost, hands a detection out twice or not at all."""
    for key, m, d, e in entries(got):
        nt = len(e['thresholds'])
        assert e['n_gt'] == k and 1 <= nt <= 41 and set(e['thresholds']) == {0.5}
        assert (e['tp'], e['fp'], e['fn']) == ([k] * nt, [n - k] * nt, [0] * nt), (key, m, d, _counts(e))


def expect_valid_behind_ignored(got):
    """ignored_candidates(True), moderate and hard (A and B valid, n_gt = 2).  Pass 1 of compute_statistics does not look at a
    candidate's ignore flag: A takes the best score among 0..70, which is 70 (0.95), B takes 71 (0.9); get_thresholds of
    (0.95, 0.9) over two ground truths keeps both.  At 0.95 only 70 passes the threshold: A is a true positive, B is missed.
    At 0.9 A's loop first takes 0 (ignored, nothing taken yet), passes over 1..69 (valid_detection is set) and then takes
    70, the first candidate with ignored_det == 0: a true positive; 0..69 are under the minimum height, never false positives.
    Easy (A and every box of 30 px or less are ignored, n_gt = 1): B alone, threshold 0.9."""
    for key, m, d, e in entries(got, difficulties=('moderate', 'hard')):
        assert _counts(e) == (2, [0.95, 0.9], [1, 2], [0, 0], [1, 0]), (key, m, d, _counts(e))
    for key, m, d, e in entries(got, difficulties=('easy',)):
        assert _counts(e) == (1, [0.9], [1], [0], [0]), (key, m, d, _counts(e))


def expect_all_ignored(got):
    """ignored_candidates(False), moderate and hard (n_gt = 3).  Pass 1 gives A the candidate 0 (the best score, first of
    equals), which is ignored, so A yields no score; A2's only candidate, 0, is taken: no score either; the only threshold is
    B's 0.9.  There A's loop takes 0, the first ignored candidate (valid_detection is set, so 1..70 are passed over, and no
    valid one follows), and `ignored_det[det_idx] == 1` makes A neither a true positive nor a miss.  A2 finds 0 assigned and
    1..70 out of reach: the one miss -- which is what tells the lowest index from any other ignored candidate.  B is the true
    positive.  No ignored row is false.  Easy: A and A2 are ignored, B alone."""
    for key, m, d, e in entries(got, difficulties=('moderate', 'hard')):
        assert _counts(e) == (3, [0.9], [1], [0], [1]), (key, m, d, _counts(e))
    for key, m, d, e in entries(got, difficulties=('easy',)):
        assert _counts(e) == (1, [0.9], [1], [0], [0]), (key, m, d, _counts(e))


def expect_inside_dontcare(got, n=200):
    for key, m, d, e in entries(got):
        assert _counts(e) == (1, [0.9], [1], [0 if m == 'bbox' else n], [0]), (key, m, d, _counts(e))


# ---------------------------------------------------------------- near-degenerate BEV pairs and their exact overlaps

SWEEP_KINDS = ('same', 'yaw_eps', 'quarter_turns_eps', 'one_length_along', 'one_width_across', 'scaled')
SWEEP_PER_FRAME = 200
SWEEP_FRAMES = {'near': 85, 'far': 15}                          # 20 000 planted pairs
SWEEP_SEED = 23


def _sweep_pair(rng, band):
    type_ = str(rng.choice(['Car', 'Van', 'Pedestrian', 'Cyclist']))
    g = _row(rng, type_)
    g[11] = float(rng.uniform(-30, 30))
    g[13] = float(rng.uniform(5, 80)) if band == 'near' else float(rng.uniform(480, 520))
    d = list(g)
    d[12] += float(rng.choice([0.0, 0.05, -0.2]))               # the 3-D overlap differs from the BEV one
    kind = SWEEP_KINDS[int(rng.integers(0, len(SWEEP_KINDS)))]
    eps = float(10.0 ** rng.uniform(-16, -3)) * float(rng.choice([-1.0, 1.0]))
    l, w, ry = g[10], g[9], g[14]
    c, s = math.cos(ry), math.sin(ry)
    if kind == 'same':
        d[12] = g[12]
    elif kind == 'yaw_eps':
        d[14] = ry + eps
    elif kind == 'quarter_turns_eps':
        d[14] = ry + int(rng.integers(1, 4)) * (math.pi / 2) + eps
    elif kind == 'one_length_along':                             # the length axis of footprint() is (cos ry, -sin ry)
        d[11], d[13] = g[11] + (l + eps) * c, g[13] - (l + eps) * s
    elif kind == 'one_width_across':                             # the width axis is (sin ry, cos ry): a shared long edge
        d[11], d[13] = g[11] + w * s, g[13] + w * c
        d[14] = ry + eps * float(rng.choice([0.0, 1.0]))
    else:
        d[10], d[9] = l * (1.0 + eps), w * (1.0 + eps * float(rng.choice([1.0, -1.0, 0.5])))
    return g, d, kind


def bev_sweep(seed=SWEEP_SEED):
    """[(band, gt frame, det frame, kinds)]: SWEEP_PER_FRAME ground truths and as many detections per frame, detection k built
    from ground truth k by a perturbation of size 10**uniform(-16, -3) of kind kinds[k]."""
    rng = np.random.default_rng(seed)
    out = []
    for band in ('near', 'far'):
        for _ in range(SWEEP_FRAMES[band]):
            pairs = [_sweep_pair(rng, band) for _ in range(SWEEP_PER_FRAME)]
            out.append((band, labels([p[0] for p in pairs]), np.array([tuple(p[1]) + (0.5,) for p in pairs], dtype=ke.RESULT_DTYPE),
                        [p[2] for p in pairs]))
    return out


def swapped(g, d):
    """The frame with the roles exchanged: the detections as labels, the labels as detections."""
    names = ke.LABEL_DTYPE.names
    g2 = np.array([tuple(r[n] for n in names) for r in d], dtype=ke.LABEL_DTYPE)
    d2 = np.array([tuple(r[n] for n in names) + (0.5,) for r in g], dtype=ke.RESULT_DTYPE)
    return g2, d2


def _near(g_frame, d_frame):
    """(n_gt, n_det) bool: False only where the two footprints are certainly disjoint -- the centres are further apart than the
    two half diagonals plus a margin that dwarfs every rounding in this test (1e-6 m)."""
    r = (np.hypot(g_frame['l'], g_frame['w'])[:, None] + np.hypot(d_frame['l'], d_frame['w'])[None, :]) / 2.0
    dist = np.hypot(g_frame['x'][:, None] - d_frame['x'][None, :], g_frame['z'][:, None] - d_frame['z'][None, :])
    return dist <= r + 1e-6


def exact_overlaps(g_frame, d_frame, also_float=False):
    """(bev, 3d) matrices (n_gt, n_det) from ref.bev_intersection_exact; pairs that are certainly disjoint are 0 without the
    rational arithmetic.  also_float: the same two from the float reference for the pairs that are not, elsewhere 0."""
    out = np.zeros((4 if also_float else 2, len(g_frame), len(d_frame)))
    for i, j in zip(*np.nonzero(_near(g_frame, d_frame))):
        d, g = d_frame[j], g_frame[i]
        out[0, i, j], out[1, i, j] = ref.ground_and_box3d_overlap(d, g, ref.bev_intersection_exact)
        if also_float:
            out[2, i, j], out[3, i, j] = ref.ground_and_box3d_overlap(d, g)
    return out
