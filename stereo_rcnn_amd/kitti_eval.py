"""KITTI object evaluation: AP_2d (bbox), AOS, AP_bev and AP_3d at Easy / Moderate / Hard, from the label files and the
result files `test_net` writes -- the published algorithm of the KITTI object devkit (`evaluate_object_3d_offline`),
restated, with the matching on the MI355X (stereo_rcnn_amd/csrc/kitti_eval.hip).

    python -m stereo_rcnn_amd.kitti_eval --label-dir <.../training/label_2> --result-dir out [--split val.txt]
                                         [--json ap.json] [--overlaps car=0.7,0.5,0.5 ...]
    python -m stereo_rcnn_amd.run_kitti --label-dir <.../label_2> <test_net arguments>    # the split, then this table

What runs where:
  * host (numpy): parsing, cleanData's ignore flags, getThresholds and the AP sums -- cheap and sequential;
  * device: every det x gt overlap of the split (2-D, BEV, 3-D) and every det x don't-care overlap in one launch, then the
    greedy per-frame match of computeStatistics in two launches (pass 1 collects the true positives' scores, pass 2 counts
    tp / fp / fn and the AOS similarity at up to 41 score thresholds), one wavefront per (class, difficulty, metric,
    overlap set, threshold, frame).  There is no CPU fallback.

Rules (cumulative difficulties, ignored neighbour classes Van / Person_sitting, don't-care regions for the 2-D metric only,
strict `overlap > MIN_OVERLAP`) follow the devkit; the docstrings of the functions below say where.  Two choices the
devkit leaves open: a threshold at which tp + fp == 0 gives precision 0 (the devkit divides by zero), and without a split
list the frames are the result files that exist, which is believed to be what the offline devkit does but has not been
checked against its source.  AP_R11 is the devkit's 11-point average, AP_R40 the 40-point one of the updated devkit.
"""
import argparse
import json
import os
import time

import numpy as np

from ._lib import KITTI_COLS, KITTI_MAX_DET as MAX_DET_PER_FRAME     # the library's row width and per-frame limit

CLASSES = ('Car', 'Pedestrian', 'Cyclist')
NEIGHBOUR = {'car': 'van', 'pedestrian': 'person_sitting'}         # counted as ignored, not as false
DIFFICULTIES = ('easy', 'moderate', 'hard')
MIN_HEIGHT = (40.0, 25.0, 25.0)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.30, 0.50)
METRICS = ('bbox', 'bev', '3d')                                     # device metric ids 0 / 1 / 2; 'aos' rides on 'bbox'
DEFAULT_OVERLAPS = {'Car': ((0.7, 0.7, 0.7), (0.7, 0.5, 0.5)),
                    'Pedestrian': ((0.5, 0.5, 0.5), (0.5, 0.25, 0.25)),
                    'Cyclist': ((0.5, 0.5, 0.5), (0.5, 0.25, 0.25))}
N_SAMPLE_PTS = 41

LABEL_DTYPE = np.dtype([('type', 'U32'), ('truncated', 'f8'), ('occluded', 'i4')] +
                       [(f, 'f8') for f in ('alpha', 'x1', 'y1', 'x2', 'y2', 'h', 'w', 'l', 'x', 'y', 'z', 'ry')])
RESULT_DTYPE = np.dtype(LABEL_DTYPE.descr + [('score', 'f8')])
# device row: [x1 y1 x2 y2 h w l x y z ry alpha score] (KITTI_COLS of them)
_ROW = ('x1', 'y1', 'x2', 'y2', 'h', 'w', 'l', 'x', 'y', 'z', 'ry', 'alpha')


def _read(path, dtype, n_fields):
    rows = []
    with open(path) as fh:
        for ln in fh:
            p = ln.split()
            if not p:
                continue
            if len(p) < n_fields:
                raise ValueError('%s: %d fields, expected %d: %r' % (path, len(p), n_fields, ln))
            rows.append((p[0], float(p[1]), int(float(p[2]))) + tuple(float(v) for v in p[3:n_fields]))
    return np.array(rows, dtype=dtype)


def read_label(path):
    """A KITTI label file -> structured array (LABEL_DTYPE): `type trunc occ alpha x1 y1 x2 y2 h w l x y z ry`."""
    return _read(path, LABEL_DTYPE, 15)


def read_result(path):
    """A KITTI result file (the label fields + `score`, as kitti_utils.write_detection_results writes) -> RESULT_DTYPE."""
    return _read(path, RESULT_DTYPE, 16)


def _result_root(result_dir):
    data = os.path.join(result_dir, 'data')
    return data if os.path.isdir(data) else result_dir


def load_split(label_dir, result_dir, ids=None):
    """(ids, gt_frames, det_frames).  Results are read from `<result_dir>/data` or, if that does not exist, `<result_dir>`.
    With `ids` the frames are exactly those ids, and a frame without a result file has no detections; without, the frames
    are the result files that exist (sorted)."""
    root = _result_root(result_dir)
    if ids is None:
        ids = sorted(f[:-4] for f in os.listdir(root) if f.endswith('.txt'))
    ids = list(ids)
    gts, dets = [], []
    for i in ids:
        gts.append(read_label(os.path.join(label_dir, i + '.txt')))
        p = os.path.join(root, i + '.txt')
        dets.append(read_result(p) if os.path.exists(p) else np.zeros(0, RESULT_DTYPE))
    return ids, gts, dets


def get_thresholds(v, n_gt):
    """getThresholds: the scores at which recall passes the 41 sample points (v: the true positives' scores of pass 1)."""
    v = sorted((float(s) for s in v), reverse=True)
    t, current_recall = [], 0.0
    for i in range(len(v)):
        l_recall = (i + 1) / float(n_gt)
        r_recall = (i + 2) / float(n_gt) if i < len(v) - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < len(v) - 1:
            continue
        t.append(v[i])
        current_recall += 1.0 / (N_SAMPLE_PTS - 1.0)
    return t


def average_precision(precision, n_gt):
    """{'R11', 'R40', 'precision', 'n_gt'} of a 41-point precision (or AOS) array: the suffix maximum p[i] = max(p[i:]), then
    AP_R11 = 100/11 * sum(p[0, 4, ..., 40]) and AP_R40 = 100/40 * sum(p[1..40]); both None when n_gt == 0."""
    p = [float(x) for x in np.maximum.accumulate(np.asarray(precision, np.float64)[::-1])[::-1]]
    assert len(p) == N_SAMPLE_PTS
    r11 = sum(p[i] for i in range(0, N_SAMPLE_PTS, 4)) / 11.0 * 100.0
    r40 = sum(p[i] for i in range(1, N_SAMPLE_PTS)) / 40.0 * 100.0
    return {'R11': r11 if n_gt > 0 else None, 'R40': r40 if n_gt > 0 else None, 'precision': p, 'n_gt': int(n_gt)}


def clean_flags(types, truncated, occluded, height, det_types, det_height, cls, difficulty):
    """cleanData for one class and difficulty over flat arrays: (ignored_gt, ignored_det, n_gt), the flags int8 in {0, 1, -1}.
    types / det_types: lower-case class names; height: the 2-D box height of each row."""
    c = cls.lower()
    valid = np.where(types == c, 1, np.where(types == NEIGHBOUR.get(c, '\0'), 0, -1))
    ignore = ((occluded > MAX_OCCLUSION[difficulty]) | (truncated > MAX_TRUNCATION[difficulty]) |
              (height <= MIN_HEIGHT[difficulty]))
    ign_gt = np.where((valid == 1) & ~ignore, 0, np.where((valid == 0) | ((valid == 1) & ignore), 1, -1)).astype(np.int8)
    ign_det = np.where(det_height < MIN_HEIGHT[difficulty], 1, np.where(det_types == c, 0, -1)).astype(np.int8)
    return ign_gt, ign_det, int((ign_gt == 0).sum())


def overlap_key(triple):
    return ', '.join('%.2f' % v for v in triple)


def _canonical(cls):
    for c in CLASSES:
        if c.lower() == cls.lower():
            return c
    raise ValueError('unknown class %r (evaluated: %s)' % (cls, ', '.join(CLASSES)))


class _Flat(object):
    """The split as flat host arrays and per-frame offsets (DontCare rows split off into the don't-care list)."""

    def __init__(self, gt_frames, det_frames):
        if len(gt_frames) != len(det_frames):
            raise ValueError('%d ground-truth frames, %d detection frames' % (len(gt_frames), len(det_frames)))
        nf = len(gt_frames)
        gts, dcs, dets = [], [], []
        self.gt_off, self.dc_off, self.det_off = (np.zeros(nf + 1, np.int64) for _ in range(3))
        for f, (g, d) in enumerate(zip(gt_frames, det_frames)):
            lower = np.char.lower(g['type'].astype(str)) if len(g) else np.zeros(0, 'U1')
            dc = lower == 'dontcare'
            gts.append(g[~dc])
            dcs.append(g[dc])
            dets.append(d)
            self.gt_off[f + 1] = self.gt_off[f] + int((~dc).sum())
            self.dc_off[f + 1] = self.dc_off[f] + int(dc.sum())
            self.det_off[f + 1] = self.det_off[f] + len(d)
        self.gt = np.concatenate(gts) if nf else np.zeros(0, LABEL_DTYPE)
        self.dc = np.concatenate(dcs) if nf else np.zeros(0, LABEL_DTYPE)
        self.det = np.concatenate(dets).astype(RESULT_DTYPE) if nf else np.zeros(0, RESULT_DTYPE)
        self.n_frames = nf
        nd, ng, nc = np.diff(self.det_off), np.diff(self.gt_off), np.diff(self.dc_off)
        self.pair_off = np.concatenate([[0], np.cumsum(nd * ng)]).astype(np.int64)
        self.dcpair_off = np.concatenate([[0], np.cumsum(nd * nc)]).astype(np.int64)
        self.max_det = int(nd.max()) if nf else 0
        self.gt_types = np.char.lower(self.gt['type'].astype(str))
        self.det_types = np.char.lower(self.det['type'].astype(str))
        self.gt_height = np.abs(self.gt['y1'] - self.gt['y2'])
        self.det_height = self.det['y2'] - self.det['y1']

    @staticmethod
    def rows(a, with_score):
        out = np.zeros((len(a), KITTI_COLS), np.float64)
        for k, name in enumerate(_ROW):
            out[:, k] = a[name]
        if with_score:
            out[:, 12] = a['score']
        return out


def _device_overlaps(fl, dev):
    """Uploads the split and launches srcnn_kitti_overlaps: (srcnn_kitti_split, [tensors it points at]); the overlap
    matrices are the last four tensors (image, BEV, 3-D, don't-care)."""
    import ctypes
    import torch
    from . import _lib

    def dt(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)

    rows = [dt(_Flat.rows(a, a is fl.det), np.float64) if len(a) else torch.zeros(KITTI_COLS, dtype=torch.float64, device=dev)
            for a in (fl.det, fl.gt, fl.dc)]
    offs = [dt(a, np.int32) for a in (fl.det_off, fl.gt_off, fl.dc_off)] + [dt(a, np.int64) for a in (fl.pair_off, fl.dcpair_off)]
    npair, ndc = int(fl.pair_off[-1]), int(fl.dcpair_off[-1])
    ovs = [torch.empty(max(npair, 1), dtype=torch.float64, device=dev) for _ in range(3)] + \
        [torch.empty(max(ndc, 1), dtype=torch.float64, device=dev)]
    split = _lib.KittiSplit(fl.n_frames, fl.max_det, *[o.data_ptr() for o in offs], *[r.data_ptr() for r in rows],
                            *[o.data_ptr() for o in ovs])
    _lib.check(_lib.lib().srcnn_kitti_overlaps(ctypes.byref(split), torch.cuda.current_stream(dev).cuda_stream),
               'srcnn_kitti_overlaps')
    return split, rows + offs + ovs


def overlaps(gt_frames, det_frames, device=None):
    """The device overlaps of a split, per frame: {'bbox', 'bev', '3d': (n_gt, n_det), 'dontcare': (n_dontcare, n_det)}
    float64 arrays, ground truth without its DontCare rows (in file order), detection j in column j."""
    import torch
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    fl = _Flat(gt_frames, det_frames)
    with torch.cuda.device(dev):
        _, keep = _device_overlaps(fl, dev)
        ov = [t.cpu().numpy() for t in keep[-4:]]
    out = []
    for f in range(fl.n_frames):
        nd, ng, nc = (int(o[f + 1] - o[f]) for o in (fl.det_off, fl.gt_off, fl.dc_off))
        a, b = int(fl.pair_off[f]), int(fl.dcpair_off[f])
        e = {name: ov[k][a:a + ng * nd].reshape(ng, nd) for k, name in enumerate(METRICS)}
        e['dontcare'] = ov[3][b:b + nc * nd].reshape(nc, nd)
        out.append(e)
    return out


def evaluate(gt_frames, det_frames, classes=None, overlap_sets=None, device=None):
    """The KITTI AP table of a split.
    gt_frames / det_frames: per frame, read_label / read_result arrays (in split order; DontCare rows stay in the labels).
    classes: the classes to evaluate (default Car, Pedestrian, Cyclist); as in the devkit, a class is evaluated only if at
    least one detection of it exists.  overlap_sets: {class: [(image, bev, 3d), ...]} replacing DEFAULT_OVERLAPS per class.
    device: a CUDA device (default: the current one).
    Returns {class: {overlap key: {metric: {difficulty: entry}}}} with the overlap key '0.70, 0.50, 0.50', the metrics
    'bbox', 'aos', 'bev', '3d' and the difficulties 'easy', 'moderate', 'hard'; an entry holds 'R11', 'R40' (None when the
    difficulty has no ground truth), 'precision' (41 points after the suffix maximum; the AOS ratio for 'aos'), 'n_gt', and
    for the AP metrics the 'thresholds' and the per-threshold 'tp', 'fp', 'fn' summed over the split."""
    import ctypes
    import torch
    from . import _lib
    L = _lib.lib()
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    fl = _Flat(gt_frames, det_frames)
    # a frame over MAX_DET_PER_FRAME detections is refused by the library (SRCNN_ERR_ARG -> RuntimeError), never truncated
    sets = {c: [tuple(float(v) for v in t) for t in DEFAULT_OVERLAPS[c]] for c in CLASSES}
    for c, lst in (overlap_sets or {}).items():
        sets[_canonical(c)] = [tuple(float(v) for v in t) for t in lst]
    wanted = [_canonical(c) for c in (classes or CLASSES)]
    evaluated = [c for c in wanted if (fl.det_types == c.lower()).any()]

    # cleanData: one flag set per (class, difficulty)
    ign_gt, ign_det, n_gt = [], [], {}
    for k, c in enumerate(evaluated):
        for d in range(3):
            g, dd, n = clean_flags(fl.gt_types, fl.gt['truncated'], fl.gt['occluded'], fl.gt_height, fl.det_types,
                                   fl.det_height, c, d)
            ign_gt.append(g)
            ign_det.append(dd)
            n_gt[(c, d)] = n
    cfgs = []                                   # (class, set index, metric, difficulty)
    for k, c in enumerate(evaluated):
        for s, triple in enumerate(sets[c]):
            for m in range(3):
                for d in range(3):
                    cfgs.append((c, s, m, d, k * 3 + d, triple[m]))
    result = {c: {overlap_key(t): {} for t in sets[c]} for c in evaluated}
    if not cfgs:
        return result

    def dt(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)

    ng_total, nd_total = len(fl.gt), len(fl.det)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        split, keep = _device_overlaps(fl, dev)                 # keep: the tensors the descriptors point at

        n_cfg = len(cfgs)
        t_flags = dt([c[4] for c in cfgs], np.int32)
        t_metric = dt([c[2] for c in cfgs], np.int32)
        t_minov = dt([c[5] for c in cfgs], np.float64)
        t_igt = dt(np.stack(ign_gt) if ng_total else np.zeros((len(ign_gt), 1)), np.int8)
        t_idet = dt(np.stack(ign_det) if nd_total else np.zeros((len(ign_det), 1)), np.int8)
        gt_score = torch.empty((n_cfg, max(ng_total, 1)), dtype=torch.float64, device=dev)
        keep += [t_flags, t_metric, t_minov, t_igt, t_idet, gt_score]
        m1 = _lib.KittiMatchDesc(n_cfg, 1, 0, ng_total, nd_total, t_flags.data_ptr(), t_metric.data_ptr(), t_minov.data_ptr(),
                                 None, None, t_igt.data_ptr(), t_idet.data_ptr(), gt_score.data_ptr(), None, None, None, None)
        _lib.check(L.srcnn_kitti_match(ctypes.byref(split), ctypes.byref(m1), st), 'srcnn_kitti_match (pass 1)')
        scores = gt_score.cpu().numpy()[:, :ng_total]

        # getThresholds per configuration, on the host between the passes
        thresholds = np.zeros((n_cfg, N_SAMPLE_PTS), np.float64)
        n_thresh = np.zeros(n_cfg, np.int32)
        cfg_thr = []
        for i, (c, s, m, d, _, _) in enumerate(cfgs):
            n = n_gt[(c, d)]
            t = get_thresholds(scores[i][scores[i] != -np.inf], n) if n > 0 else []
            assert len(t) <= N_SAMPLE_PTS
            thresholds[i, :len(t)] = t
            n_thresh[i] = len(t)
            cfg_thr.append(t)
        t_thr, t_nthr = dt(thresholds, np.float64), dt(n_thresh, np.int32)
        shape = (n_cfg, N_SAMPLE_PTS, max(fl.n_frames, 1))
        tp, fp, fn = (torch.empty(shape, dtype=torch.int32, device=dev) for _ in range(3))
        sim = torch.empty(shape, dtype=torch.float64, device=dev)
        keep += [t_thr, t_nthr, tp, fp, fn, sim]
        m2 = _lib.KittiMatchDesc(n_cfg, N_SAMPLE_PTS, 1, ng_total, nd_total, t_flags.data_ptr(), t_metric.data_ptr(),
                                 t_minov.data_ptr(), t_nthr.data_ptr(), t_thr.data_ptr(), t_igt.data_ptr(), t_idet.data_ptr(),
                                 None, tp.data_ptr(), fp.data_ptr(), fn.data_ptr(), sim.data_ptr())
        _lib.check(L.srcnn_kitti_match(ctypes.byref(split), ctypes.byref(m2), st), 'srcnn_kitti_match (pass 2)')
        tp, fp, fn, sim = (x.cpu().numpy()[:, :, :fl.n_frames] for x in (tp, fp, fn, sim))

    tp_s, fp_s, fn_s = (x.sum(axis=2, dtype=np.int64) for x in (tp, fp, fn))
    sim_s = np.zeros((n_cfg, N_SAMPLE_PTS), np.float64)
    for f in range(fl.n_frames):                # frame by frame in split order; a frame with tp + fp == 0 adds nothing
        col = sim[:, :, f]
        sim_s += np.where(col == -1.0, 0.0, col)
    for i, (c, s, m, d, _, _) in enumerate(cfgs):
        key, dname, n = overlap_key(sets[c][s]), DIFFICULTIES[d], n_gt[(c, d)]
        nt = int(n_thresh[i])
        prec, aos = np.zeros(N_SAMPLE_PTS), np.zeros(N_SAMPLE_PTS)
        for t in range(nt):
            den = tp_s[i, t] + fp_s[i, t]
            prec[t] = tp_s[i, t] / float(den) if den > 0 else 0.0
            aos[t] = sim_s[i, t] / float(den) if den > 0 else 0.0
        entries = [(METRICS[m], prec)] + ([('aos', aos)] if m == 0 else [])
        for name, arr in entries:
            e = average_precision(arr, n)
            if name != 'aos':
                e.update(thresholds=[float(v) for v in cfg_thr[i]], tp=[int(v) for v in tp_s[i, :nt]],
                         fp=[int(v) for v in fp_s[i, :nt]], fn=[int(v) for v in fn_s[i, :nt]])
            result[c][key].setdefault(name, {})[dname] = e
    for c in result:                            # metric order of the devkit's printout
        for key in result[c]:
            result[c][key] = {name: result[c][key][name] for name in ('bbox', 'bev', '3d', 'aos')}
    return result


def format_table(result):
    """Devkit-style lines: `Car AP@0.70, 0.70, 0.70:` then the bbox / bev / 3d / aos rows, easy, moderate, hard."""
    def fmt(v):
        return '   n/a ' if v is None else '%7.4f' % v
    lines = []
    for c, by_set in result.items():
        for key, by_metric in by_set.items():
            lines.append('%s AP@%s:' % (c, key))
            for name, by_diff in by_metric.items():
                for label in ('R11', 'R40'):
                    lines.append('%-4s AP(%s): %s' % (name, label, ', '.join(fmt(by_diff[d][label]) for d in DIFFICULTIES)))
    return '\n'.join(lines)


def parse_overlaps(items):
    """['car=0.7,0.5,0.5', 'car=0.7,0.7,0.7', ...] -> {'Car': [(0.7, 0.5, 0.5), (0.7, 0.7, 0.7)]}."""
    out = {}
    for it in items or []:
        name, _, vals = it.partition('=')
        t = tuple(float(v) for v in vals.split(','))
        if len(t) != 3:
            raise ValueError('--overlaps %s: three values (image, bev, 3d) expected' % it)
        out.setdefault(_canonical(name), []).append(t)
    return out


def read_ids(path):
    with open(path) as fh:
        return [ln.strip() for ln in fh if ln.strip()]


def evaluate_split(label_dir, result_dir, ids, device=None, log=print):
    """The AP table of a split's result files over exactly `ids` (a frame without a result file has no detections): logs the
    table and writes <result_dir>/ap.json.  Returns the result dict."""
    t0 = time.perf_counter()
    ids, gts, dets = load_split(label_dir, result_dir, ids)
    res = evaluate(gts, dets, device=device)
    log(format_table(res))
    path = os.path.join(result_dir, 'ap.json')
    with open(path, 'w') as fh:
        json.dump(res, fh, indent=1)
    log('KITTI evaluation of %d frames: %.2f s -> %s' % (len(ids), time.perf_counter() - t0, path))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--label-dir', required=True, help='KITTI label_2 directory (<id>.txt)')
    ap.add_argument('--result-dir', required=True, help='result directory (<dir>/data/<id>.txt, or <dir>/<id>.txt)')
    ap.add_argument('--split', help='text file with one frame id per line (default: the result files that exist)')
    ap.add_argument('--json', help='write the result dict here')
    ap.add_argument('--overlaps', nargs='+', metavar='CLASS=IMG,BEV,3D',
                    help="minimum overlaps replacing a class's defaults (repeat a class for several sets)")
    ap.add_argument('--device', default=None, help='CUDA device (default: the current one)')
    args = ap.parse_args(argv)
    t0 = time.perf_counter()
    ids = read_ids(args.split) if args.split else None
    ids, gts, dets = load_split(args.label_dir, args.result_dir, ids)
    t1 = time.perf_counter()
    res = evaluate(gts, dets, overlap_sets=parse_overlaps(args.overlaps), device=args.device)
    t2 = time.perf_counter()
    print(format_table(res))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)
    print('%d frames: %.2f s (parse %.2f s, evaluate %.2f s)' % (len(ids), t2 - t0, t1 - t0, t2 - t1), flush=True)
    return res


if __name__ == '__main__':
    main()
