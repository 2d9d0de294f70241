"""Generates tests/golden/reference_loader.npz by running the REFERENCE's own data path -- datasets.kitti / datasets.imdb,
roi_data_layer.roidb / minibatch / roibatchLoader, model.utils.kitti_utils / blob -- on a synthetic KITTI-style dataset, under
reference_shims.install(...).  Runs where the reference is present only; the tests read the .npz.

Added in memory for these modules (nothing of the reference is edited or copied):
  * `cPickle` -> pickle; `scipy.misc.imread` -> PIL (RGB); `cv2.imread` -> PIL (BGR); `cv2.resize` ->
    oracle.preprocess.cv2_resize_linear_f32 and `cv2.INTER_LINEAR`: the image side is pinned to the project's OpenCV restatement,
    as everywhere else here, the annotation, flip, ground-truth and shuffle sides are the reference's code;
  * the working directory is a temporary one that holds data/kitti/splits/train.txt (no trailing newline: kitti.py:111 splits on
    '\\n') and data/kitti/object/training/{image_2,image_3,label_2,calib};
  * roibatchLoader's `np` is a proxy whose random.shuffle also shuffles an index column from the same generator state, so the
    permutation is recorded.
The file holds data only: label / calibration texts and image shapes, hand-built roidb entries, small uint8 images, and every
array the reference produced from them.
"""
import os
import pickle
import sys
import tempfile
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
warnings.filterwarnings('ignore')

import numpy as np   # noqa: E402
from PIL import Image  # noqa: E402

from oracle import ops as oracle_ops          # noqa: E402
from oracle import preprocess as oracle_pre   # noqa: E402
import reference_shims                        # noqa: E402

reference_shims.install(oracle_ops)


def _imread_rgb(path):
    with Image.open(path) as im:
        return np.array(im.convert('RGB'), dtype=np.uint8)


def install_loader_shims():
    sys.modules['cPickle'] = pickle
    cv2 = sys.modules['cv2']
    cv2.INTER_LINEAR = 1
    cv2.imread = lambda path: np.ascontiguousarray(_imread_rgb(path)[:, :, ::-1])
    cv2.resize = lambda img, dsize, dst=None, fx=None, fy=None, interpolation=None: oracle_pre.cv2_resize_linear_f32(img, fx, fy)
    misc = types.ModuleType('scipy.misc')
    misc.imread = _imread_rgb
    sys.modules['scipy.misc'] = misc


install_loader_shims()

CALIB = """P0: 7.215377000000e+02 0.000000000000e+00 6.095593000000e+02 0.000000000000e+00 0.000000000000e+00 7.215377000000e+02 1.728540000000e+02 0.000000000000e+00 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 0.000000000000e+00
P1: 7.215377000000e+02 0.000000000000e+00 6.095593000000e+02 -3.875744000000e+02 0.000000000000e+00 7.215377000000e+02 1.728540000000e+02 0.000000000000e+00 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 0.000000000000e+00
P2: 7.215377000000e+02 0.000000000000e+00 6.095593000000e+02 4.485728000000e+01 0.000000000000e+00 7.215377000000e+02 1.728540000000e+02 2.163791000000e-01 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 2.745884000000e-03
P3: 7.215377000000e+02 0.000000000000e+00 6.095593000000e+02 -3.395242000000e+02 0.000000000000e+00 7.215377000000e+02 1.728540000000e+02 2.199936000000e+00 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 2.729905000000e-03
R0_rect: 9.999239000000e-01 9.837760000000e-03 -7.445048000000e-03 -9.869795000000e-03 9.999421000000e-01 -4.278459000000e-03 7.402527000000e-03 4.351614000000e-03 9.999631000000e-01
Tr_velo_to_cam: 7.533745000000e-03 -9.999714000000e-01 -6.166020000000e-04 -4.069766000000e-03 1.480249000000e-02 7.280733000000e-04 -9.998902000000e-01 -7.631618000000e-02 9.998621000000e-01 7.523790000000e-03 1.480755000000e-02 -2.717806000000e-01
Tr_imu_to_velo: 9.999976000000e-01 7.553071000000e-04 -2.035826000000e-03 -8.086759000000e-01 -7.854027000000e-04 9.998898000000e-01 -1.482298000000e-02 3.195559000000e-01 2.024406000000e-03 1.482454000000e-02 9.998881000000e-01 -7.997231000000e-01
"""
# the same rig with another focal length and principal point (the 370 x 1224 sequences)
CALIB_B = CALIB.replace('7.215377000000e+02', '7.070493000000e+02').replace('6.095593000000e+02', '6.040814000000e+02') \
               .replace('1.728540000000e+02', '1.805066000000e+02').replace('4.485728000000e+01', '4.575831000000e+01') \
               .replace('-3.395242000000e+02', '-3.341081000000e+02')


def obj(cls, trunc, occ, alpha, h, w, l, x, y, z, ry, box=(0, 0, 50, 50)):
    """One label line (the 2-D box columns are not read by read_obj_data)."""
    return '%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f' % (
        (cls, trunc, occ, alpha) + tuple(box) + (h, w, l, x, y, z, ry))


DONTCARE = 'DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10'
PEDESTRIAN = 'Pedestrian 0.00 0 -0.20 712.40 143.00 810.73 307.92 1.89 0.48 1.20 1.84 1.47 8.41 0.01'

FRAMES = [
    # 0: plain cars on both sides of the axis, alpha of both signs; a Van (used class, not a Car), a pedestrian, a DontCare
    ('000000', (375, 1242), CALIB, [
        obj('Car', 0.00, 0, -1.58, 1.52, 1.63, 3.88, -3.20, 1.62, 17.50, -1.76),
        obj('Car', 0.00, 1, 1.85, 1.47, 1.60, 4.12, 4.62, 1.71, 24.30, 2.04),
        obj('Van', 0.00, 0, -1.40, 2.20, 1.90, 5.10, -8.10, 1.80, 30.20, -1.66),
        obj('Car', 0.00, 0, 0.40, 1.55, 1.67, 3.64, 9.30, 1.58, 21.00, 0.81),
        PEDESTRIAN, DONTCARE]),
    # 1: each clause of the object filter: truncated, occlusion 3, 10 rows or less; one car stays
    ('000001', (370, 1224), CALIB_B, [
        obj('Car', 0.99, 0, -1.20, 1.50, 1.62, 3.90, -6.50, 1.65, 9.00, -1.80),
        obj('Car', 0.00, 3, 1.60, 1.48, 1.58, 3.70, 6.00, 1.60, 26.00, 1.83),
        obj('Car', 0.00, 0, -1.57, 1.00, 1.55, 3.50, -1.00, 1.62, 80.00, -1.58),
        obj('Car', 0.00, 0, -1.70, 1.51, 1.66, 4.05, 2.10, 1.66, 14.20, -1.55),
        DONTCARE]),
    # 2: a near car, one fully hidden behind it (removed), one partly hidden behind it (shortened range, keypoints lost)
    ('000002', (374, 1238), CALIB, [
        obj('Car', 0.00, 0, -1.57, 1.60, 1.80, 4.30, 0.40, 1.65, 8.00, -1.52),
        obj('Car', 0.00, 2, -1.57, 1.45, 1.55, 3.60, 0.60, 1.64, 22.00, -1.54),
        obj('Car', 0.00, 1, -1.00, 1.50, 1.60, 3.90, -1.90, 1.66, 16.00, -1.12),
        obj('Car', 0.00, 0, 1.30, 1.50, 1.62, 3.95, 7.90, 1.60, 19.00, 1.69)]),
    # 3: a car beside the camera with corners behind it (z < 0), clamped right and bottom; one clamped left; one clamped top and bottom
    ('000003', (376, 1241), CALIB, [
        obj('Car', 0.60, 0, -2.10, 1.50, 1.60, 4.00, 2.60, 1.60, 1.80, -1.57),
        obj('Car', 0.40, 0, -0.90, 1.52, 1.64, 3.80, -4.60, 1.64, 7.00, -1.80),
        obj('Car', 0.30, 0, -1.50, 3.60, 1.70, 4.20, 0.30, 1.70, 4.50, -1.45)]),
    # 4: label angles beyond +pi and -pi (wrapped by the flip), one just inside
    ('000004', (375, 1242), CALIB, [
        obj('Car', 0.00, 0, 3.30, 1.50, 1.60, 3.90, -4.00, 1.62, 15.00, 3.04),
        obj('Car', 0.00, 0, -3.25, 1.49, 1.61, 3.85, 3.80, 1.63, 18.50, -3.05),
        obj('Car', 0.00, 0, 3.10, 1.53, 1.65, 4.00, 0.20, 1.61, 30.00, 3.11),
        obj('Car', 0.00, 0, -0.05, 1.46, 1.57, 3.60, -14.00, 1.70, 27.00, -0.39)]),
    # 5: nothing survives the filter: dropped by filter_roidb, and so is its flipped copy
    ('000005', (375, 1242), CALIB, [
        obj('Van', 0.00, 0, -1.40, 2.20, 1.90, 5.10, -3.10, 1.80, 20.20, -1.55),
        obj('Car', 1.00, 0, -1.20, 1.50, 1.62, 3.90, -5.00, 1.65, 7.00, -1.80),
        obj('Truck', 0.00, 0, 1.58, 3.20, 2.60, 9.00, 5.00, 1.90, 35.00, 1.72),
        DONTCARE]),
    # 6: a car of which the near one leaves three columns or less: visible width <= 3 (x of the near car is searched below)
    ('000006', (375, 1242), CALIB, [
        obj('Car', 0.00, 2, -1.57, 1.50, 1.60, 3.90, 0.00, 1.65, 30.00, -1.57),
        'NEAR',
        obj('Misc', 0.00, 0, -1.57, 1.20, 1.00, 2.00, -10.00, 1.65, 25.00, -1.57),
        obj('Car', 0.00, 0, 1.20, 1.50, 1.62, 3.95, 8.40, 1.60, 26.00, 1.51)]),
]


def write_dataset(tmp, frames):
    base = os.path.join(tmp, 'data', 'kitti', 'object', 'training')
    for d in ('image_2', 'image_3', 'label_2', 'calib'):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    os.makedirs(os.path.join(tmp, 'data', 'kitti', 'splits'), exist_ok=True)
    for fid, (H, W), calib, lines in frames:
        for d in ('image_2', 'image_3'):
            Image.fromarray(np.zeros((H, W, 3), dtype=np.uint8)).save(os.path.join(base, d, fid + '.png'))
        open(os.path.join(base, 'label_2', fid + '.txt'), 'w').write('\n'.join(lines) + '\n')
        open(os.path.join(base, 'calib', fid + '.txt'), 'w').write(calib)
    open(os.path.join(tmp, 'data', 'kitti', 'splits', 'train.txt'), 'w').write('\n'.join(f[0] for f in frames))
    cache = os.path.join(tmp, 'data', 'kitti', 'object', 'kitti_train_gt_roidb.pkl')
    if os.path.exists(cache):
        os.remove(cache)
    return base


def analyse(tmp, fid, shape):
    """The reference's objects of one frame before and after both occlusion passes (for the assertions below)."""
    from datasets.kitti import kitti
    from model.utils import kitti_utils
    base = os.path.join(tmp, 'data', 'kitti', 'object', 'training')
    calib = kitti_utils.read_obj_calibration(os.path.join(base, 'calib', fid + '.txt'))
    raw = kitti_utils.read_obj_data(os.path.join(base, 'label_2', fid + '.txt'), calib, shape + (3,))
    raw_boxes = [[o.boxes[j].box.copy() for j in range(2)] for o in raw]
    raw_kpts = [[o.boxes[j].keypoints.copy() for j in range(2)] for o in raw]
    k = kitti('train', os.path.join(tmp, 'data', 'kitti', 'object'))
    after = k.remove_occluded_keypoints(list(raw))
    after = k.remove_occluded_keypoints(after, left=False)
    return raw, raw_boxes, raw_kpts, after


def annotation_frames(tmp, d):
    from roi_data_layer.roidb import combined_roidb
    from model.utils.config import cfg
    from model.utils import kitti_utils
    frames = [list(f) for f in FRAMES]
    # frame 6: move the near car until it leaves the far one (object 0) a visible width of at most 3 columns in an eye
    found = None
    for step in range(0, 400):
        x = 0.40 + 0.005 * step
        lines = [ln if ln != 'NEAR' else obj('Car', 0.00, 0, -1.57, 1.55, 1.70, 4.10, x, 1.65, 10.00, -1.57) for ln in FRAMES[6][3]]
        write_dataset(tmp, [(FRAMES[6][0], FRAMES[6][1], FRAMES[6][2], lines)])
        raw, _, _, after = analyse(tmp, '000006', FRAMES[6][1])
        far = raw[0]
        if far not in after:
            continue
        widths = [far.boxes[j].visible_right - far.boxes[j].visible_left for j in range(2)]
        if min(widths) <= 3 and max(widths) > 0:
            found = lines
            break
    assert found is not None, "no position of the near car leaves a visible width <= 3"
    frames[6][3] = found
    frames = [tuple(f) for f in frames]
    write_dataset(tmp, frames)

    # ---- what the frames must contain
    info = {f[0]: analyse(tmp, f[0], f[1]) for f in frames}
    raw, boxes, kpts, after = info['000001']
    assert raw[0].truncate >= 0.98 and raw[1].occlusion == 3 and boxes[2][0][3] - boxes[2][0][1] <= 10
    raw, boxes, kpts, after = info['000002']
    assert raw[1] not in after, "the fully hidden car is removed"
    part = raw[2]
    assert part in after and part.boxes[0].visible_right < part.boxes[0].box[2], "the partly hidden car's range is shortened"
    assert (part.boxes[0].keypoints == -1).sum() > (kpts[2][0] == -1).sum(), "it lost a keypoint to the occlusion pass"
    raw, boxes, kpts, after = info['000003']
    H3, W3 = FRAMES[3][1]
    assert boxes[0][0][2] == W3 - 1 and boxes[0][0][3] == H3 - 1, "clamped right and bottom"
    assert boxes[1][0][0] == 0, "clamped left"
    assert boxes[2][0][1] == 0 and boxes[2][0][3] == H3 - 1, "clamped top and bottom"
    c = raw[0]
    zs = [(c.pos + c.R.dot(v) / 2.0)[2] for v in ([-c.dim[0], 0, -c.dim[2]], [c.dim[0], 0, c.dim[2]], [-c.dim[0], 0, c.dim[2]],
                                                  [c.dim[0], 0, -c.dim[2]])]
    assert min(zs) < 0 < max(zs), "corners behind the camera"
    raw, boxes, kpts, after = info['000006']
    far = raw[0]
    assert far in after and min(far.boxes[j].visible_right - far.boxes[j].visible_left for j in range(2)) <= 3

    cfg.TRAIN.USE_FLIPPED = True
    imdb, roidb, ratio_list, ratio_index = combined_roidb('kitti_train')
    n_frames = len(frames)
    ids = [f[0] for f in frames] * 2
    kept = [os.path.basename(e['img_left'])[:-4] for e in roidb]
    assert '000005' not in kept and len(roidb) == 2 * (n_frames - 1), (kept, len(roidb))
    assert kept == [i for i in ids if i != '000005']
    n_objs = [len(e['boxes_left']) for e in roidb]
    print('roidb entries', len(roidb), 'objects', n_objs, 'ratio_index', ratio_index.tolist())
    alphas = np.concatenate([e['dim_orien'][:, 3] for e in roidb[:n_frames - 1]])
    assert (alphas > np.pi).any() and (alphas < -np.pi).any() and (alphas > 0).any() and (alphas < 0).any()
    d['ann_ids'] = np.asarray([f[0] for f in frames])
    d['ann_shapes'] = np.asarray([f[1] for f in frames], dtype=np.int64)
    d['ann_labels'] = np.asarray(['\n'.join(f[3]) + '\n' for f in frames])
    d['ann_calibs'] = np.asarray([f[2] for f in frames])
    d['roidb_len'] = np.int64(len(roidb))
    d['roidb_ids'] = np.asarray(kept)
    d['ratio_list'] = np.asarray(ratio_list)
    d['ratio_index'] = np.asarray(ratio_index, dtype=np.int64)
    for i, e in enumerate(roidb):
        for k in ('boxes_left', 'boxes_right', 'boxes_merge', 'dim_orien', 'kpts', 'gt_classes'):
            d['roidb_%d_%s' % (i, k)] = e[k]
        if not e['flipped']:
            for k in ('kpts_right', 'truncation', 'occlusion'):
                d['roidb_%d_%s' % (i, k)] = e[k]
        d['roidb_%d_meta' % i] = np.asarray([int(e['flipped']), e['width'], e['height'], e['need_crop']], dtype=np.int64)


def ratio_case(d):
    from roi_data_layer.roidb import rank_roidb_ratio
    wh = [(1242, 375), (100, 100), (90, 100), (100, 70), (60, 100), (100, 55), (40, 100), (130, 100), (175, 100), (51, 100)]
    rd = [{'width': w, 'height': h} for w, h in wh]
    ratio_list, ratio_index = rank_roidb_ratio(rd)
    inside = [w / float(h) for w, h in wh if 0.5 <= w / float(h) <= 2]
    assert len(set(inside)) == len(inside) and sum(e['need_crop'] for e in rd) == 2
    d.update(rank_wh=np.asarray(wh, dtype=np.int64), rank_ratio_list=np.asarray(ratio_list),
             rank_ratio_index=np.asarray(ratio_index, dtype=np.int64), rank_need_crop=np.asarray([e['need_crop'] for e in rd], dtype=np.int64))


class _ShuffleRecorder(object):
    def __init__(self):
        self.perm = None
        self.random = self

    def shuffle(self, x):
        before = x.copy()
        state = np.random.get_state()
        idx = np.arange(len(x))
        np.random.shuffle(idx)
        np.random.set_state(state)
        np.random.shuffle(x)
        assert np.array_equal(x, before[idx]), "the index column saw another permutation"
        self.perm = idx

    def __getattr__(self, name):
        return getattr(np, name)


def hand_entry(rng, n, width, height, flipped, special):
    """n objects inside a width x height image; `special`: rows with x1 beyond the blob and keypoints on and past the edges."""
    x1 = rng.uniform(0, width - 30, n)
    w = rng.uniform(8, 28, n)
    y1 = rng.uniform(0, height - 16, n)
    hh = rng.uniform(6, 14, n)
    left = np.stack([x1, y1, x1 + w, y1 + hh], 1).astype(np.float32)
    disp = rng.uniform(1, 6, n).astype(np.float32)
    right = left.copy()
    right[:, 0] -= disp
    right[:, 2] -= disp
    right[:, 0] = np.maximum(right[:, 0], 0)
    merge = left.copy()
    merge[:, 0] = np.minimum(left[:, 0], right[:, 0])
    merge[:, 2] = np.maximum(left[:, 2], right[:, 2])
    dim_orien = np.stack([rng.uniform(1.4, 1.9, n), rng.uniform(1.3, 1.7, n), rng.uniform(3.3, 4.5, n), rng.uniform(-3.3, 3.3, n)], 1)
    kpts = np.full((n, 6), -1.0)
    for i in range(n):
        kpts[i, rng.randint(4)] = left[i, 0] + rng.uniform(0.2, 0.8) * w[i]
        kpts[i, 4], kpts[i, 5] = left[i, 0] + 0.05 * w[i], left[i, 0] + 0.93 * w[i]
    kpts = kpts.astype(np.float32)
    if special:
        left[0, 0] = width + 3.5                 # x1 beyond the blob width after scaling
        merge[0, 0] = width + 1.25
        right[0, 0] = width + 0.5
        kpts[0] = [0.0, -0.01, width - 0.5, width - 0.49, 0.0, width - 0.5]       # exactly 0 / im_width - 1 at scale 2, and just past
        if n > 1:
            kpts[1, 4], kpts[1, 5] = -0.25, width + 2.0
    return {'boxes_left': left, 'boxes_right': right, 'boxes_merge': merge, 'dim_orien': dim_orien.astype(np.float32), 'kpts': kpts,
            'gt_classes': np.ones(n, dtype=np.int32), 'flipped': flipped}


def loader_cases(tmp, d):
    import roi_data_layer.roibatchLoader as rbl
    from model.utils.config import cfg
    rec = _ShuffleRecorder()
    rbl.np = rec
    rng = np.random.RandomState(21)
    # (n, H, W, target, flipped, special): scale 2 where the exact edges are wanted, 1.6 elsewhere
    cases = [(1, 32, 100, 64, False, True), (2, 32, 100, 64, True, True), (30, 40, 132, 64, False, False),
             (31, 40, 132, 64, False, False), (40, 40, 132, 64, True, False)]
    cfg.TRAIN.MAX_SIZE = 2484
    for ci, (n, H, W, target, flipped, special) in enumerate(cases):
        e = hand_entry(rng, n, W, H, flipped, special)
        for eye in ('left', 'right'):
            path = os.path.join(tmp, 'hand_%d_%s.png' % (ci, eye))
            Image.fromarray(rng.randint(0, 256, (H, W, 3)).astype(np.uint8)).save(path)
            e['img_' + eye] = path
        e['width'], e['height'], e['need_crop'] = W, H, 1
        cfg.TRAIN.SCALES = (target,)
        ds = rbl.roibatchLoader([e], np.asarray([2.0]), np.asarray([0]), 1, 2, training=True)
        rec.perm = None
        np.random.seed(100 + ci)
        out = ds[0]
        perm = rec.perm if rec.perm is not None else np.arange(n)
        assert cfg.MAX_NUM_GT_BOXES == 30 and out[8] == min(n, 30)
        im_info = out[2].numpy()
        scale = float(target) / H
        assert im_info[1] == out[0].shape[2] and abs(im_info[2] - scale) < 1e-6
        if special:
            assert scale == 2.0 and (e['boxes_left'][:, 0] * scale > im_info[1]).any()
            k = out[7].numpy()[:n][np.argsort(perm)] if n > 1 else out[7].numpy()[:n]
            assert k[0].tolist() == [0.0, -1.0, im_info[1] - 1, -1.0, 0.0, im_info[1] - 1], k[0]
        if n > 30:
            assert sorted(perm[:30].tolist()) != list(range(30)), "truncation after the shuffle drops other rows than truncation before it"
        pre = 'hand_%d_' % ci
        for k in ('boxes_left', 'boxes_right', 'boxes_merge', 'dim_orien', 'kpts', 'gt_classes'):
            d[pre + k] = e[k]
        d[pre + 'meta'] = np.asarray([n, H, W, target, int(flipped)], dtype=np.int64)
        d[pre + 'perm'] = np.asarray(perm, dtype=np.int64)
        d[pre + 'im_info'] = im_info
        for name, t in zip(('gt_left', 'gt_right', 'gt_merge', 'gt_dim_orien', 'gt_kpts'), out[3:8]):
            d[pre + name] = t.numpy().astype(np.float32)
        d[pre + 'num_boxes'] = np.int64(out[8])
    d['hand_cases'] = np.int64(len(cases))


def image_cases(tmp, d):
    from roi_data_layer import minibatch
    from model.utils.config import cfg
    rng = np.random.RandomState(33)
    # (H, W, target, max_size, flipped): scales 11/7, 1.625, 48/37 (non-terminating), 1.6 = 600/375 with the crop
    cases = [(7, 11, 11, 2484, False), (7, 11, 11, 2484, True), (8, 13, 13, 2484, False), (8, 13, 13, 2484, True),
             (37, 41, 48, 2484, False), (37, 41, 48, 2484, True), (30, 100, 48, 150, True)]
    imgs = {}
    for ci, (H, W, target, max_size, flipped) in enumerate(cases):
        key = (H, W)
        if key not in imgs:
            imgs[key] = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)]
        e = {'flipped': flipped}
        for eye, im in zip(('left', 'right'), imgs[key]):
            path = os.path.join(tmp, 'img_%d_%s.png' % (ci, eye))
            Image.fromarray(im).save(path)
            e['img_' + eye] = path
        cfg.TRAIN.SCALES, cfg.TRAIN.MAX_SIZE = (target,), max_size
        bl, br, scales = minibatch._get_image_blob([e], [0])
        assert scales[0] == float(target) / float(min(H, W))
        if max_size < 2484:
            assert bl.shape[2] == max_size, "the crop case crops"
        pre = 'img_%d_' % ci
        d[pre + 'left'], d[pre + 'right'] = imgs[key]
        d[pre + 'meta'] = np.asarray([H, W, target, max_size, int(flipped)], dtype=np.int64)
        d[pre + 'blob_left'], d[pre + 'blob_right'] = bl, br
    cfg.TRAIN.SCALES, cfg.TRAIN.MAX_SIZE = (600,), 2484
    d['img_cases'] = np.int64(len(cases))


def main():
    d = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            annotation_frames(tmp, d)
            ratio_case(d)
            loader_cases(tmp, d)
            image_cases(tmp, d)
        finally:
            os.chdir(cwd)
    path = os.path.join(HERE, 'reference_loader.npz')
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
