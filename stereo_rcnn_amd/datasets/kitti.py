"""KITTI annotations -> the training roidb: the per-dataset half of the reference's data path, host numpy, run once.

Restates lib/datasets/kitti.py (remove_occluded_keypoints :141-197, _load_kitti_annotation :199-279), lib/datasets/imdb.py
(append_flipped_images :117-176) and lib/roi_data_layer/roidb.py (prepare_roidb's paths and sizes :23-31, rank_roidb_ratio :49-73,
filter_roidb :75-86), in the reference's order of operations and dtypes (float64 geometry, float32 / int32 arrays), so that every
array equals the reference's bit for bit (tests/test_loader_roidb_cpu.py against tests/golden/reference_loader.npz).

Left out: the scipy-sparse `gt_overlaps` / `gt_subindexes*` / `*subclasses` bookkeeping of _load_kitti_annotation.  Nothing
downstream of prepare_roidb's own sanity checks reads it (minibatch.py takes boxes, dim_orien, kpts, gt_classes and flipped).
No pickle cache is written.  The split file is an argument.

rank_roidb_ratio sorts with np.argsort(kind='stable').  The reference's default (unstable) sort leaves the order of equal ratios
to the numpy build; every KITTI frame is wider than 2:1 and clips to ratio 2, so on KITTI the reference's order is arbitrary
anyway and the stable one (index order) is as good as any.
"""
import math
import os

import numpy as np

from ..images import read_split
from ..model.utils import kitti_utils

CLASSES = ('__background__', 'Car')
_CLASS_TO_IND = dict(zip(CLASSES, range(len(CLASSES))))


def image_paths(kitti_path, index):
    return (os.path.join(kitti_path, 'training', 'image_2', index + '.png'),
            os.path.join(kitti_path, 'training', 'image_3', index + '.png'))


def remove_occluded_keypoints(objects, left=True):
    """kitti.py:141-197: the visible column range of every box from a 1260-column depth line over all objects, keypoints of
    fully hidden boxes set to -1 and those objects removed, then keypoints outside the visible range (+-5) or within 3 columns of
    the outermost keypoints set to -1."""
    ix = 0 if left else 1
    depth_line = np.zeros(1260, dtype=float)
    for o in objects:
        for col in range(int(o.boxes[ix].box[0]), int(o.boxes[ix].box[2]) + 1):
            pixel = depth_line[col]
            if pixel == 0.0:
                depth_line[col] = o.pos[2]
            elif o.pos[2] < depth_line[col]:
                depth_line[col] = (o.pos[2] + pixel) / 2.0
    for o in objects:
        bx = o.boxes[ix]
        bx.visible_left = bx.box[0]
        bx.visible_right = bx.box[2]
        left_visible = not (depth_line[int(bx.box[0])] < o.pos[2])
        right_visible = not (depth_line[int(bx.box[2])] < o.pos[2])
        if not right_visible and not left_visible:
            bx.visible_right = bx.box[0]
            bx.keypoints[:] = -1
        for col in range(int(bx.box[0]), int(bx.box[2]) + 1):
            if left_visible and depth_line[col] >= o.pos[2]:
                bx.visible_right = col
            elif right_visible and depth_line[col] < o.pos[2]:
                bx.visible_left = col
    objects = [o for o in objects if np.sum(o.boxes[ix].keypoints) > -4]
    for o in objects:
        bx = o.boxes[ix]
        left_kpt, right_kpt = 5000, 0
        for j in range(4):
            if bx.keypoints[j] != -1:
                if bx.keypoints[j] < left_kpt:
                    left_kpt = bx.keypoints[j]
                if bx.keypoints[j] > right_kpt:
                    right_kpt = bx.keypoints[j]
        for j in range(4):
            if bx.keypoints[j] != -1:
                if bx.keypoints[j] < bx.visible_left - 5 or bx.keypoints[j] > bx.visible_right + 5 or \
                        bx.keypoints[j] < left_kpt + 3 or bx.keypoints[j] > right_kpt - 3:
                    bx.keypoints[j] = -1
    return objects


def load_annotation(label_path, calib_path, im_shape):
    """One unflipped roidb entry (kitti.py:199-279).  im_shape: (H, W[, 3]) of the left image."""
    calib = kitti_utils.read_obj_calibration(calib_path)
    origin = kitti_utils.read_obj_data(label_path, calib, im_shape)
    origin = remove_occluded_keypoints(origin)
    origin = remove_occluded_keypoints(origin, left=False)
    objects = [o for o in origin
               if o.truncate < 0.98 and o.occlusion < 3 and (o.boxes[0].box[3] - o.boxes[0].box[1]) > 10 and o.cls in CLASSES
               and o.boxes[0].visible_right - o.boxes[0].visible_left > 3
               and o.boxes[1].visible_right - o.boxes[1].visible_left > 3]
    n = len(objects)
    e = {'boxes_left': np.zeros((n, 4), dtype=np.float32), 'boxes_right': np.zeros((n, 4), dtype=np.float32),
         'boxes_merge': np.zeros((n, 4), dtype=np.float32), 'dim_orien': np.zeros((n, 4), dtype=np.float32),
         'kpts': np.zeros((n, 6), dtype=np.float32), 'kpts_right': np.zeros((n, 6), dtype=np.float32),
         'truncation': np.zeros((n), dtype=np.float32), 'occlusion': np.zeros((n), dtype=np.float32),
         'gt_classes': np.zeros((n), dtype=np.int32), 'flipped': False}
    for i, o in enumerate(objects):
        e['boxes_left'][i, :] = o.boxes[0].box
        e['boxes_right'][i, :] = o.boxes[1].box
        e['boxes_merge'][i, :] = o.boxes[2].box
        e['dim_orien'][i, 0:3] = o.dim
        e['dim_orien'][i, 3] = o.alpha
        e['kpts'][i, :4] = o.boxes[0].keypoints
        e['kpts'][i, 4] = o.boxes[0].visible_left
        e['kpts'][i, 5] = o.boxes[0].visible_right
        e['kpts_right'][i, :4] = o.boxes[1].keypoints
        e['kpts_right'][i, 4] = o.boxes[1].visible_left
        e['kpts_right'][i, 5] = o.boxes[1].visible_right
        e['occlusion'][i] = o.occlusion
        e['truncation'][i] = o.truncate
        e['gt_classes'][i] = _CLASS_TO_IND[o.cls]
    return e


def flipped_entry(entry, width):
    """imdb.py:120-175 for one entry: the flipped frame's LEFT boxes are the mirrored RIGHT boxes and the other way round, its
    kpts the mirrored kpts_right in the order 3, 2, 1, 0 / 5, 4, its angle wrapped into [-pi, pi] and reflected.  `width` is a
    Python int and pi a Python float: numpy computes each line in float32, as it does in the reference."""
    def mirror(boxes):
        boxes = boxes.copy()
        oldx1, oldx2 = boxes[:, 0].copy(), boxes[:, 2].copy()
        boxes[:, 0] = width - oldx2 - 1
        boxes[:, 2] = width - oldx1 - 1
        assert (boxes[:, 2] >= boxes[:, 0]).all()
        return boxes
    boxes_left, boxes_right, boxes_merge = mirror(entry['boxes_right']), mirror(entry['boxes_left']), mirror(entry['boxes_merge'])
    dim_orien = entry['dim_orien'].copy()
    out_range1 = dim_orien[:, 3] > math.pi
    out_range2 = dim_orien[:, 3] < -math.pi
    dim_orien[:, 3][out_range1] = dim_orien[:, 3][out_range1] - 2.0 * math.pi
    dim_orien[:, 3][out_range2] = dim_orien[:, 3][out_range2] + 2.0 * math.pi
    positive = dim_orien[:, 3] >= 0
    negative = dim_orien[:, 3] < 0
    dim_orien[:, 3][positive] = math.pi - dim_orien[:, 3][positive]
    dim_orien[:, 3][negative] = -math.pi - dim_orien[:, 3][negative]
    old = entry['kpts_right']
    kpts = old.copy()
    for dst, src in ((0, 3), (1, 2), (2, 1), (3, 0), (4, 5), (5, 4)):
        kpts[:, dst] = width - old[:, src] - 1
    return {'boxes_left': boxes_left, 'boxes_right': boxes_right, 'boxes_merge': boxes_merge, 'dim_orien': dim_orien, 'kpts': kpts,
            'gt_classes': entry['gt_classes'], 'flipped': True}


def filter_roidb(roidb):
    """roidb.py:75-86: entries without a box are dropped."""
    return [e for e in roidb if len(e['boxes_left']) != 0 and len(e['boxes_right']) != 0 and len(e['boxes_merge']) != 0]


def rank_roidb_ratio(roidb):
    """roidb.py:49-73: width / height clipped to [0.5, 2] ('need_crop' set where it was clipped), sorted ascending.  Returns
    (ratio_list sorted, ratio_index).  Stable sort: see the module docstring."""
    ratio_large, ratio_small = 2, 0.5
    ratio_list = []
    for e in roidb:
        ratio = e['width'] / float(e['height'])
        if ratio > ratio_large:
            e['need_crop'] = 1
            ratio = ratio_large
        elif ratio < ratio_small:
            e['need_crop'] = 1
            ratio = ratio_small
        else:
            e['need_crop'] = 0
        ratio_list.append(ratio)
    ratio_list = np.array(ratio_list)
    ratio_index = np.argsort(ratio_list, kind='stable')
    return ratio_list[ratio_index], ratio_index


def build_roidb(kitti_path, split_file, use_flipped=True, training=True):
    """combined_roidb('kitti_train') (roidb.py:88-131) for one dataset: annotations of every frame of `split_file`, the flipped
    copies appended behind them (cfg.TRAIN.USE_FLIPPED), 'img_left' / 'img_right' / 'width' / 'height' from PIL as prepare_roidb
    and _get_widths take them, entries without boxes filtered out, ranked by ratio.  Returns (roidb, ratio_list, ratio_index)."""
    from PIL import Image
    ids = read_split(split_file)
    roidb, sizes = [], []
    for index in ids:
        left, right = image_paths(kitti_path, index)
        with Image.open(left) as im:
            size = im.size                               # (width, height)
        e = load_annotation(os.path.join(kitti_path, 'training', 'label_2', index + '.txt'),
                            os.path.join(kitti_path, 'training', 'calib', index + '.txt'), (size[1], size[0], 3))
        roidb.append(e)
        sizes.append(size)
    if use_flipped:
        roidb.extend([flipped_entry(roidb[i], sizes[i][0]) for i in range(len(ids))])
        ids, sizes = ids * 2, sizes * 2
    for e, index, size in zip(roidb, ids, sizes):
        e['img_left'], e['img_right'] = image_paths(kitti_path, index)
        e['width'], e['height'] = size[0], size[1]
    if training:
        roidb = filter_roidb(roidb)
    ratio_list, ratio_index = rank_roidb_ratio(roidb)
    return roidb, ratio_list, ratio_index
