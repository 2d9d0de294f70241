"""Host-side KITTI helpers on the inference path - reference lib/model/utils/kitti_utils.py:
`read_obj_calibration` (:97-159), `infer_boundary` (:398-437), `write_detection_results` (:440-460) -- and, for the training
data loader (stereo_rcnn_amd/datasets/kitti.py), `Box2d` / `KittiObject` (:13-31), `E2R` (:57-76) and `read_obj_data` (:161-265).
Pure host I/O / tiny numpy loops in the reference as well.  Of the lidar helpers `velo_to_cam2` is the matrix of
`lidar_to_cam_frame` (:303-340); the per-point work of `get_point_cloud` and the drawing live in stereo_rcnn_amd/visualize.py."""
import math
import os

import numpy as np


class FrameCalibrationData(object):
    """Calibration of one frame (P0..P3, rectification, velodyne->cam), as in kitti_utils.py:37-66."""

    def __init__(self):
        self.p0 = self.p1 = self.p2 = self.p3 = None
        self.p2_2 = self.p2_3 = None
        self.r0_rect = None
        self.t_cam2_cam0 = None
        self.tr_velodyne_to_cam0 = None


def _row(line):
    return [float(v) for v in line.strip().split(' ')[1:] if v != '']


def read_obj_calibration(calib_path):
    """Parse a KITTI object calibration file (kitti_utils.py:97-159)."""
    with open(calib_path, 'r') as fh:
        lines = [ln for ln in fh.read().split('\n')]
    c = FrameCalibrationData()
    p = [np.reshape(_row(lines[i]), (3, 4)) for i in range(4)]
    c.p0, c.p1, c.p2, c.p3 = p
    c.p2_2 = np.copy(p[2])
    c.p2_2[0, 3] -= c.p2[0, 3]
    c.p2_3 = np.copy(p[3])
    c.p2_3[0, 3] -= c.p2[0, 3]
    c.t_cam2_cam0 = np.zeros(3)
    c.t_cam2_cam0[0] = (c.p2[0, 3] - c.p0[0, 3]) / c.p2[0, 0]
    c.r0_rect = np.reshape(_row(lines[4]), (3, 3))
    c.tr_velodyne_to_cam0 = np.reshape(_row(lines[5]), (3, 4))
    return c


def velo_to_cam2(calib):
    """The 4x4 float64 matrix that takes a homogeneous velodyne point into the camera-2 frame (kitti_utils.py:303-340,
    lidar_to_cam_frame): translation by t_cam2_cam0, times R0_rect padded to 4x4, times Tr_velo_to_cam padded to 4x4, multiplied
    in the reference's order (rectification . velodyne first).  The per-point product and the bird's-eye filter run on the
    device (engine.bev_lidar)."""
    rect = np.zeros((4, 4))
    rect[:3, :3] = calib.r0_rect
    rect[3, 3] = 1.0
    velo = np.zeros((4, 4))
    velo[:3, :4] = calib.tr_velodyne_to_cam0
    velo[3, 3] = 1.0
    shift = np.identity(4)
    shift[0:3, 3] = calib.t_cam2_cam0
    return np.dot(shift, np.dot(rect, velo))


def infer_boundary(im_shape, boxes_left):
    """Occlusion border of every object from the 2-D boxes alone (kitti_utils.py:398-437):
    a 1-D 'depth line' over image columns (depth ~ 1050 / y2), then per box the visible [left, right]."""
    boxes_left = np.asarray(boxes_left)
    n = boxes_left.shape[0]
    left_right = np.zeros((n, 2), dtype=np.float32)
    depth_line = np.zeros(im_shape[1] + 1, dtype=float)
    for i in range(n):
        depth = 1050.0 / boxes_left[i, 3]
        for col in range(int(boxes_left[i, 0]), int(boxes_left[i, 2]) + 1):
            pixel = depth_line[col]
            if pixel == 0.0:
                depth_line[col] = depth
            elif depth < depth_line[col]:
                depth_line[col] = (depth + pixel) / 2.0
    for i in range(n):
        d = 1050.0 / boxes_left[i, 3]
        x1, x2 = int(boxes_left[i, 0]), int(boxes_left[i, 2])
        left_right[i, 0], left_right[i, 1] = boxes_left[i, 0], boxes_left[i, 2]
        left_visible = not (depth_line[x1] < d)
        right_visible = not (depth_line[x2] < d)
        if not right_visible and not left_visible:
            left_right[i, 1] = boxes_left[i, 0]
        for col in range(x1, x2 + 1):
            if left_visible and depth_line[col] >= d:
                left_right[i, 1] = col
            elif right_visible and depth_line[col] < d:
                left_right[i, 0] = col
    return left_right


def write_detection_results(result_dir, file_number, calib, box_left, pos, dim, orien, score):
    """Append one detection to `<result_dir>/data/<file_number>.txt` in the KITTI result format consumed by
    the external evaluator (kitti_utils.py:440-460): `Car -1 -1 alpha x1 y1 x2 y2 h w l x y z ry score`,
    x moved from the cam2 to the cam0 frame, yaw reported as `orien - 1.57`."""
    if result_dir is None:
        return
    result_dir = result_dir + '/data'
    dis_cam02 = calib.t_cam2_cam0[0]
    alpha = orien - math.pi / 2 + math.atan2(-pos[0], pos[2])
    line = 'Car -1 -1 '
    line += '%f %f %f %f %f ' % (alpha, box_left[0], box_left[1], box_left[2], box_left[3])
    line += '%f %f %f %f %f %f %f %f \n' % (dim[1], dim[0], dim[2], pos[0] - dis_cam02, pos[1], pos[2],
                                            orien - 1.57, score)
    os.makedirs(result_dir, exist_ok=True)
    with open(os.path.join(result_dir, file_number + '.txt'), 'a') as fh:
        fh.write(line)


class Box2d(object):
    """kitti_utils.py:13-18."""

    def __init__(self):
        self.box = []               # left, top, right, bottom in the image
        self.keypoints = []         # u coordinates of the 4 keypoints, -1 = invisible
        self.visible_left = 0       # leftmost column not occluded by another object
        self.visible_right = 0      # rightmost one


class KittiObject(object):
    """kitti_utils.py:20-31."""

    def __init__(self):
        self.cls = ''               # Car, Van, Truck, Misc
        self.truncate = 0           # float 0 (not truncated) .. 1
        self.occlusion = 0          # integer 0..3
        self.alpha = 0              # viewpoint angle
        self.boxes = (Box2d(), Box2d(), Box2d())      # left, right, merge
        self.pos = []               # x, y, z in the cam2 frame
        self.dim = []               # width (x), height (y), length (z)
        self.orientation = 0
        self.R = []                 # rotation matrix in the cam2 frame


def E2R(Ry, Rx, Rz):
    """Euler angles to the rotation matrix, R_pitch . R_yaw (kitti_utils.py:57-76; Rz is unused there too)."""
    R_yaw = np.array([[math.cos(Ry), 0, math.sin(Ry)],
                      [0, 1, 0],
                      [-math.sin(Ry), 0, math.cos(Ry)]])
    R_pitch = np.array([[1, 0, 0],
                        [0, math.cos(Rx), -math.sin(Rx)],
                        [0, math.sin(Rx), math.cos(Rx)]])
    return R_pitch.dot(R_yaw)


def _space2image(P, pts3):
    n = P.dot(pts3)                 # kitti_utils.py:78-90
    return np.array([n[0] / n[2], n[1] / n[2]])


USED_CLASSES = ('Car', 'Van', 'Truck', 'Misc')


def read_obj_data(label_path, calib=None, im_shape=None):
    """The labelled objects of one KITTI frame (kitti_utils.py:161-265), float64 in the reference's order of operations: the four
    used classes; position moved from the cam0 to the cam2 frame; orientation + pi/2 and E2R; the eight box corners projected
    through p2_2 (left) / p2_3 (right), corners with z < 0 skipped; boxes clamped to the image; of the four bottom keypoints the
    leftmost and the rightmost stay and the others stay only if no deeper than the centre; the merge box is the union."""
    objects = []
    with open(label_path, 'r') as fh:
        lines = fh.readlines()
    for line in lines:
        d = line.split()
        if d[0] not in USED_CLASSES:
            continue
        o = KittiObject()
        o.cls = d[0]
        o.truncate = float(d[1])
        o.occlusion = int(d[2])
        o.alpha = float(d[3])
        o.dim = np.array([d[9], d[8], d[10]]).astype(float)                # width, height, length
        o.pos = np.array(d[11:14]).astype(float) + calib.t_cam2_cam0
        o.orientation = float(d[14]) + math.pi / 2
        o.R = E2R(o.orientation, 0, 0)
        w, h, l = o.dim[0], o.dim[1], o.dim[2]
        corners = [o.pos + o.R.dot([-w, 0, -l]) / 2.0,
                   o.pos + o.R.dot([-w, 0, l]) / 2.0,
                   o.pos + o.R.dot([w, 0, l]) / 2.0,
                   o.pos + o.R.dot([w, 0, -l]) / 2.0,
                   o.pos + o.R.dot([-w, -2.0 * h, -l]) / 2.0,
                   o.pos + o.R.dot([-w, -2.0 * h, l]) / 2.0,
                   o.pos + o.R.dot([w, -2.0 * h, l]) / 2.0,
                   o.pos + o.R.dot([w, -2.0 * h, -l]) / 2.0]
        o.boxes[0].box = np.array([10000, 10000, 0, 0]).astype(float)
        o.boxes[1].box = np.array([10000, 10000, 0, 0]).astype(float)
        o.boxes[2].box = np.array([0.0, 0.0, 0.0, 0.0]).astype(float)
        o.boxes[0].keypoints = np.array([-1.0, -1.0, -1.0, -1.0]).astype(float)
        o.boxes[1].keypoints = np.array([-1.0, -1.0, -1.0, -1.0]).astype(float)
        for j in range(2):
            bx = o.boxes[j]
            P = calib.p2_2 if j == 0 else calib.p2_3
            for i in range(8):
                if corners[i][2] < 0:
                    continue
                pt2 = _space2image(P, np.append(corners[i], [1]))
                if i < 4:
                    bx.keypoints[i] = pt2[0]
                bx.box[0] = min(bx.box[0], pt2[0])
                bx.box[1] = min(bx.box[1], pt2[1])
                bx.box[2] = max(bx.box[2], pt2[0])
                bx.box[3] = max(bx.box[3], pt2[1])
            bx.box[0] = max(bx.box[0], 0)
            bx.box[1] = max(bx.box[1], 0)
            if im_shape is not None:
                bx.box[2] = min(bx.box[2], im_shape[1] - 1)
                bx.box[3] = min(bx.box[3], im_shape[0] - 1)
            left_keypoint, right_keypoint = 5000, 0
            left_inx, right_inx = -1, -1
            for i in range(4):
                if bx.keypoints[i] < left_keypoint:
                    left_keypoint = bx.keypoints[i]
                    left_inx = i
                if bx.keypoints[i] > right_keypoint:
                    right_keypoint = bx.keypoints[i]
                    right_inx = i
            for i in range(4):
                if i == left_inx or i == right_inx:
                    continue
                if corners[i][2] > o.pos[2]:
                    bx.keypoints[i] = -1
        o.boxes[2].box[0] = min(o.boxes[1].box[0], o.boxes[0].box[0])
        o.boxes[2].box[1] = min(o.boxes[1].box[1], o.boxes[0].box[1])
        o.boxes[2].box[2] = max(o.boxes[1].box[2], o.boxes[0].box[2])
        o.boxes[2].box[3] = max(o.boxes[1].box[3], o.boxes[0].box[3])
        objects.append(o)
    return objects
