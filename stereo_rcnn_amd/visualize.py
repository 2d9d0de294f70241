"""Result visualisation - the picture of the reference's demo.py:225-333 / test_net.py:231-339: the left image over the right
image with the 2-D boxes, the projected 3-D wireframes on the left image and a bird's-eye view of the lidar points with the 3-D
boxes, drawn ON THE DEVICE from a detection record (distributed.REC_COLS) by csrc/overlay.hip -- no host read of a detection,
so a flow with pairs in flight can emit pictures without stalling them.

What follows the reference is everything up to the integer pixel coordinates (objects, end points, integer conversions, colours,
thicknesses, panel layout); the line rasterisation rule is this project's own (include/srcnn_hip.h, "result visualisation"):
cv2 is not a dependency, and pixel equality with OpenCV's cv2.line is not claimed.  Images are uint8 RGB here (the reference's
are BGR): (204, 0, 0) is its (0, 0, 204).

`vis_detections`, `vis_box_in_bev`, `vis_single_box_in_img` and `vis_lidar_in_bev` keep the reference's names and argument order
for ported scripts and work in place on device uint8 RGB tensors."""
import numpy as np
import torch

from . import _lib, engine
from .model.utils import kitti_utils

REC_COLS = _lib.REC_COLS


def read_lidar(path):
    """A KITTI velodyne file: float32 (N, 4) tensor of x, y, z, intensity (kitti_utils.py:360-362)."""
    data = np.fromfile(path, dtype=np.float32)
    return torch.from_numpy(data[:data.size // 4 * 4].reshape(-1, 4))


def render_result(left_u8, right_u8, record, calib, lidar=None, vis_thresh=0.7):
    """The whole panel of one pair: uint8 RGB (2 H, W + x_max, 3) on the device.  left_u8 / right_u8: uint8 RGB (H, W, 3) device
    tensors; record: the pair's (max_det + 1, REC_COLS) device record; calib: its FrameCalibrationData; lidar: (N, 4) float32
    points (host tensors are uploaded) or None = a white bird's-eye view, as the reference shows without a lidar file.  Runs on the
    current stream and reads nothing back."""
    dev = left_u8.device
    plane = None
    if lidar is not None:
        pts = lidar.to(dev, non_blocking=True).contiguous()
        plane = engine.bev_lidar(pts, kitti_utils.velo_to_cam2(calib), int(left_u8.shape[0]))
    return engine.render_overlay(left_u8, right_u8, record, calib.p2, vis_thresh, plane)


def save_png(panel, path):
    """Write a uint8 RGB (h, w, 3) tensor as a PNG (the one host read of the picture)."""
    from PIL import Image
    Image.fromarray(panel.detach().cpu().numpy()).save(path)


def _record_of(dev, rows):
    rec = torch.zeros((rows.shape[0] + 1, REC_COLS), dtype=torch.float32)
    rec[0, 0] = rows.shape[0]
    rec[1:] = rows
    return rec.to(dev)


def vis_detections(im, class_name, dets, thresh=0.8, kpts=None):
    """net_utils.vis_detections: the first 100 rows of dets (n, 5) [x1, y1, x2, y2, score] with score > thresh as red rectangles.
    im: uint8 RGB (H, W, 3) device tensor, drawn in place and returned; dets: a device tensor (never read back) or an array."""
    dets = torch.as_tensor(dets, dtype=torch.float32).to(im.device)
    rec = torch.zeros((dets.shape[0] + 1, REC_COLS), dtype=torch.float32, device=im.device)
    rec[0, 0] = dets.shape[0]
    rec[1:, 0] = dets[:, -1]
    rec[1:, 1:5] = dets[:, :4]
    H = int(im.shape[0])
    panel = engine.render_overlay(im, im, rec, np.zeros((3, 4)), thresh, bev=False, layers=_lib.OVERLAY_BOXES)
    im.copy_(panel[:H])
    return im


def _pose_record(dev, pos, dim, theta):
    row = torch.zeros((1, REC_COLS), dtype=torch.float32)
    row[0, 0], row[0, 25] = 1.0, 1.0
    row[0, 9:12] = torch.as_tensor(np.asarray(dim, np.float64)[:3], dtype=torch.float32)
    row[0, 27:30] = torch.as_tensor(np.asarray(pos, np.float64)[:3], dtype=torch.float32)
    row[0, 30] = float(theta)
    return _record_of(dev, row)


def vis_single_box_in_img(img, calib, pos, dim, theta):
    """vis_3d_utils.vis_single_box_in_img: the green wireframe of one 3-D box (pos, dim = (w, h, l), theta; float32 as in a record)
    projected with calib.p2.  img: uint8 RGB (H, W, 3) device tensor, drawn in place and returned."""
    H = int(img.shape[0])
    panel = engine.render_overlay(img, img, _pose_record(img.device, pos, dim, theta), calib.p2, 0.0, bev=False,
                                  layers=_lib.OVERLAY_WIREFRAMES)
    img.copy_(panel[:H])
    return img


def vis_lidar_in_bev(pointcloud, calib, width=750):
    """vis_3d_utils.vis_lidar_in_bev over kitti_utils.get_point_cloud: the (width, x_max, 3) bird's-eye picture of a velodyne cloud
    ((N, 4) float32 device tensor; unlike the reference's it is still in the velodyne frame: the kernel transforms it)."""
    assert width % 2 == 0, "width is 2 H"
    plane = engine.bev_lidar(pointcloud, kitti_utils.velo_to_cam2(calib), width // 2)
    return plane.unsqueeze(2).expand(-1, -1, 3).contiguous()


def vis_box_in_bev(im_bev, pos, dim, orien, width=750, gt=False):
    """vis_3d_utils.vis_box_in_bev: one box's footprint and heading on a bird's-eye picture, green, or red (the reference's BGR
    (0, 0, 255)) for gt=True.  im_bev: uint8 RGB (width, x_max, 3) device tensor, drawn in place and returned."""
    assert width % 2 == 0 and int(im_bev.shape[0]) == width, "width is 2 H, the picture's height"
    H = width // 2
    blank = torch.zeros((H, 1, 3), dtype=torch.uint8, device=im_bev.device)
    panel = engine.render_overlay(blank, blank, _pose_record(im_bev.device, pos, dim, orien), np.zeros((3, 4)), 0.0,
                                  layers=_lib.OVERLAY_BEV_BOXES)
    drawn = panel[:, 1:]
    assert tuple(drawn.shape) == tuple(im_bev.shape)
    mask = (drawn != 255).any(dim=2, keepdim=True)                 # the box's pixels on the white background
    colour = torch.tensor([255, 0, 0] if gt else [0, 200, 0], dtype=torch.uint8, device=im_bev.device)
    im_bev.copy_(torch.where(mask, colour.expand_as(im_bev), im_bev))
    return im_bev
