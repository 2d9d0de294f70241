"""One stereo pair from disk - the reference's demo.py:63-338:

    python -m stereo_rcnn_amd.demo --left demo/left.png --right demo/right.png --calib demo/calib.txt --checkpoint models_stereo/stereo_rcnn_12_6477.pth

Prints one KITTI-format line per aligned object (class, alpha, 2-D box, h w l, x y z, ry, score) and the two phase
times the reference reports (`det_time`: forward + decode, `solve_time`: 3-D solve + dense alignment).  `--out result.png` also
writes the picture the reference shows in a window (demo.py:225-333: both images with the 2-D boxes, the 3-D wireframes, the
bird's-eye view of `--lidar demo/lidar.bin` with the 3-D boxes), drawn on the device by stereo_rcnn_amd/visualize.py."""
import argparse
import os
import sys
import tempfile
import time

import torch

from . import pipeline
from .images import read_png_rgb
from .model.stereo_rcnn.resnet import load_checkpoint, resnet
from .model.utils import kitti_utils


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--left', required=True)
    ap.add_argument('--right', required=True)
    ap.add_argument('--calib', required=True)
    ap.add_argument('--checkpoint', required=True)
    ap.add_argument('--precision', choices=['f16x3', 'f32'], default='f16x3')
    ap.add_argument('--out', default=None, help='write the result picture (PNG) here')
    ap.add_argument('--lidar', default=None, help='velodyne .bin for the bird\'s-eye view of --out (absent: a white one, as the reference)')
    ap.add_argument('--vis-thresh', type=float, default=0.7, help='score above which --out draws a detection (demo.py:95)')
    args = ap.parse_args(argv)
    if args.lidar and not os.path.isfile(args.lidar):
        ap.error('--lidar %s: no such file (leave the option out for a white bird\'s-eye view)' % args.lidar)
    from . import serving
    serving.before_hip()
    serving.enter(1)                      # one pair: latency regime (branches on side streams, in-situ plans)
    dev = torch.device('cuda:0')
    model = resnet(('__background__', 'Car'), 101, pretrained=False)
    model.create_architecture()
    load_checkpoint(model, args.checkpoint)
    model.cuda()
    model.eval()
    model.precision = args.precision
    left, right = read_png_rgb(args.left), read_png_rgb(args.right)
    calib = kitti_utils.read_obj_calibration(args.calib)
    lu, ru = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    pipeline.detect_3d_images(model, lu, ru, calib)                             # first call: per-shape autotuning
    torch.cuda.synchronize()
    t0 = time.time()
    objs = pipeline.detect_3d_images(model, lu, ru, calib)                      # preprocessing .. rectified 3-D boxes, on the device
    torch.cuda.synchronize()
    dt = time.time() - t0
    with tempfile.TemporaryDirectory() as td:
        pipeline.write_kitti_results(td, 'demo', calib, [o for o in objs if o['aligned']])
        try:
            sys.stdout.write(open(td + '/data/demo.txt').read())
        except FileNotFoundError:
            pass
    print('%d objects (%d aligned) in %.1f ms' % (len(objs), sum(o['aligned'] for o in objs), dt * 1e3))
    if args.out:
        from . import visualize
        from .distributed import objects_to_record
        lidar = visualize.read_lidar(args.lidar) if args.lidar else None           # none: a white bird's-eye view (kitti_utils.py:353-354)
        panel = visualize.render_result(lu, ru, objects_to_record(objs).to(dev), calib, lidar, args.vis_thresh)
        visualize.save_png(panel, args.out)


if __name__ == '__main__':
    main()
