"""The KITTI split driver followed by its evaluation: `test_net` over the split, then (rank 0, after every rank has written
its result files) the AP table of `kitti_eval` -- AP_2d / AOS / AP_bev / AP_3d at Easy / Moderate / Hard, matching on the
GPU -- printed and written to <result-dir>/ap.json.

    python -m stereo_rcnn_amd.run_kitti --label-dir <.../training/label_2> <test_net arguments>
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m stereo_rcnn_amd.run_kitti --label-dir L ...

Every argument but --label-dir goes to `python -m stereo_rcnn_amd.test_net` unchanged (--kitti-root, --split, --checkpoint,
--result-dir, ...).  test_net.main returns once every rank has passed its final barrier, so rank 0 evaluates complete files.
"""
import argparse
import os
import sys

from . import images, kitti_eval, test_net


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, add_help=False)
    ap.add_argument('--label-dir', required=True, help='KITTI label_2 directory (<id>.txt)')
    ap.add_argument('--split', required=True)
    ap.add_argument('--result-dir', required=True)
    args, _ = ap.parse_known_args(argv)
    rest, skip = [], False
    for a in (argv if argv is not None else sys.argv[1:]):      # everything but --label-dir goes to test_net
        if skip:
            skip = False
        elif a == '--label-dir':
            skip = True
        elif not a.startswith('--label-dir='):
            rest.append(a)
    test_net.main(rest)
    if int(os.environ.get('RANK', 0)) == 0:
        import torch
        device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)))
        return kitti_eval.evaluate_split(args.label_dir, args.result_dir, images.read_split(args.split), device,
                                         log=lambda s: print(s, flush=True))
    return None


if __name__ == '__main__':
    main()
