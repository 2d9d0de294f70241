"""The KITTI split driver with the reference's result picture per frame (test_net.py:231-339 draws it in a window):

    python -m stereo_rcnn_amd.vis_net --vis-dir DIR <test_net arguments>
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m stereo_rcnn_amd.vis_net --vis-dir DIR ...

Every argument but --vis-dir / --vis-thresh goes to `python -m stereo_rcnn_amd.test_net` unchanged, and test_net.main runs as
it always does (same arguments, model loading, sharding, frame path: page-locked ring, decode workers, pairs in flight, result
files, --gather).  While it runs, `pictures()` stands between its loop and `pipeline.detect_3d_stream`: every frame that goes in is
remembered (a device copy of the pair, made on a copy stream when the frame is a page-locked ring entry that will be reused),
and when its objects come out a writer thread draws <vis-dir>/<id>.png on a stream of its own (stereo_rcnn_amd/visualize.py;
<kitti-root>/velodyne/<id>.bin behind the bird's-eye view where the file exists), so the pairs in flight are not held up.  Leaving
`pictures()` waits for every picture and raises what the writer raised.  Only the uint8 frame form (--solver host | device) carries
the images a picture needs; --solver scipy is refused."""
import argparse
import collections
import concurrent.futures as cf
import contextlib
import os
import sys

import numpy as np
import torch

from . import images, pipeline, test_net, visualize
from .distributed import objects_to_record, shard_indices


class PictureWriter(object):
    """Draws <vis_dir>/<ids[k]>.png for the k-th frame that passes through `stream()`.  `close()` must be called when the loop
    that consumes `stream()` is over (the loop may abandon the generator after its last frame): it waits for every picture
    and raises the first error of the writer thread."""
    BACKLOG = 16

    def __init__(self, device, vis_dir, ids, kitti_root=None, vis_thresh=0.7):
        self.device, self.vis_dir, self.ids, self.kitti_root, self.vis_thresh = torch.device(device), vis_dir, list(ids), kitti_root, vis_thresh
        os.makedirs(vis_dir, exist_ok=True)
        self.pending = collections.deque()
        self.count = 0                      # frames handed to the writer
        self.executor = cf.ThreadPoolExecutor(max_workers=1)
        self.copy_stream = self.draw_stream = None      # made with the first frame: HIP must not start before the driver says so

    def _keep(self, image):
        """A device copy of one image that stays valid until its picture is drawn, and the event after which it is complete."""
        if isinstance(image, torch.Tensor) and image.is_cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))          # uploaded by the loop on its stream; a tensor of the frame's own
            return image, ev
        host = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.array(image, copy=True))
        with torch.cuda.stream(self.copy_stream):
            dev = host.to(self.device, non_blocking=True)
            dev.record_stream(self.draw_stream)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        return dev, ev

    def _draw(self, frame, left, right, events, calib, objs):
        path = os.path.join(self.kitti_root, 'velodyne', frame + '.bin') if self.kitti_root else None
        lidar = visualize.read_lidar(path) if path and os.path.isfile(path) else None
        with torch.cuda.device(self.device), torch.cuda.stream(self.draw_stream):
            for ev in events:
                self.draw_stream.wait_event(ev)
            panel = visualize.render_result(left, right, objects_to_record(objs).to(self.device), calib, lidar, self.vis_thresh)
            visualize.save_png(panel, os.path.join(self.vis_dir, frame + '.png'))

    def stream(self, detect, frames):
        """`detect(frames)` with a picture per frame: a generator of the same object lists."""
        kept = collections.deque()

        def remembered():
            for frame in frames:
                if len(frame) != 3:
                    raise ValueError('pictures need the uint8 frame form (left, right, calib): use --solver host or device')
                if self.copy_stream is None:
                    self.copy_stream, self.draw_stream = torch.cuda.Stream(self.device), torch.cuda.Stream(self.device)
                (left, ev_l), (right, ev_r) = self._keep(frame[0]), self._keep(frame[1])
                kept.append((left, right, (ev_l, ev_r), frame[2]))
                yield frame

        for objs in detect(remembered()):
            left, right, events, calib = kept.popleft()
            for ev in events:
                ev.synchronize()            # long done (the pair went through the network since): a ring entry is free for reuse from here
            name = self.ids[self.count]
            self.count += 1
            self.pending.append(self.executor.submit(self._draw, name, left, right, events, calib, objs))
            while len(self.pending) > self.BACKLOG:
                self.pending.popleft().result()         # bounded backlog; raises what the writer raised
            yield objs

    def close(self):
        try:
            while self.pending:
                self.pending.popleft().result()
        finally:
            self.executor.shutdown(wait=True)
            self.pending.clear()


@contextlib.contextmanager
def pictures(device, vis_dir, ids, kitti_root=None, vis_thresh=0.7):
    """While the block runs, every frame sequence given to pipeline.detect_3d_stream (by test_net.run_split, say) also yields
    <vis_dir>/<id>.png, ids in the order of the frames.  Leaving the block waits for the pictures and raises the writer's first
    error; yields the PictureWriter."""
    writer = PictureWriter(device, vis_dir, ids, kitti_root, vis_thresh)
    plain = pipeline.detect_3d_stream

    def with_pictures(model, frames, *args, **kwargs):
        return writer.stream(lambda f: plain(model, f, *args, **kwargs), frames)

    pipeline.detect_3d_stream = with_pictures
    try:
        yield writer
    except BaseException:
        pipeline.detect_3d_stream = plain
        try:
            writer.close()
        except Exception:
            pass                            # the block's own error is the one to report
        raise
    else:
        pipeline.detect_3d_stream = plain
        writer.close()


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, add_help=False)
    ap.add_argument('--vis-dir', required=True, help='directory of the <id>.png pictures')
    ap.add_argument('--vis-thresh', type=float, default=0.7, help='score above which a detection is drawn (test_net.py:105)')
    ap.add_argument('--kitti-root', required=True)
    ap.add_argument('--split', required=True)
    args, rest = ap.parse_known_args(argv)
    rest += ['--kitti-root', args.kitti_root, '--split', args.split]          # everything but the two picture options goes to test_net
    rank, world, local = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1)), int(os.environ.get('LOCAL_RANK', 0))
    ids = images.read_split(args.split)
    mine = [ids[i] for i in shard_indices(len(ids), rank, world)]             # test_net.main's own sharding
    with pictures(torch.device('cuda', local), args.vis_dir, mine, args.kitti_root, args.vis_thresh) as writer:
        test_net.main(rest)
    print('[rank %d] %d pictures in %s' % (rank, writer.count, args.vis_dir), flush=True)


if __name__ == '__main__':
    main()
