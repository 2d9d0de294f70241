"""The host side of the KITTI image input, shared by the split driver (test_net.run_split), the training loader
(data.TrainLoader), the picture writer and the validator: split files, the PNG reader, the decode worker processes
(png_worker.py) and the page-locked ring the preprocessing kernels read where it is.  numpy only at import; torch is imported
when the ring allocates."""
import os

import numpy as np


def read_split(path):
    """The frame ids of a split file, one per line (blank lines are passed over)."""
    with open(path) as fh:
        return [ln.strip() for ln in fh if ln.strip()]


def read_png_rgb(path):
    """uint8 (H, W, 3) RGB.  (The reference reads BGR with cv2 and flips; the device preprocessing takes RGB.)"""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'), dtype=np.uint8)


class DecodeWorkers(object):
    """`n` png_worker.py processes and the shared file they decode into (one slot of two images per worker).  decode() hands a
    request to an idle worker and blocks the calling THREAD on its answer (a pipe read: no GIL held), then returns views of the
    worker's slot and the worker itself -- the caller copies the pixels out (into the page-locked ring) and release()s it."""

    def __init__(self, n, nbytes=3 * 512 * 1408):
        import mmap
        import queue
        import subprocess
        import sys
        import tempfile
        self.n, self.nbytes = n, nbytes
        base = '/dev/shm' if os.path.isdir('/dev/shm') and os.access('/dev/shm', os.W_OK) else tempfile.gettempdir()
        fd, self.path = tempfile.mkstemp(prefix='srcnn_png_', dir=base)
        os.ftruncate(fd, n * 2 * nbytes)
        self.mm = mmap.mmap(fd, 0)
        os.close(fd)
        self.view = np.frombuffer(self.mm, dtype=np.uint8)
        script = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'png_worker.py')
        self.procs, self.idle = [], queue.Queue()
        try:
            for i in range(n):
                self.procs.append(subprocess.Popen([sys.executable, script, self.path, str(i), str(nbytes)], stdin=subprocess.PIPE,
                                                   stdout=subprocess.PIPE, universal_newlines=True, bufsize=1))
            for i, pr in enumerate(self.procs):
                if pr.stdout.readline().strip() != 'ready':
                    raise RuntimeError('PNG decode worker %d did not start (exit code %s)' % (i, pr.poll()))
                self.idle.put(i)
        except Exception:
            self.close()
            raise
        os.unlink(self.path)              # every worker has it mapped: the file goes away with the last mapping
        self.path = None

    def decode(self, paths):
        import json
        i = self.idle.get()
        pr = self.procs[i]
        try:
            pr.stdin.write(json.dumps({'paths': list(paths)}) + '\n')
            pr.stdin.flush()
            line = pr.stdout.readline()
            if not line:
                raise RuntimeError('PNG decode worker %d died (exit code %s)' % (i, pr.poll()))
            reply = json.loads(line)
            if 'error' in reply:
                raise RuntimeError('PNG decode worker: %s' % reply['error'])
        except Exception:
            self.idle.put(i)
            raise
        base, out = i * 2 * self.nbytes, []
        for k, shape in enumerate(reply['shapes']):
            nb = int(np.prod(shape))
            out.append(self.view[base + k * self.nbytes: base + k * self.nbytes + nb].reshape(shape))
        return i, out

    def release(self, i):
        self.idle.put(i)

    def close(self):
        for pr in self.procs:
            try:
                pr.stdin.close()
            except Exception:
                pass
        for pr in self.procs:
            try:
                pr.wait(timeout=5)
            except Exception:
                pr.kill()
        self.procs = []
        if self.path:
            try:
                os.unlink(self.path)
            except OSError:
                pass
            self.path = None


_decode_workers = {}


def decode_workers(n):
    """The process-wide set of `n` decode workers (started on first use, reused by later splits, stopped at exit)."""
    w = _decode_workers.get(n)
    if w is None:
        import atexit
        w = _decode_workers[n] = DecodeWorkers(n)
        atexit.register(w.close)
    return w


def _page_locked(nbytes):
    import torch
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)


class PinnedPairs(object):
    """A ring of `n` page-locked uint8 (left, right) buffers the DEVICE reads where they are (round 6): a decode thread copies its
    two decoded images into an entry, and the preprocessing kernel reads them over the bus -- no hipMemcpy in any stream.  An
    asynchronous H2D copy per image looked free (0.35 ms of the loop thread per pair) and cost the streamed flow 1.0 ms per pair
    (profiles/flow3d_input_path_r06.txt: 5.9 ms with device-resident images or zero-copy, 6.9 with two H2D copies per frame, 8.5
    with the copies on a stream of their own) -- the copies, not their bytes.
    An entry is [left, right, event] and is rewritten only after its last reader: the reader leaves its event in the entry and
    entry() waits for it (data.TrainLoader), or sets none and makes the ring long enough (test_net.run_split).  grow=False: entries
    of 3 * 512 * 1408 bytes, a larger image is refused; grow=True: they start at 3 * 376 * 1242 bytes and are replaced on demand."""

    def __init__(self, n, grow=False):
        self.n, self.grow, self.nbytes = n, grow, 3 * 376 * 1242 if grow else 3 * 512 * 1408
        self.entries = [[None, None, None] for _ in range(n)]       # left, right, event of the last reader

    def entry(self, j):
        e = self.entries[j % self.n]
        if e[2] is not None:
            e[2].synchronize()
            e[2] = None
        return e

    def put(self, e, k, arr):
        """Copies `arr` into buffer `k` (0 left, 1 right) of entry `e`; returns the page-locked view of its shape."""
        arr = np.ascontiguousarray(arr, dtype=np.uint8)
        if e[k] is None or e[k].numel() < arr.nbytes:
            assert self.grow or arr.nbytes <= self.nbytes, "image larger than the staging ring's entries"
            e[k] = _page_locked(max(arr.nbytes, self.nbytes))
        view = e[k][:arr.nbytes].view(*arr.shape)
        np.copyto(view.numpy(), arr)
        return view
