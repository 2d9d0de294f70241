"""The training data loader: roidb entries in, forward_train's nine inputs out.

The per-iteration half of the reference's data path (lib/roi_data_layer/minibatch.py, roibatchLoader.py, lib/model/utils/blob.py and
the sampler of trainval_net.py:81-101).  The roidb comes from stereo_rcnn_amd.datasets.kitti.build_roidb (host, once); here its
ground truth is packed once into a device table (pack_gt_table), PNG pairs are decoded by worker processes (png_worker.py: numpy
and PIL only, they never open the GPU) into page-locked buffers, and a batch is two launches of csrc/loader.hip on a side stream:
engine.preprocess_train (flip, mean, OpenCV's INTER_LINEAR, zero padding, reading the page-locked images where they are) and
engine.gt_batch (scale, clamp, mask, shuffle, truncate, pad).  Nothing is read back from the device.

Batches.  With batch_size 1 every tensor equals the reference's.  The reference's default collate cannot batch KITTI's four image
sizes; here, with batch_size > 1, the images of a batch are zero-padded to the batch maximum (as blob.im_list_to_blob would),
each im_info row carries ITS image's resized height, width (after the MAX_SIZE crop) and scale, and the x1 / keypoint clamps of
an image's ground truth use that image's own width.

Randomness.  Everything random comes from `generator` (a CPU torch.Generator), drawn on the caller's thread in visit order: the
epoch's torch.randperm (BatchSampler), then per sample the index into cfg.TRAIN.SCALES (minibatch.py:27) and one uint32 shuffle
key per object (np.random.shuffle of roibatchLoader.py:75 as a sort by (key, index)).  `draws` replays recorded ones instead:
{'order': positions (optional), 'scale_inds': one per visited sample, 'keys': per visited sample a tensor of n keys}.  The
number of decode workers has no influence on any result.
"""
import collections
import math

import numpy as np
import torch

from . import _lib, engine
from .images import DecodeWorkers, PinnedPairs, read_png_rgb
from .model.utils.config import cfg


def pack_gt_table(roidb):
    """(table (rows, GT_COLS) float32, offsets (len(roidb) + 1) int64): per object with a non-zero class (minibatch.py:43) left box,
    right box, merge box, dim w h l, sin(alpha), cos(alpha), kpts, class.  sin / cos: math.sin / math.cos of the float32 angle
    widened to double, stored as float32 -- what minibatch.py:68-69 computes on every call."""
    rows, offsets = [], [0]
    for e in roidb:
        inds = np.where(e['gt_classes'] != 0)[0]
        t = np.empty((len(inds), _lib.GT_COLS), dtype=np.float32)
        t[:, 0:4] = e['boxes_left'][inds]
        t[:, 4:8] = e['boxes_right'][inds]
        t[:, 8:12] = e['boxes_merge'][inds]
        t[:, 12:15] = e['dim_orien'][inds][:, 0:3]
        for i, k in enumerate(inds):
            t[i, 15] = math.sin(e['dim_orien'][k, 3])
            t[i, 16] = math.cos(e['dim_orien'][k, 3])
        t[:, 17:23] = e['kpts'][inds]
        t[:, 23] = e['gt_classes'][inds]
        rows.append(t)
        offsets.append(offsets[-1] + len(inds))
    table = np.concatenate(rows, 0) if rows else np.zeros((0, _lib.GT_COLS), dtype=np.float32)
    return np.ascontiguousarray(table), np.asarray(offsets, dtype=np.int64)


class BatchSampler(object):
    """The index order of trainval_net.py:81-101: torch.randperm over the whole batches, each batch its batch_size consecutive
    positions, the leftover positions appended in order."""

    def __init__(self, train_size, batch_size, generator=None):
        self.num_data, self.batch_size, self.generator = int(train_size), int(batch_size), generator
        self.num_per_batch = int(train_size / batch_size)

    def __iter__(self):
        return iter(self.order().tolist())

    def order(self):
        rng = torch.arange(0, self.batch_size).view(1, self.batch_size).long()
        rand_num = torch.randperm(self.num_per_batch, generator=self.generator).view(-1, 1) * self.batch_size
        out = (rand_num.expand(self.num_per_batch, self.batch_size) + rng).reshape(-1)
        if self.num_data % self.batch_size:
            out = torch.cat((out, torch.arange(self.num_per_batch * self.batch_size, self.num_data).long()), 0)
        return out

    def __len__(self):
        return self.num_data


def keys_to_words(keys):
    """uint32 keys given as a non-negative integer tensor -> the same words in an int32 tensor (torch has no uint32 arithmetic)."""
    return torch.from_numpy((keys.to(torch.int64).numpy() & 0xFFFFFFFF).astype(np.uint32).view(np.int32))


class TrainLoader(object):
    """Iterator over one epoch at a time: `for batch in loader` yields (im_left, im_right, im_info, gt_boxes_left, gt_boxes_right,
    gt_boxes_merge, gt_dim_orien, gt_kpts, num_boxes) -- images float32 (B, 3, H, W) and ground truth (B, MAX_NUM_GT_BOXES, 5|5|5|5|6)
    on `device`, num_boxes int64 (B) on `device`, im_info float32 (B, 3) on the CPU (train_step's one host read never waits).
    roidb / ratio_index: datasets.kitti.build_roidb; sample position p of the sampler is roidb[ratio_index[p]].
    workers: PNG decode processes (0 = decode on the calling thread; at most 16); prefetch: batches assembled ahead on a side
    stream, an event ordering each before the consumer's stream.  The last batch of an epoch holds the leftover samples.
    `visited` lists the roidb indices of the batches yielded so far in the current epoch."""

    def __init__(self, roidb, ratio_index, batch_size, device, generator=None, workers=4, prefetch=2, draws=None):
        assert 0 < batch_size <= _lib.LOADER_MAX_BATCH, "batch_size must be 1..%d" % _lib.LOADER_MAX_BATCH
        self.roidb, self.ratio_index = roidb, [int(i) for i in ratio_index]
        self.batch_size, self.device = int(batch_size), torch.device(device)
        self.generator = generator if generator is not None else torch.Generator().manual_seed(int(cfg.RNG_SEED))
        self.n_workers, self.prefetch = max(0, min(int(workers), 16)), max(0, int(prefetch))
        self.draws = draws
        table, offsets = pack_gt_table(roidb)
        self.table = torch.from_numpy(table).to(self.device)
        self.offsets = offsets
        self.sampler = BatchSampler(len(roidb), self.batch_size, self.generator)
        self.depth = max(1, self.prefetch)
        self.ring, self.taken = PinnedPairs((2 * self.depth + 2) * self.batch_size, grow=True), 0
        self.side = torch.cuda.Stream(device=self.device)
        self.workers = self.pool = None
        self.visited = []

    def __len__(self):
        return -(-len(self.roidb) // self.batch_size)

    # ---- decode
    def _start_workers(self):
        if self.n_workers and self.workers is None:
            import concurrent.futures as cf
            self.workers = DecodeWorkers(self.n_workers)
            self.pool = cf.ThreadPoolExecutor(max_workers=self.n_workers)

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None
        if self.workers is not None:
            self.workers.close()
            self.workers = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _decode(self, entry, slot):
        paths = (entry['img_left'], entry['img_right'])
        if self.workers is None:
            return [self.ring.put(slot, k, read_png_rgb(p)) for k, p in enumerate(paths)]
        w, arrs = self.workers.decode(paths)          # this thread sleeps on the worker's pipe meanwhile
        try:
            return [self.ring.put(slot, k, a) for k, a in enumerate(arrs)]
        finally:
            self.workers.release(w)

    # ---- one batch
    def _schedule(self, positions, cursor):
        """Draws of the batch (on this thread, in visit order) and its decodes (submitted)."""
        scales_cfg = cfg.TRAIN.SCALES
        items = []
        for p in positions:
            idx = self.ratio_index[p]
            e = self.roidb[idx]
            n = int(self.offsets[idx + 1] - self.offsets[idx])
            if self.draws is not None:
                si, keys = int(self.draws['scale_inds'][cursor]), self.draws['keys'][cursor]
            else:
                si = int(torch.randint(0, len(scales_cfg), (1,), generator=self.generator))
                keys = torch.randint(0, 2 ** 32, (n,), dtype=torch.int64, generator=self.generator)
            assert int(keys.numel()) == n, "one shuffle key per object"
            cursor += 1
            slot = self.ring.entry(self.taken)           # waits for the batch that last read this entry, if it is still running
            self.taken += 1
            job = self.pool.submit(self._decode, e, slot) if self.pool is not None else self._decode(e, slot)
            items.append((idx, e, n, scales_cfg[si], keys_to_words(keys), slot, job))
        return items, cursor

    def _assemble(self, items):
        B = len(items)
        pairs, flipped, scales = [], [], []
        for idx, e, n, target, keys, slot, job in items:
            l, r = job.result() if hasattr(job, 'result') else job
            assert tuple(l.shape) == tuple(r.shape), "left and right image of %s differ in size" % e['img_left']
            pairs.append((l, r))
            flipped.append(bool(e['flipped']))
            scales.append(float(target) / float(min(int(l.shape[0]), int(l.shape[1]))))       # blob.py:49-51
        stride = max(1, max(it[2] for it in items))
        keys_host = torch.zeros((B, stride), dtype=torch.int32, pin_memory=True)
        for b, it in enumerate(items):
            keys_host[b, :it[2]] = it[4]
        with torch.cuda.stream(self.side):
            im_left, im_right, sizes = engine.preprocess_train(pairs, flipped, scales, int(cfg.TRAIN.MAX_SIZE), device=self.device)
            keys_dev = keys_host.to(self.device, non_blocking=True)
            slots = [(int(self.offsets[it[0]]), it[2], scales[b], float(sizes[b][1])) for b, it in enumerate(items)]
            gt = engine.gt_batch(self.table, slots, keys_dev, int(cfg.MAX_NUM_GT_BOXES))
            ev = torch.cuda.Event()
            ev.record(self.side)
        for it in items:
            it[5][2] = ev                                      # the ring entries are free again once this batch was assembled
        im_info = torch.tensor([[float(oh), float(ow), s] for (oh, ow), s in zip(sizes, scales)], dtype=torch.float32)
        return [it[0] for it in items], ev, [im_left, im_right, im_info] + gt, keys_dev

    def __iter__(self):
        self._start_workers()
        self.visited = []
        if self.draws is not None and self.draws.get('order') is not None:
            order = [int(v) for v in self.draws['order']]
        else:
            order = self.sampler.order().tolist()
        B = self.batch_size
        batches = collections.deque(order[i:i + B] for i in range(0, len(order), B))
        sched, ready, cursor = collections.deque(), collections.deque(), 0
        while batches or sched or ready:
            while batches and len(sched) < self.depth:
                items, cursor = self._schedule(batches.popleft(), cursor)
                sched.append(items)
            while sched and len(ready) < self.depth:
                ready.append(self._assemble(sched.popleft()))
                while batches and len(sched) < self.depth:
                    items, cursor = self._schedule(batches.popleft(), cursor)
                    sched.append(items)
            ids, ev, batch, keys_dev = ready.popleft()
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            for t in batch + [keys_dev]:
                if t.is_cuda:
                    t.record_stream(cur)                       # allocated on the side stream, consumed on this one
            self.visited.append(ids)
            yield tuple(batch)
