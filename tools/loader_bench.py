"""The training loader's batch assembly and sustained rate, at KITTI's 375 x 1242.

    python tools/loader_bench.py [--out profiles/loader_bench.txt] [--reps 40] [--pairs 32]

1. One batch assembly for B = 1 and B = 4, device-resident uint8 pairs and a device-resident ground-truth table, whole calls
   between device events, versions ALTERNATING, 5 untimed runs first, medians of --reps runs with min and max:
     * fused : engine.preprocess_train + engine.gt_batch (csrc/loader.hip: two launches per batch);
     * eager : the same result from torch ops on the device -- fixture.preprocess's route (channel flip, float32 minus the means,
       F.interpolate bilinear, zero padding into the batch blob) per image, and the torch composition of the ground-truth rows
       (scale, clamp, mask, argsort of the keys, index, pad).  Eager's resize is torch's, not OpenCV's: it is a yardstick for time,
       its pixels differ in the last bits.
   Bytes the kernels have to move: 2 B x (3 x 600 x 1987 x 4 written + 375 x 1242 x 3 read) plus the ground-truth rows; GB/s =
   those bytes over the median, beside the 6.3 TB/s copy ceiling (layer_table.py's peak).
2. The loader's sustained rate: --pairs synthetic 375 x 1242 PNG pairs (fixture.synthetic_pair) written to a temporary directory,
   TrainLoader at batch size 1, a consumer that only waits for each batch on its stream; one untimed epoch, then one timed one
   (host clock around work that ends in a synchronise), at workers 0 and 4.
3. training.train_step on the same box: R-101, one 600 x 1987 pair from that loader, cfg.TRAIN.RPN_PRE_NMS_TOP_N = 8192, 2 untimed
   and 5 timed steps, host clock around steps that end in a synchronise.  The last line says whether the loader with a no-op
   consumer outruns it.
Runner and timer: tools/benchlib.py."""
import os
import tempfile
import time

import benchlib

HBM_COPY_CEILING_TBS = 6.3
H, W, TARGET = 375, 1242, 600
CALIB = ("P0: 721.5377 0 609.5593 0 0 721.5377 172.854 0 0 0 1 0\nP1: 721.5377 0 609.5593 -387.5744 0 721.5377 172.854 0 0 0 1 0\n"
         "P2: 721.5377 0 609.5593 44.85728 0 721.5377 172.854 0.2163791 0 0 1 0.002745884\n"
         "P3: 721.5377 0 609.5593 -339.5242 0 721.5377 172.854 2.199936 0 0 1 0.002729905\n"
         "R0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 0 -1 0 0 0 0 -1 0 1 0 0 0\nTr_imu_to_velo: 1 0 0 0 0 1 0 0 0 0 1 0\n")
LABEL = ("Car 0.00 0 -1.58 0 0 50 50 1.52 1.63 3.88 -3.20 1.62 17.50 -1.76\nCar 0.00 1 1.85 0 0 50 50 1.47 1.60 4.12 4.62 1.71 24.30 2.04\n"
         "Car 0.00 0 0.40 0 0 50 50 1.55 1.67 3.64 9.30 1.58 21.00 0.81\n")


def write_dataset(root, pairs):
    from PIL import Image
    from stereo_rcnn_amd import fixture
    base = os.path.join(root, 'training')
    for d in ('image_2', 'image_3', 'label_2', 'calib'):
        os.makedirs(os.path.join(base, d))
    ids = ['%06d' % i for i in range(pairs)]
    for i, fid in enumerate(ids):
        l, r = fixture.synthetic_pair(100 + i, H, W)
        Image.fromarray(l).save(os.path.join(base, 'image_2', fid + '.png'))
        Image.fromarray(r).save(os.path.join(base, 'image_3', fid + '.png'))
        open(os.path.join(base, 'label_2', fid + '.txt'), 'w').write(LABEL)
        open(os.path.join(base, 'calib', fid + '.txt'), 'w').write(CALIB)
    split = os.path.join(root, 'train.txt')
    open(split, 'w').write('\n'.join(ids))
    return split


def eager_batch(pairs, flipped, scale, table, slots, keys, K):
    """The eager route on the device (see the module docstring)."""
    import torch
    import torch.nn.functional as F
    dev = table.device
    means = torch.tensor([102.9801, 115.9465, 122.7717], dtype=torch.float64, device=dev).view(3, 1, 1)
    ims = [[], []]
    for (l, r), f in zip(pairs, flipped):
        if f:
            l, r = r.flip(1), l.flip(1)
        for k, im in enumerate((l, r)):
            t = (im.permute(2, 0, 1).flip(0).double() - means).float().unsqueeze(0)
            ims[k].append(F.interpolate(t, scale_factor=scale, mode='bilinear', align_corners=False, recompute_scale_factor=False))
    Hm, Wm = max(t.shape[2] for t in ims[0]), max(t.shape[3] for t in ims[0])
    blobs = []
    for k in range(2):
        blob = torch.zeros((len(pairs), 3, Hm, Wm), dtype=torch.float32, device=dev)
        for b, t in enumerate(ims[k]):
            blob[b, :, :t.shape[2], :t.shape[3]] = t[0]
        blobs.append(blob)
    outs = [torch.zeros((len(slots), K, c), dtype=torch.float32, device=dev) for c in (5, 5, 5, 5, 6)]
    for b, (r0, n, s, wd) in enumerate(slots):
        rows = table[r0:r0 + n][torch.argsort(keys[b, :n].long() & 0xFFFFFFFF, stable=True)][:K]
        m = rows.shape[0]
        for g in range(3):
            box = rows[:, 4 * g:4 * g + 4] * s
            box[:, 0] = torch.clamp(box[:, 0], max=wd)
            outs[g][b, :m, :4], outs[g][b, :m, 4] = box, rows[:, 23]
        outs[3][b, :m] = rows[:, 12:17]
        kp = rows[:, 17:23] * s
        outs[4][b, :m] = torch.where((kp < 0) | (kp > wd - 1), torch.full_like(kp, -1.0), kp)
    return blobs, outs


def child(reps, pairs):
    import numpy as np
    import torch
    from stereo_rcnn_amd import _lib, data, engine, fixture, training
    from stereo_rcnn_amd.datasets import kitti
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    from stereo_rcnn_amd.model.utils.config import cfg
    dev = benchlib.device()
    K = int(cfg.MAX_NUM_GT_BOXES)
    with tempfile.TemporaryDirectory() as root:
        split = write_dataset(root, pairs)
        roidb, _, ratio_index = kitti.build_roidb(root, split)
        print('%d synthetic %d x %d PNG pairs, %d roidb entries (flipped copies included), %d objects each'
              % (pairs, H, W, len(roidb), len(roidb[0]['boxes_left'])))
        table_np, off = data.pack_gt_table(roidb)
        table = torch.from_numpy(table_np).to(dev)
        scale = float(TARGET) / H

        # ---- 1. one batch assembly
        print('\n1. one batch assembly, device-resident inputs (us between device events; %d runs each, alternating)' % reps)
        print('%-3s %-6s %10s %10s %10s %14s %8s %s' % ('B', 'route', 'median', 'min', 'max', 'bytes counted', 'GB/s',
                                                        'share of the %.1f TB/s copy ceiling' % HBM_COPY_CEILING_TBS))
        for B in (1, 4):
            imgs = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev).contiguous() for a in fixture.synthetic_pair(7 + b, H, W)) for b in range(B)]
            flipped = [b % 2 == 1 for b in range(B)]
            n = [int(off[b + 1] - off[b]) for b in range(B)]
            keys = torch.randint(0, 2 ** 31, (B, max(n)), dtype=torch.int32, device=dev)
            slots = [(int(off[b]), n[b], scale, 1987.0) for b in range(B)]
            routes = {'fused': lambda: (engine.preprocess_train(imgs, flipped, [scale] * B, 2484), engine.gt_batch(table, slots, keys, K)),
                      'eager': lambda: eager_batch(imgs, flipped, scale, table, slots, keys, K)}
            nbytes = 2 * B * (3 * 600 * 1987 * 4 + H * W * 3) + sum(n) * _lib.GT_COLS * 4 + B * K * 26 * 4
            times = benchlib.alternating(list(routes.items()), reps, warmup=5, sync_before=True)
            for k in routes:
                med, lo, hi = (t * 1e3 for t in benchlib.stats(times[k]))
                gbs = nbytes / (med * 1e-6) / 1e9
                print('%-3d %-6s %10.1f %10.1f %10.1f %14d %8.0f %.1f %%' % (B, k, med, lo, hi, nbytes, gbs,
                                                                            100.0 * gbs / (HBM_COPY_CEILING_TBS * 1e3)))
            print('    least time for those bytes at the copy ceiling: %.1f us' % (nbytes / (HBM_COPY_CEILING_TBS * 1e12) * 1e6))

        # ---- 2. the loader's sustained rate
        print('\n2. TrainLoader, batch size 1, prefetch 2, a consumer that only waits for the batch (one warm epoch, one timed)')
        rates = {}
        for workers in (0, 4):
            loader = data.TrainLoader(roidb, ratio_index, 1, dev, generator=torch.Generator().manual_seed(1), workers=workers, prefetch=2)
            try:
                for _ in loader:
                    torch.cuda.current_stream().synchronize()
                t0 = time.perf_counter()
                count = 0
                for _ in loader:
                    torch.cuda.current_stream().synchronize()
                    count += 1
                dt = time.perf_counter() - t0
            finally:
                loader.close()
            rates[workers] = count / dt
            print('workers %d: %d pairs in %.3f s = %.1f pairs/s' % (workers, count, dt, rates[workers]))

        # ---- 3. train_step on the same box
        print('\n3. training.train_step, R-101, one 600 x 1987 pair, RPN_PRE_NMS_TOP_N 8192 (2 warm steps, 5 timed)')
        cfg.TRAIN.RPN_PRE_NMS_TOP_N = 8192
        loader = data.TrainLoader(roidb, ratio_index, 1, dev, generator=torch.Generator().manual_seed(1), workers=0)
        batch = next(iter(loader))
        model = resnet(kitti.CLASSES, 101)
        model.create_architecture()
        model.load_state_dict(fixture.make_state_dict(3))
        model.to(dev)
        uncert = torch.full((6,), -1.0, device=dev, requires_grad=True)
        opt = training.make_optimizer(model, uncert)
        gen = torch.Generator(device=dev).manual_seed(2)
        steps = []
        for i in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            training.train_step(model, opt, uncert, batch, clip_norm=10., generator=gen)
            torch.cuda.synchronize()
            if i >= 2:
                steps.append(time.perf_counter() - t0)
        step = float(np.median(steps))
        print('train_step: median %.1f ms (min %.1f, max %.1f) = %.2f pairs/s' % (step * 1e3, min(steps) * 1e3, max(steps) * 1e3, 1.0 / step))
        for workers in (0, 4):
            print('loader with a no-op consumer, workers %d: %.1f pairs/s = %.1f x the train_step rate -> %s'
                  % (workers, rates[workers], rates[workers] * step,
                     'the loader outruns the step' if rates[workers] * step > 1.0 else 'the loader is the bottleneck'))


def main():
    benchlib.main(__file__, child, out='loader_bench.txt', reps=40, timeout=420, extra=[('--pairs', dict(type=int, default=32))],
                  header='# python tools/loader_bench.py --reps %(reps)d --pairs %(pairs)d   (see the tool for what each line measures)')


if __name__ == '__main__':
    main()
