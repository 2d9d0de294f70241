"""The result picture of one KITTI-sized pair, on the device and composed on the host.

    python tools/overlay_bench.py [--out profiles/overlay_bench.txt] [--reps 40]

375 x 1242 images, a record of 40 aligned objects (2-D boxes, wireframes, bird's-eye boxes: 1040 live segments of 7800 slots at
max_det 300) and a 120 000-point velodyne cloud, all device-resident.  Whole calls, the two routes ALTERNATING, 5 untimed runs
first, medians of --reps runs with min and max:
  * device : engine.bev_lidar + engine.render_overlay (csrc/overlay.hip: a memset and three launches), between device events;
             the panel stays on the device.  Also each of the two calls alone.
  * host   : the same panel composed with numpy and PIL ImageDraw from a record ALREADY on the host -- the device -> host copy of
             the two images (which the device route avoids) is inside the time, the record's is not; host clock around work that
             starts and ends synchronised.  PIL's lines are not this project's rasterisation rule: the host route is a yardstick
             for time, its pixels differ along slanted lines.
Bytes the device route has to move: the two images read (2 x 375 x 1242 x 3) + the points read (120 000 x 16) + the plane
written and read (2 x 750 x 428) + the panel written (750 x 1670 x 3); GB/s = those bytes over the median, beside the 6.3 TB/s
copy ceiling (layer_table.py's peak).  No ratio is claimed in advance: the file records what was measured.
Runner and timer: tools/benchlib.py."""
import math
import time

import benchlib

HBM_COPY_CEILING_TBS = 6.3
H, W, OBJECTS, POINTS, MAX_DET = 375, 1242, 40, 120000, 300
P2 = ((721.5377, 0, 609.5593, 44.85728), (0, 721.5377, 172.854, 0.2163791), (0, 0, 1, 0.002745884))
VELO = ((0.0, -1.0, 0.0, 0.06), (0.0, 0.0, -1.0, -0.08), (1.0, 0.0, 0.0, -0.27))


def make_record(np):
    rng = np.random.default_rng(1)
    rec = np.zeros((MAX_DET + 1, 32), np.float32)
    rec[0, 0] = OBJECTS
    for i in range(OBJECTS):
        x, y, z, th = rng.uniform(-12, 12), rng.uniform(1.2, 1.8), rng.uniform(8, 60), rng.uniform(-math.pi, math.pi)
        u, v, s = 721.5 * x / z + 609.6, 721.5 * (y - 0.8) / z + 172.9, 721.5 / z
        r = rec[1 + i]
        r[0] = rng.uniform(0.75, 1.0)
        r[1:5] = (u - 1.5 * s, v - 0.9 * s, u + 1.5 * s, v + 0.9 * s)
        r[5:9] = r[1:5] - np.float32([388.0 / z, 0, 388.0 / z, 0])
        r[9:12] = (rng.uniform(1.5, 1.9), rng.uniform(1.4, 1.7), rng.uniform(3.4, 4.6))
        r[20], r[25] = 1.0, 1.0
        r[21:25] = r[27:31] = (x, y, z, th)
    return rec


def host_panel(np, left, right, rec, pts, vis_thresh=0.7):
    """numpy + PIL ImageDraw: the reference's flow (demo.py:225-333) with PIL in cv2's place."""
    from PIL import Image, ImageDraw
    from stereo_rcnn_amd import engine
    res, x_max, y_max, x_off, y_off = engine.bev_geometry(H)
    m = np.asarray(VELO)
    cam = pts[:, :3].astype(np.float64) @ m[:, :3].T + m[:, 3]
    keep = (cam[:, 2] > 0) & (cam[:, 2] < 70) & (cam[:, 0] > -20) & (cam[:, 0] < 20)
    xi = np.minimum((cam[keep, 0] / res).astype(np.int32) - x_off, x_max - 1)
    yi = np.minimum((-cam[keep, 2] / res).astype(np.int32) + y_off, y_max - 1)
    plane = np.full((y_max, x_max), 255, np.uint8)
    plane[yi, xi] = 100
    ims = [Image.fromarray(left), Image.fromarray(right), Image.fromarray(np.repeat(plane[:, :, None], 3, axis=2))]
    draw = [ImageDraw.Draw(im) for im in ims]
    p2 = np.asarray(P2)[:, :3]
    n = int(rec[0, 0])
    for r in rec[1:1 + min(n, 100)]:
        if r[0] > vis_thresh:
            for k in (0, 1):
                b = [int(np.round(v)) for v in r[1 + 4 * k:5 + 4 * k]]
                draw[k].rectangle(b, outline=(204, 0, 0), width=1)
    for r in rec[1:1 + n]:
        if not (r[0] > vis_thresh and r[25] > 0):
            continue
        w, h, l = [float(v) for v in r[9:12]]
        pos, c, s = r[27:30].astype(np.float64), math.cos(float(r[30])), math.sin(float(r[30]))
        rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        corners = [pos + rot.dot(v) / 2.0 for v in ([-w, 0, -l], [-w, 0, l], [w, 0, l], [w, 0, -l], [-w, -2 * h, -l], [-w, -2 * h, l],
                                                    [w, -2 * h, l], [w, -2 * h, -l])]
        bev = [(int(p[0] / res) - x_off, int(-p[2] / res) + y_off) for p in corners[:4] + [pos + rot.dot([0, 0, l * 2 / 3])]]
        for i, j in ((0, 1), (1, 2), (2, 3), (0, 3), (1, 4), (2, 4)):
            draw[2].line([bev[i], bev[j]], fill=(0, 200, 0), width=2)
        if any(p[2] < 0 for p in corners):
            continue
        px = []
        for p in corners:
            q = p2.dot(p)
            px.append((int(q[0] / q[2]), int(q[1] / q[2])))
        for i, j in ((0, 1), (1, 2), (2, 3), (0, 3), (4, 5), (5, 6), (6, 7), (7, 4), (4, 0), (5, 1), (6, 2), (7, 3)):
            draw[0].line([px[i], px[j]], fill=(0, 200, 0), width=1)
    both = np.concatenate((np.asarray(ims[0]), np.asarray(ims[1])), axis=0)
    return np.concatenate((both, np.asarray(ims[2])), axis=1)


def child(reps):
    import numpy as np
    import torch
    from stereo_rcnn_amd import _lib, engine, fixture
    dev = benchlib.device()
    print('device: %s' % torch.cuda.get_device_name(0))
    left_np, right_np = fixture.synthetic_pair(7, H, W)
    rec_np = make_record(np)
    rng = np.random.default_rng(2)
    pts_np = np.stack((rng.uniform(0, 80, POINTS), rng.uniform(-25, 25, POINTS), rng.uniform(-2, 1, POINTS), rng.uniform(0, 1, POINTS)),
                      axis=1).astype(np.float32)
    left, right, rec, pts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (left_np, right_np, rec_np, pts_np)]
    res, x_max, y_max, _, _ = engine.bev_geometry(H)
    plane = torch.empty((y_max, x_max), dtype=torch.uint8, device=dev)
    panel = torch.empty((2 * H, W + x_max, 3), dtype=torch.uint8, device=dev)
    velo = np.asarray(VELO)

    def device_route():
        engine.bev_lidar(pts, velo, H, out=plane)
        engine.render_overlay(left, right, rec, P2, 0.7, plane, out=panel)

    def host_clock(fn, inner, sync_before):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    routes = [('device', device_route),
              ('lidar', lambda: engine.bev_lidar(pts, velo, H, out=plane)),
              ('render', lambda: engine.render_overlay(left, right, rec, P2, 0.7, plane, out=panel)),
              ('host', lambda: host_panel(np, left.cpu().numpy(), right.cpu().numpy(), rec_np, pts_np), host_clock)]
    times = {k: [t * 1e3 for t in v] for k, v in benchlib.alternating(routes, reps, warmup=5, sync_before=True).items()}      # us
    got, want = panel.cpu().numpy(), host_panel(np, left_np, right_np, rec_np, pts_np)
    print('%d x %d pair, %d aligned objects of max_det %d (%d segment slots), %d lidar points, panel %d x %d'
          % (H, W, OBJECTS, MAX_DET, MAX_DET * _lib.OVERLAY_SLOTS_PER_ROW, POINTS, got.shape[0], got.shape[1]))
    print('pixels where the device panel and the PIL panel differ (another line rule, not an error): %d of %d; outside the drawn '
          'lines of either: %d' % (int((got != want).any(2).sum()), got.shape[0] * got.shape[1],
                                   int(((got != want).any(2) & ~(((got == (0, 200, 0)).all(2)) | ((want == (0, 200, 0)).all(2))
                                                                | ((got == (204, 0, 0)).all(2)) | ((want == (204, 0, 0)).all(2)))).sum())))
    nbytes = {'device': 2 * H * W * 3 + POINTS * 16 + 2 * y_max * x_max + 2 * H * (W + x_max) * 3,
              'lidar': POINTS * 16 + y_max * x_max, 'render': 2 * H * W * 3 + y_max * x_max + 2 * H * (W + x_max) * 3}
    print('\nus per call (%d runs each, alternating; device routes between device events, host route on the host clock)' % reps)
    print('%-7s %10s %10s %10s %14s %8s %s' % ('route', 'median', 'min', 'max', 'bytes counted', 'GB/s',
                                                'share of the %.1f TB/s copy ceiling' % HBM_COPY_CEILING_TBS))
    for k in times:
        med = float(np.median(times[k]))
        if k in nbytes:
            gbs = nbytes[k] / (med * 1e-6) / 1e9
            print('%-7s %10.1f %10.1f %10.1f %14d %8.1f %.2f %%' % (k, med, min(times[k]), max(times[k]), nbytes[k], gbs,
                                                                  100.0 * gbs / (HBM_COPY_CEILING_TBS * 1e3)))
        else:
            print('%-7s %10.1f %10.1f %10.1f %14s %8s' % (k, med, min(times[k]), max(times[k]), '-', '-'))
    print('host median / device median: %.1f' % (float(np.median(times['host'])) / float(np.median(times['device']))))
    print('least time for the device route\'s bytes at the copy ceiling: %.2f us' % (nbytes['device'] / (HBM_COPY_CEILING_TBS * 1e12) * 1e6))


def main():
    benchlib.main(__file__, child, out='overlay_bench.txt', reps=40, timeout=240,
                  header='# python tools/overlay_bench.py --reps %(reps)d   (see the tool for what each line measures)')


if __name__ == '__main__':
    main()
