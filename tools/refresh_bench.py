"""What it costs to bring an inference plan up to trained parameters (R-101, one 600 x 1987 pair, f16x3 engine, recorded program):

  (a) rebuild   Weights(model.state_dict(), dev) + Plan(...) + first run   -- the eager path: new buffers, ~150 host reads
  (b) refresh   Plan.refresh(model) + first run                            -- srcnn_prep_weights in place, one host read
  (c) kernel    srcnn_prep_weights alone, GB/s over the bytes it must move (sources read once; weight, hi, lo written once)

Whole calls, wall clock around a device synchronisation AND between device events, the sides alternating; the parameters move by a
factor of 1 + 1e-4 before every measurement so that each side sees new values (no layer's scale crosses a power of two: the
recorded program survives the refresh; the first run of (b) still re-calibrates the activation scales, as (a)'s does).
Every call is timed, the first included, so there is no warm-up to discard.  Runner and device-event window: tools/benchlib.py.

    python tools/refresh_bench.py [--reps 3] [--out profiles/refresh_bench.txt]
"""
import time

import torch

import benchlib


def child(reps):
    from stereo_rcnn_amd import engine
    from stereo_rcnn_amd.model.stereo_rcnn.plan import Plan, Weights
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    dev = benchlib.device()
    torch.manual_seed(3)
    model = resnet(('__background__', 'Car'), 101, pretrained=False)
    model.create_architecture()
    model.to(dev).eval()
    H, W = 600, 1987
    g = torch.Generator().manual_seed(5)
    inputs = (torch.randn(1, 3, H, W, generator=g).to(dev) * 50, torch.randn(1, 3, H, W, generator=g).to(dev) * 50,
              torch.tensor([[H, W, 1.6]], device=dev))

    def first_run(p):
        p.set_inputs(*inputs)
        p.run(precision='f16x3', use_program=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        devt = benchlib.window(fn)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, devt

    def move():
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(1.0001)

    plan = Plan(Weights(model.state_dict(), dev), 1, H, W)
    first_run(plan)                                   # tunes the conv plans, splits every weight, calibrates, records
    first_run(plan)
    w = plan.w
    sd = w._on_device(model.state_dict(), dev)
    index = {e['name']: i for i, e in enumerate(w.prepared.table)}
    specs = [w._spec(e, sd, index) for e in w.prepared.table]
    elems = sum(s.dst_w.numel() for s in specs if s.alias_of < 0)
    split = sum(s.dst_hi.numel() for s in specs if s.dst_hi is not None)
    nbytes = elems * 8 + split * 4                    # float32 in, float32 out; hi and lo out
    rows = {'a': [], 'b': [], 'c': []}
    reports = []
    for _ in range(reps):
        move()
        rows['a'].append(timed(lambda: first_run(Plan(Weights(model.state_dict(), dev), 1, H, W))))
        move()

        def refresh():
            reports.append(plan.refresh(model))
            first_run(plan)
        rows['b'].append(timed(refresh))
        rows['c'].append(timed(lambda: engine.prep_weights_into(specs)))
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ['refresh_bench: R-101, 1 x 600 x 1987 pair, f16x3 engine with recorded program, %s, %d repetitions, sides alternating'
             % (torch.cuda.get_device_name(0), reps),
             'regime: one process, one stream, nothing else in flight; whole calls; wall = host clock around a device sync, dev = device events',
             '%d prepared layers, %.1f M weight elements, %.1f M of them split to hi / lo' % (len(specs), elems / 1e6, split / 1e6)]
    for key, what in (('a', 'rebuild: Weights + Plan + first run'), ('b', 'refresh: Plan.refresh + first run'), ('c', 'srcnn_prep_weights alone')):
        wall, devt = [r[0] for r in rows[key]], [r[1] for r in rows[key]]
        lines.append('(%s) %-38s wall median %9.2f ms  (all: %s)   dev median %9.2f ms' % (key, what, med(wall), ' '.join('%.1f' % v for v in wall), med(devt)))
    t = med([r[1] for r in rows['c']]) * 1e-3
    lines.append('(c) moves %.1f MB compulsory -> %.0f GB/s = %.1f %% of the 6.3 TB/s copy ceiling' % (nbytes / 1e6, nbytes / t / 1e9, nbytes / t / 6.3e12 * 100))
    lines.append('refresh reports: %d scale changes, programs dropped in %d of %d' % (sum(len(r['scale_changed']) for r in reports),
                                                                                   sum(r['programs_dropped'] for r in reports), len(reports)))
    print('\n'.join(lines))


def main():
    # the time limit: a run with the default arguments took 7 s on a warm box; the room is for a first run (train_step_bench's took six times as long)
    benchlib.main(__file__, child, out=None, reps=3, timeout=300, header=None)


if __name__ == '__main__':
    main()
