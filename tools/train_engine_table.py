"""The table autograd.choose_engine ('auto') is fitted to: every distinct trainable layer of the R-101 step at 600 x 1987 on the
fp32 engine and on the f16x3 engine, forward and backward, and the cost of preparing all weights once.

    python tools/train_engine_table.py [--out profiles/train_engine_table.txt] [--reps 30]

1. Per layer (tools/conv_backward_bench.py's list) and direction, three calls that ALTERNATE inside every round:
     * fp32     : srcnn_conv2d precision 0 (forward) / srcnn_conv2d_backward (dx, dw, db) -- what forward_train runs by default;
     * handed   : the f16x3 call with max |x| handed over (forward: x_amax given, y_amax requested) -- it still clears, scans w and
                  splits w itself;
     * prepared : the same with the weights prepared (srcnn_conv2d_*_f16x3_prepared): no pass over w inside the call.
   Whole calls between device events, medians after 10 untimed rounds.  The prepared call's results must equal the handed call's.
   `ratio` = prepared / fp32 is what the rule is fitted to: with training.TrainWeights the preparation is paid once per step, not per
   call, so a layer's f16x3 time excludes it.
2. That once-per-step cost: TrainWeights(model).prepare() of the R-101 model -- the eager folds plus the one
   srcnn_train_weights_prepare call -- and the call alone on already folded weights (engine.prepare_train_weights).
The `row` lines are machine-readable: --emit-python prints stereo_rcnn_amd/train_engine_table.py from a profile without a GPU.
Runner and timer: tools/benchlib.py."""
import re
import sys

import benchlib
from conv_backward_bench import LAYERS


def layers(dev, reps):
    import torch
    from stereo_rcnn_amd import engine
    print('%-30s %-8s %9s %6s %7s | %9s %9s %11s | %11s %9s' % ('layer', 'dir', 'M', 'N', 'K', 'fp32 us', 'handed us', 'prepared us',
                                                                 'handed/fp32', 'ratio'))
    rows = []
    for name, B, H, W, cin, cout, k, s, p in LAYERS:
        gen = torch.Generator().manual_seed(1)
        OH, OW = engine.conv_out_hw(H, W, k, k, s, p)
        x = torch.randn(B, H, W, cin, generator=gen).to(dev)
        w = (torch.randn(cout, k, k, cin, generator=gen) / float(k * k * cin) ** 0.5).to(dev)
        cw = engine.ConvW(w, torch.randn(cout, generator=gen).to(dev), k, k, s, p, True)
        dy = (torch.randn(B, OH, OW, cout, generator=gen) * 1e-3).to(dev)
        ys = [torch.empty(B, OH, OW, cout, device=dev) for _ in range(3)]
        xw, yw = engine.absmax(x), torch.empty(1, dtype=torch.int32, device=dev)
        prepared, = engine.prepare_train_weights([w])
        outs = [{'dx': torch.empty_like(x), 'dw': torch.empty_like(w), 'db': torch.empty(cout, device=dev)} for _ in range(3)]

        fwd = [('fp32', lambda: engine.conv2d(cw, x, B, H, W, ys[0], OH, OW, precision='f32', plan=(0, 0, 0, 0, 0))),
               ('handed', lambda: engine.conv2d_train_f16x3(cw, x, B, H, W, ys[1], OH, OW, x_amax=xw, y_amax=yw)),
               ('prepared', lambda: engine.conv2d_train_f16x3(cw, x, B, H, W, ys[2], OH, OW, x_amax=xw, y_amax=yw, prepared=prepared))]
        for _, fn in fwd:
            fn()
        torch.cuda.synchronize()
        assert torch.equal(ys[1], ys[2]), name
        y = ys[0]
        bwd = [('fp32', lambda: engine.conv2d_backward(cw, x, B, H, W, y, dy, OH, OW, out=outs[0])),
               ('handed', lambda: engine.conv2d_backward(cw, x, B, H, W, y, dy, OH, OW, out=outs[1], precision='f16x3', x_amax=xw)),
               ('prepared', lambda: engine.conv2d_backward(cw, x, B, H, W, y, dy, OH, OW, out=outs[2], precision='f16x3', x_amax=xw,
                                                           prepared=prepared))]
        for _, fn in bwd:
            fn()
        torch.cuda.synchronize()
        assert all(torch.equal(outs[1][q], outs[2][q]) for q in ('dx', 'dw', 'db')), name
        for direction, versions in (('forward', fwd), ('backward', bwd)):
            med = {k_: benchlib.stats(v)[0] * 1e3 for k_, v in benchlib.alternating(versions, reps, warmup=10).items()}
            M, N, K = B * OH * OW, cout, k * k * cin
            print('%-30s %-8s %9d %6d %7d | %9.1f %9.1f %11.1f | %11.2f %9.3f' % (name, direction, M, N, K, med['fp32'], med['handed'],
                  med['prepared'], med['handed'] / med['fp32'], med['prepared'] / med['fp32']), flush=True)
            rows.append((direction, M, N, K, med['prepared'] / med['fp32']))
    print('(medians of %d runs in us, event-timed one call at a time, launch overhead included)' % reps)
    for r in rows:
        print('row %s %d %d %d %.3f' % r)


def prepare(dev, reps):
    import torch
    from stereo_rcnn_amd import engine, training
    from train_step_bench import headline_case
    model, _ = headline_case(dev)
    tw = training.TrainWeights(model)
    with torch.no_grad():
        folded = [w.contiguous() for _, w, _ in tw.enumerate()]
    floats = sum(w.numel() for w in folded)
    t = benchlib.alternating([('whole', lambda: tw.prepare()), ('call', lambda: engine.prepare_train_weights(folded))], reps, warmup=3)
    whole, call = benchlib.stats(t['whole']), benchlib.stats(t['call'])
    print('preparation once per step, ResNet-101: %d layers, %.1f M weights' % (len(folded), floats / 1e6))
    print('  TrainWeights.prepare() (eager folds and re-layouts + the call): %.3f ms (%.3f, %.3f)' % whole)
    print('  srcnn_train_weights_prepare alone (%d launches): %.3f ms (%.3f, %.3f); %.0f GB/s over 4 B read + 8 B written per weight'
          % ((3 + (len(folded) - 1) // 48,) + call + (floats * 12 / call[0] / 1e6,)))


def child(reps):
    import torch
    dev = benchlib.device()
    print('device: %s; clocks before: %s' % (torch.cuda.get_device_name(0), benchlib.clocks()))
    layers(dev, reps)
    prepare(dev, max(5, reps // 3))
    print('clocks after: ' + benchlib.clocks())


def emit_python(profile):
    rows = re.findall(r'^row (\w+) (\d+) (\d+) (\d+) ([\d.]+)$', open(profile).read(), flags=re.M)
    print('"""The measured rows autograd.choose_engine is fitted to: (direction, M, N, K, f16x3 / fp32 time) per distinct trainable layer of the')
    print('R-101 step at 600 x 1987, f16x3 with maxima handed over and weights prepared.  Generated from profiles/train_engine_table.txt by')
    print('`python tools/train_engine_table.py --emit-python profiles/train_engine_table.txt`; data only."""')
    print('ROWS = (')
    for d, M, N, K, r in rows:
        print("    ('%s', %s, %s, %s, %s)," % (d, M, N, K, r))
    print(')')


def main():
    if len(sys.argv) == 3 and sys.argv[1] == '--emit-python':
        return emit_python(sys.argv[2])
    benchlib.main(__file__, child, out='train_engine_table.txt', reps=30, timeout=420,
                  header='# python tools/train_engine_table.py --reps %(reps)d   (see the tool for what each column measures)')


if __name__ == '__main__':
    main()
