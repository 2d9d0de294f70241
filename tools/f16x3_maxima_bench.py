"""What handing max |x| from layer to layer buys the opt-in 3 x f16 training path (reuse_maxima; srcnn_conv2d_forward_f16x3_maxima).

    python tools/f16x3_maxima_bench.py [--out profiles/f16x3_maxima_bench.txt] [--reps 50] [--step-reps 10] [--skip-step]

1. Per layer (tools/conv_backward_bench.py's layer list: the trainable trunk and head at B = 1, one 600 x 1987 image), three
   forwards that ALTERNATE inside every round:
     * fp32   : srcnn_conv2d, precision 0, heuristic plan, bias + ReLU -- what forward_train runs by default;
     * f16x3  : srcnn_conv2d_forward_f16x3, everything the call issues (clear, max|w|, max|x|, weight split, GEMM);
     * handed : srcnn_conv2d_forward_f16x3_maxima with x_amax given (no max|x| pass) and y_amax requested (the epilogue's maximum).
   Whole calls between device events, medians of --reps after 10 untimed rounds.  The handed call's y must equal the plain call's.
2. The training step (ResNet-101, 600 x 1987, B = 1: tools/train_step_bench.py's case), forward + backward of the six losses, four
   legs alternating in the same rounds: fp32 both ways; f16x3 both ways with reuse_maxima off (the parent's f16x3 step); the same
   with reuse_maxima on; f16x3 backward only with reuse_maxima on / off.  engine.F16X3_MAXIMA of one step is printed beside them.
Runner and timer: tools/benchlib.py."""
import benchlib
from conv_backward_bench import LAYERS


def layers(dev, reps):
    import torch
    from stereo_rcnn_amd import engine
    print('%-30s %9s %6s %7s | %9s | %9s %9s | %10s %11s %12s'
          % ('layer', 'M', 'N', 'K', 'fp32 us', 'f16x3 us', 'handed us', 'f16x3/fp32', 'handed/fp32', 'handed/f16x3'))
    for name, B, H, W, cin, cout, k, s, p in LAYERS:
        gen = torch.Generator().manual_seed(1)
        OH, OW = engine.conv_out_hw(H, W, k, k, s, p)
        x = torch.randn(B, H, W, cin, generator=gen).to(dev)
        w = (torch.randn(cout, k, k, cin, generator=gen) / float(k * k * cin) ** 0.5).to(dev)
        cw = engine.ConvW(w, torch.randn(cout, generator=gen).to(dev), k, k, s, p, True)
        y32, y16, yh = (torch.empty(B, OH, OW, cout, device=dev) for _ in range(3))
        xw, yw = engine.absmax(x), torch.empty(1, dtype=torch.int32, device=dev)

        def fp32():
            engine.conv2d(cw, x, B, H, W, y32, OH, OW, precision='f32', plan=(0, 0, 0, 0, 0))

        def f16x3():
            engine.conv2d_train_f16x3(cw, x, B, H, W, y16, OH, OW)

        def handed():
            engine.conv2d_train_f16x3(cw, x, B, H, W, yh, OH, OW, x_amax=xw, y_amax=yw)

        fp32(), f16x3(), handed()
        torch.cuda.synchronize()
        assert torch.equal(y16, yh), name                   # the same bits: only who found the maximum differs
        assert float(yw.view(torch.float32)) == float(yh.abs().max()), name
        times = benchlib.alternating([('fp32', fp32), ('f16x3', f16x3), ('handed', handed)], reps, warmup=10)
        med = {k_: benchlib.stats(v)[0] * 1e3 for k_, v in times.items()}
        print('%-30s %9d %6d %7d | %9.1f | %9.1f %9.1f | %10.2f %11.2f %12.2f'
              % (name, B * OH * OW, cout, k * k * cin, med['fp32'], med['f16x3'], med['handed'], med['f16x3'] / med['fp32'],
                 med['handed'] / med['fp32'], med['handed'] / med['f16x3']), flush=True)
    print('(medians of %d runs in us, event-timed one call at a time, launch overhead included: 5 launches for f16x3, 4 for handed)' % reps)


def step(dev, reps):
    import torch
    from stereo_rcnn_amd import engine, training
    from train_step_bench import headline_case
    model, args = headline_case(dev)
    gen = torch.Generator(device=dev).manual_seed(1)

    def leg(fp, bp, reuse):
        def run():
            for p in model.parameters():
                p.grad = None
            sum(training.forward_train(model, *args, generator=gen, forward_precision=fp, backward_precision=bp,
                                       reuse_maxima=reuse)[8:14]).backward()
        return run

    legs = [('fp32', leg('f32', 'f32', True)), ('f16x3 off', leg('f16x3', 'f16x3', False)), ('f16x3 on', leg('f16x3', 'f16x3', True)),
            ('bwd16 off', leg('f32', 'f16x3', False)), ('bwd16 on', leg('f32', 'f16x3', True))]
    counters = {}
    for name, fn in legs:
        engine.reset_f16x3_maxima()
        fn()
        torch.cuda.synchronize()
        counters[name] = dict(engine.F16X3_MAXIMA)
    r = {k: benchlib.stats(v) for k, v in benchlib.alternating(legs, reps, warmup=2).items()}
    print('forward + backward of the training step, ResNet-101, 600 x 1987, B = 1, %d alternating runs, ms: median (min, max)' % reps)
    what = {'fp32': 'exact-fp32 engine both ways', 'f16x3 off': 'forward and backward f16x3, reuse_maxima=False',
            'f16x3 on': 'forward and backward f16x3, reuse_maxima=True', 'bwd16 off': 'fp32 forward, f16x3 backward, reuse_maxima=False',
            'bwd16 on': 'fp32 forward, f16x3 backward, reuse_maxima=True'}
    for name, _ in legs:
        print('  %-52s %7.1f (%.1f, %.1f); / fp32 step %.3f; max|x| scans %d, served by an older word %d'
              % ((what[name] + ':',) + r[name] + (r[name][0] / r['fp32'][0], counters[name]['scans'], counters[name]['reused'])))
    print('  reuse_maxima on / off, f16x3 both ways: %.3f; f16x3 backward only: %.3f'
          % (r['f16x3 on'][0] / r['f16x3 off'][0], r['bwd16 on'][0] / r['bwd16 off'][0]))


def child(reps, step_reps, skip_step):
    import torch
    dev = benchlib.device()
    print('device: %s; clocks before: %s' % (torch.cuda.get_device_name(0), benchlib.clocks()))
    layers(dev, reps)
    if not skip_step:
        step(dev, step_reps)
    print('clocks after: ' + benchlib.clocks())


def main():
    benchlib.main(__file__, child, out='f16x3_maxima_bench.txt', reps=50, timeout=420,
                  extra=[('--step-reps', dict(type=int, default=10)), ('--skip-step', dict(action='store_true'))],
                  header='# python tools/f16x3_maxima_bench.py --reps %(reps)d --step-reps %(step_reps)d   (see the tool for what each column measures)')


if __name__ == '__main__':
    main()
