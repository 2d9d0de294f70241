"""The R-101 training step at 600 x 1987 with weights prepared once per step and with the engine chosen per layer.

    python tools/train_step_auto_bench.py [--out profiles/train_step_auto_bench.txt] [--reps 10]

Four legs ALTERNATE in the same rounds (forward_train + backward of the six losses; tools/train_step_bench.py's case):
  * parent   : both precisions f16x3 with reuse_maxima -- the fastest setting before these options existed;
  * prepared : the same with TrainWeights.prepare() at the start of the step (train_step's prepared_weights=True);
  * auto     : both precisions 'auto' with prepared weights;
  * fp32     : the exact-fp32 engine both ways.
Ratios are against the parent leg of the same run.  The six losses of one step at the same seed are printed per leg, and the engines
'auto' chose.  Runner and timer: tools/benchlib.py."""
import benchlib


def child(reps):
    import torch
    from stereo_rcnn_amd import autograd, training
    from train_step_bench import headline_case
    dev = benchlib.device()
    print('device: %s; clocks before: %s' % (torch.cuda.get_device_name(0), benchlib.clocks()))
    model, args = headline_case(dev)
    weights = training.TrainWeights(model)
    gen = torch.Generator(device=dev).manual_seed(1)
    settings = [('parent', 'f16x3', 'f16x3', False), ('prepared', 'f16x3', 'f16x3', True), ('auto', 'auto', 'auto', True),
                ('fp32', 'f32', 'f32', False)]

    def leg(fp, bp, prepared, generator=gen):
        def run():
            for p in model.parameters():
                p.grad = None
            w = weights.prepare() if prepared else None
            out = training.forward_train(model, *args, generator=generator, forward_precision=fp, backward_precision=bp, weights=w)
            sum(out[8:14]).backward()
            return out
        return run

    for name, fp, bp, prepared in settings:
        with autograd.record_engines() as e:
            out = leg(fp, bp, prepared, torch.Generator(device=dev).manual_seed(1))()
        print('six losses, %-8s (same seed): %s' % (name, ' '.join('%.5f' % float(v.detach()) for v in out[8:14])))
        if name == 'auto':
            print('  auto: %d convolution calls; forward f16x3 %d, fp32 %d; backward f16x3 %d, fp32 %d'
                  % (len(e), sum(r[3] == 'f16x3' for r in e), sum(r[3] == 'f32' for r in e), sum(r[4] == 'f16x3' for r in e),
                     sum(r[4] == 'f32' for r in e)))
        del out
    r = {k: benchlib.stats(v) for k, v in benchlib.alternating([(n, leg(fp, bp, pr)) for n, fp, bp, pr in settings], reps, warmup=2).items()}
    print('forward + backward of the training step, ResNet-101, 600 x 1987, B = 1, %d alternating runs, ms: median (min, max)' % reps)
    what = {'parent': 'f16x3 both ways, reuse_maxima (the parent setting)', 'prepared': '+ prepared_weights',
            'auto': "'auto' both ways + prepared_weights", 'fp32': 'exact-fp32 engine both ways'}
    for name, _, _, _ in settings:
        print('  %-52s %7.1f (%.1f, %.1f); / parent setting %.3f' % ((what[name] + ':',) + r[name] + (r[name][0] / r['parent'][0],)))
    print('clocks after: ' + benchlib.clocks())


def main():
    benchlib.main(__file__, child, out='train_step_auto_bench.txt', reps=10, timeout=420,
                  header='# python tools/train_step_auto_bench.py --reps %(reps)d   (see the tool for what each line measures)')


if __name__ == '__main__':
    main()
