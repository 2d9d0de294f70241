"""The BN fold and the re-layout of every training weight on the device (TrainWeights.prepare(device_fold=True), csrc/train_fold.hip)
against the eager torch operators they replace, R-101 at 600 x 1987, f16x3 both ways with reuse_maxima.

    python tools/train_fold_bench.py [--out profiles/train_fold_bench.txt] [--reps 10]

The legs ALTERNATE in the same rounds (tools/train_step_auto_bench.py's scheme; the case is tools/train_step_bench.py's):
  (a) TrainWeights.prepare() alone, eager fold against device fold: between device events, and as host wall time of the call
      (no wait inside the window: what the host spends enqueueing);
  (b) the whole training.train_step, prepared_weights=True against prepared_weights=True + device_fold=True;
  (c) the kernel launches of one prepare() on each path (torch.profiler's device-side kernel records);
  (d) the six losses of one forward at the same seed on both paths: they agree digit for digit (the tests hold the bits).
The eager leg IS the parent commit's path; ratios are against it, same run.  Runner and timer: tools/benchlib.py."""
import time

import benchlib


def host_window(fn, inner=1, sync_before=False):
    """ms of host time per call, the device idle at the start and not waited for inside."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    t = (time.perf_counter() - t0) * 1e3 / inner
    torch.cuda.synchronize()
    return t


def kernel_launches(fn):
    """(kernels, memory copies / sets) the device ran for one fn(), or None where the profiler gives no device records."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    except Exception as e:                                                        # the count is a by-product
        print('  (launches not counted: %s)' % type(e).__name__)
        return None
    mem = sum(1 for e in dev if e.name.lower().startswith(('memcpy', 'memset')) or 'copybuffer' in e.name.lower()
              or 'fillbuffer' in e.name.lower())
    return (len(dev) - mem, mem) if dev else None


def child(reps):
    import torch
    from stereo_rcnn_amd import training
    from train_step_bench import headline_case
    dev = benchlib.device()
    print('device: %s; clocks before: %s' % (torch.cuda.get_device_name(0), benchlib.clocks()))
    model, args = headline_case(dev)
    weights = training.TrainWeights(model)
    legs = [('eager', False), ('device', True)]
    print('%d layers; forward and backward f16x3, reuse_maxima' % len(weights.specs()))

    # (d)
    for name, fold in legs:
        for p in model.parameters():
            p.grad = None
        out = training.forward_train(model, *args, generator=torch.Generator(device=dev).manual_seed(1), forward_precision='f16x3',
                                     backward_precision='f16x3', weights=weights.prepare(device_fold=fold))
        sum(out[8:14]).backward()
        print('six losses, %-6s fold (same seed): %s' % (name, ' '.join('%.9g' % float(v.detach()) for v in out[8:14])))
        del out

    # (c)
    for name, fold in legs:
        n = kernel_launches(lambda: weights.prepare(device_fold=fold))
        if n:
            print('one prepare(), %-6s fold: %d kernel launches (+ %d memory copies / sets)' % ((name,) + n))

    # (a)
    prep = [(name, (lambda fold=fold: weights.prepare(device_fold=fold))) for name, fold in legs]
    ev = {k: benchlib.stats(v) for k, v in benchlib.alternating(prep, reps, warmup=2, sync_before=True).items()}
    host = {k: benchlib.stats(v) for k, v in benchlib.alternating(prep, reps, warmup=2, timer=host_window).items()}
    print('TrainWeights.prepare() alone, %d alternating runs, ms: median (min, max)' % reps)
    for name, _ in legs:
        print('  %-6s fold: between device events %6.2f (%.2f, %.2f); host wall time %6.2f (%.2f, %.2f)' % ((name,) + ev[name] + host[name]))

    # (b)
    def step(fold):
        uncert = torch.full((6,), -1.0, device=dev, requires_grad=True)
        opt = training.make_optimizer(model, uncert, lr=0.0)            # lr 0: the weights, and with them the work, stay the same
        gen = torch.Generator(device=dev).manual_seed(1)
        return lambda: training.train_step(model, opt, uncert, args, generator=gen, forward_precision='f16x3', backward_precision='f16x3',
                                           prepared_weights=True, device_fold=fold)

    r = {k: benchlib.stats(v) for k, v in benchlib.alternating([(n, step(f)) for n, f in legs], reps, warmup=2).items()}
    print('training.train_step (prepare, forward, backward, clipped SGD), %d alternating runs, ms: median (min, max)' % reps)
    for name, label in (('eager', 'prepared_weights (the parent path):'), ('device', 'prepared_weights + device_fold:')):
        print('  %-40s %7.1f (%.1f, %.1f); / parent path %.3f' % ((label,) + r[name] + (r[name][0] / r['eager'][0],)))
    print('clocks after: ' + benchlib.clocks())


def main():
    benchlib.main(__file__, child, out='train_fold_bench.txt', reps=10, timeout=420,
                  header='# python tools/train_fold_bench.py --reps %(reps)d   (see the tool for what each line measures)')


if __name__ == '__main__':
    main()
