"""The guarded optimiser step against the plain one on R-101's real trainable shapes (the list of tools/optim_bench.py).

    python tools/optim_guard_bench.py [--out profiles/optim_guard_bench.txt] [--reps 40]

  * plain   : stereo_rcnn_amd.optim.SGD.step(clip_norm=10.) -- srcnn_grad_norm + srcnn_sgd_step;
  * guarded : the same call with guard=True -- srcnn_grad_norm_guarded + srcnn_sgd_step_guarded (include/srcnn_hip.h): one
    more multiplication per gradient element in each pass, a third word from the norm, the update under that word;
  * accum 1/2 : guard=True, grad_scale=0.5 (the call that ends two accumulated micro-batches): the same kernels, another scale.
Both move 24 bytes per element (norm: read g 4; step: read p, g, m, write p, m 20); the guarded pair adds three words.
One process, warm (5 untimed rounds); the versions ALTERNATE inside every round, every run is a whole call between two device
events and ends in a synchronise; medians of --reps runs with min and max.  Gradients are finite, so every step is taken; the
parameters of the plain and the guarded optimiser after the same three steps are compared bit for bit before timing.  Runner and
timer: tools/benchlib.py; shapes and groups: tools/optim_bench.py."""
import benchlib
import optim_bench

CLIP = optim_bench.CLIP


def child(reps):
    import torch
    from stereo_rcnn_amd import optim
    from stereo_rcnn_amd.model.utils.config import cfg
    dev = benchlib.device()
    shapes = optim_bench.r101_shapes()
    names = [k for k, _ in shapes]
    gen = torch.Generator(device=dev).manual_seed(0)
    init = [torch.randn(s, device=dev, generator=gen) * 0.05 for _, s in shapes]
    grads = [torch.randn(s, device=dev, generator=gen) * 0.01 for _, s in shapes]
    uncert_g = torch.randn(6, device=dev, generator=gen)
    n_model = sum(t.numel() for t in init)
    print('R-101 trainable: %d tensors, %d floats (%.1f MB); + uncert (6, not clipped)' % (len(init), n_model, n_model * 4 / 1e6))

    keywords = {'plain': {}, 'guarded': {'guard': True}, 'accum 1/2': {'guard': True, 'grad_scale': 0.5}}
    state = {}
    for kind in keywords:
        ps = [t.clone().requires_grad_(True) for t in init]
        u = torch.full((6,), -1.0, device=dev, requires_grad=True)
        for p, g in zip(ps, grads):
            p.grad = g.clone()                                  # the step only reads them
        u.grad = uncert_g.clone()
        state[kind] = (ps, optim.SGD(optim_bench.groups_of(names, ps, u), momentum=cfg.TRAIN.MOMENTUM))

    def run(kind):
        ps, opt = state[kind]
        opt.step(clip_norm=CLIP, clip_params=ps, **keywords[kind])

    for _ in range(3):
        for kind in state:
            run(kind)
    torch.cuda.synchronize()
    print('plain:   gradient norm %.4f, clip coefficient %.6f' % tuple(float(v) for v in state['plain'][1].last_norm))
    print('guarded: gradient norm %.4f, clip coefficient %.6f, ok %g; skipped steps %d'
          % (tuple(float(v) for v in state['guarded'][1].last_norm) + (int(state['guarded'][1].skipped_steps),)))
    same = all(torch.equal(a.detach(), b.detach()) for a, b in zip(state['plain'][0], state['guarded'][0]))
    print('after three steps, guarded against plain: parameters %s' % ('bit-equal' if same else 'DIFFER'))
    assert same

    times = benchlib.alternating([(kind, lambda kind=kind: run(kind)) for kind in state], reps, warmup=5, sync_before=True)
    us = {k: tuple(t * 1e3 for t in benchlib.stats(v)) for k, v in times.items()}
    print('%-10s %12s %12s %12s %10s' % ('version', 'median us', 'min us', 'max us', 'GB/s'))
    for k in state:
        print('%-10s %12.1f %12.1f %12.1f %10.0f' % ((k,) + us[k] + (24 * n_model / (us[k][0] * 1e-6) / 1e9,)))
    print('guarded / plain = %.3f, accum 1/2 / plain = %.3f (medians of %d runs each)'
          % (us['guarded'][0] / us['plain'][0], us['accum 1/2'][0] / us['plain'][0], reps))


def main():
    benchlib.main(__file__, child, out='optim_guard_bench.txt', reps=40, timeout=300,
                  header='# python tools/optim_guard_bench.py --reps %(reps)d   (see the tool for what each line measures)')


if __name__ == '__main__':
    main()
