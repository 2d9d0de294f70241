"""The optimiser step on R-101's real trainable shapes: the reference's eager composition against the fused HIP step.

    python tools/optim_bench.py [--out profiles/optim_bench.txt] [--reps 40]

Shapes: every tensor of training.trainable_parameters(resnet(classes, 101)) plus the 6-element `uncert`, with the groups of
training.make_optimizer (lr 0.001, momentum 0.9, weight decay 1e-4 on weights, 0 on biases and uncert); random values, the
gradients scaled so that the norm exceeds clip_norm = 10 (the clip is active in both versions).
  * eager : the reference's clip_gradient op for op (lib/model/utils/net_utils.py:37-49: one norm() per parameter, the Python sum,
    the square root read on the host -- a blocking device-to-host read --, then grad.mul_(coefficient) per parameter) followed by
    torch.optim.SGD.step() (trainval_net.py:224-227; torch's default multi-tensor path on the device);
  * foreach : today's eager torch without the host read -- torch.nn.utils.clip_grad_norm_ + torch.optim.SGD.step() (a second
    yardstick: what eager torch can do when the reference's clip_gradient is replaced by torch's own);
  * fused : stereo_rcnn_amd.optim.SGD.step(clip_norm=10.) -- srcnn_grad_norm + srcnn_sgd_step, no host read, gradients untouched.
Bytes: counted from the operations, per element of the N clipped-and-updated floats.  eager = 56 N (norm: read g 4; mul_: read and
write g 8; weight decay: read g, p, write g 12; momentum mul_: 8; momentum add_: 12; parameter add_: 12 -- 44 N on tensors without
weight decay), fused = 24 N (norm: read g 4; step: read p, g, m, write p, m 20).  GB/s = those bytes over the median time, beside
the 6.3 TB/s copy ceiling of the MI355X (achievable of 8 TB/s HBM: the peak stereo_rcnn_amd/layer_table.py uses).
One process, warm (5 untimed runs of each); the versions ALTERNATE, every run is timed with device events around the whole call
and ends in a synchronise; medians of --reps runs with min and max.  The fused and eager parameters after the same three steps
are compared before timing.  Runner and timer: tools/benchlib.py."""
import benchlib

CLIP = 10.0
HBM_COPY_CEILING_TBS = 6.3


def reference_clip_gradient(params, clip_norm):
    """net_utils.py:37-49, op for op; np.sqrt of the device value is the host read."""
    import numpy as np
    totalnorm = 0
    for p in params:
        modulenorm = p.grad.data.norm()
        totalnorm += modulenorm ** 2
    totalnorm = np.sqrt(float(totalnorm))                   # blocking device-to-host read
    norm = clip_norm / max(totalnorm, clip_norm)
    for p in params:
        p.grad.mul_(norm)


def r101_shapes():
    """[(name, shape)] of R-101's trainable parameters, in make_optimizer's order."""
    from stereo_rcnn_amd import training
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    model = resnet(('__background__', 'Car'), 101)
    model.create_architecture()
    return [(k, tuple(p.shape)) for k, p in training.trainable_parameters(model).items()]


def groups_of(names, tensors, uncert):
    from stereo_rcnn_amd.model.utils.config import cfg
    T = cfg.TRAIN
    lr = T.LEARNING_RATE
    gs = []
    for key, t in zip(names, tensors):
        if 'bias' in key:
            gs.append({'params': [t], 'lr': lr * (T.DOUBLE_BIAS + 1), 'weight_decay': T.BIAS_DECAY and T.WEIGHT_DECAY or 0})
        else:
            gs.append({'params': [t], 'lr': lr, 'weight_decay': T.WEIGHT_DECAY})
    gs.append({'params': [uncert], 'lr': lr})
    return gs


def child(reps):
    import torch
    from stereo_rcnn_amd import optim
    from stereo_rcnn_amd.model.utils.config import cfg
    dev = benchlib.device()
    shapes = r101_shapes()
    names = [k for k, _ in shapes]
    gen = torch.Generator(device=dev).manual_seed(0)
    init = [torch.randn(s, device=dev, generator=gen) * 0.05 for _, s in shapes]
    grads = [torch.randn(s, device=dev, generator=gen) * 0.01 for _, s in shapes]
    uncert_g = torch.randn(6, device=dev, generator=gen)
    n_model = sum(t.numel() for t in init)
    n_decay = sum(t.numel() for k, t in zip(names, init) if 'bias' not in k)
    sizes = sorted(t.numel() for t in init)
    print('R-101 trainable: %d tensors, %d floats (%.1f MB); smallest %d, largest %d elements; + uncert (6, not clipped)'
          % (len(init), n_model, n_model * 4 / 1e6, sizes[0], sizes[-1]))

    def make(kind):
        ps = [t.clone().requires_grad_(True) for t in init]
        u = torch.full((6,), -1.0, device=dev, requires_grad=True)
        cls = optim.SGD if kind == 'fused' else torch.optim.SGD
        return ps, u, cls(groups_of(names, ps, u), momentum=cfg.TRAIN.MOMENTUM)

    state = {k: make(k) for k in ('eager', 'foreach', 'fused')}

    def set_grads(kind):
        ps, u, _ = state[kind]
        for p, g in zip(ps, grads):
            if p.grad is None:
                p.grad = g.clone()
            else:
                p.grad.copy_(g)                 # the eager versions scale their gradients in place: restore them (untimed)
        u.grad = uncert_g.clone()

    def run(kind):
        ps, u, opt = state[kind]
        if kind == 'eager':
            reference_clip_gradient(ps, CLIP)
            opt.step()
        elif kind == 'foreach':
            torch.nn.utils.clip_grad_norm_(ps, CLIP)
            opt.step()
        else:
            opt.step(clip_norm=CLIP, clip_params=ps)

    for _ in range(3):                                      # the same three steps in every version, compared before timing
        for kind in state:
            set_grads(kind)
            run(kind)
    torch.cuda.synchronize()
    norm, coef = (float(v) for v in state['fused'][2].last_norm)
    print('gradient norm %.4f, clip coefficient %.6f (clip_norm %.1f)' % (norm, coef, CLIP))
    for other in ('eager', 'foreach'):
        worst = max(float((a.detach() - b.detach()).abs().max() / b.detach().abs().max()) for a, b in zip(state['fused'][0], state[other][0]))
        print('after three steps, fused against %s: largest |parameter difference| / largest |parameter| of a tensor: %.2e' % (other, worst))

    times = benchlib.alternating([(kind, lambda kind=kind: run(kind)) for kind in state], reps, warmup=5, before=set_grads, sync_before=True)
    us = {k: tuple(t * 1e3 for t in benchlib.stats(v)) for k, v in times.items()}
    nbytes = {'eager': 56 * n_decay + 44 * (n_model - n_decay), 'foreach': 56 * n_decay + 44 * (n_model - n_decay), 'fused': 24 * n_model}
    med = {k: v[0] for k, v in us.items()}
    print('%-8s %12s %12s %12s %14s %10s %s' % ('version', 'median us', 'min us', 'max us', 'bytes counted', 'GB/s', 'share of the %.1f TB/s copy ceiling' % HBM_COPY_CEILING_TBS))
    for k in state:
        gbs = nbytes[k] / (med[k] * 1e-6) / 1e9
        print('%-8s %12.1f %12.1f %12.1f %14d %10.0f %.1f %%' % ((k,) + us[k] + (nbytes[k], gbs, 100.0 * gbs / (HBM_COPY_CEILING_TBS * 1e3))))
    print('fused / eager = %.3f, fused / foreach = %.3f (%d runs each)' % (med['fused'] / med['eager'], med['fused'] / med['foreach'], reps))
    print('least time for the fused bytes at the copy ceiling: %.1f us' % (nbytes['fused'] / (HBM_COPY_CEILING_TBS * 1e12) * 1e6))


def main():
    benchlib.main(__file__, child, out='optim_bench.txt', reps=40, timeout=300,
                  header='# python tools/optim_bench.py --reps %(reps)d   (see the tool for what each line measures)')


if __name__ == '__main__':
    main()
