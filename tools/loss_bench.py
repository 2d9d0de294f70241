"""The training losses, forward + backward: the fused HIP kernels against the same computation composed from eager torch ops.

    python tools/loss_bench.py [--out profiles/loss_bench.txt] [--reps 60]

Shapes: `rpn_losses` at the headline RPN size -- one 600 x 1987 image, pyramid maps 150x497, 75x249, 38x125, 19x63, 10x32 with 3
anchors per location = 298476 anchors, 256 of them labelled (cfg.TRAIN.RPN_BATCHSIZE), at most 128 foreground -- and `rcnn_losses`
at 512 rois (cfg.TRAIN.BATCH_SIZE), 2 classes, G = 28.  Each timed run is the forward of the losses and the backward down to
the gradients of the prediction tensors (upstream gradients on the device).
  * fused : stereo_rcnn_amd.model.stereo_rcnn.losses (srcnn_cross_entropy / srcnn_smooth_l1 and their backwards; no host read);
  * eager : the reference's composition in torch ops on the same device (stereo_rpn.py:113-136, stereo_rcnn.py:204-230, 274-311,
    net_utils.py:79-99): nonzero + index_select + F.cross_entropy, the target packing, expand, the ten-op smooth L1, gather, and
    three `float(torch.sum(w)) < 1` reads that make the host wait.
One process, warm (10 untimed runs of each); the two versions ALTERNATE, every run is timed with device events and ends in a
synchronise; medians of --reps runs are reported, with min and max.  The two versions' losses are compared before timing.
Runner and timer: tools/benchlib.py."""
import benchlib

MAPS = [(150, 497), (75, 249), (38, 125), (19, 63), (10, 32)]
ANCHORS = 3 * sum(h * w for h, w in MAPS)
ROIS, N_CLS, G = 512, 2, 28


def eager_smooth_l1(pred, target, w_in=None, w_out=None, sigma=1.0, dim=(1,)):
    """net_utils.py:79-99, op for op."""
    import torch
    sigma_2 = sigma ** 2
    d = pred - target
    if w_in is not None:
        d = w_in * d
    a = torch.abs(d)
    sign = (a < 1. / sigma_2).detach().float()
    v = torch.pow(d, 2) * (sigma_2 / 2.) * sign + (a - (0.5 / sigma_2)) * (1. - sign)
    if w_out is not None:
        v = w_out * v
    for i in sorted(dim, reverse=True):
        v = v.sum(i)
    return v.mean()


def eager_rpn(cls, box, label, tl, tr, inside, outside):
    import torch
    import torch.nn.functional as F
    B, A = box.shape[0], box.shape[1]
    flat = label.view(-1)
    keep = flat.ne(-1).nonzero().view(-1)                                   # host wait
    loss_cls = F.cross_entropy(torch.index_select(cls.view(-1, 2), 0, keep), torch.index_select(flat, 0, keep).long())
    targets = tl.new_zeros(B, A, 6)
    targets[:, :, :4] = tl
    targets[:, :, 4] = tr[:, :, 0]
    targets[:, :, 5] = tr[:, :, 2]
    return loss_cls, eager_smooth_l1(box, targets, inside.unsqueeze(2).expand(B, A, 6), outside.unsqueeze(2).expand(B, A, 6), sigma=3)


def eager_rcnn(cls, bbox, dim, kpts, label, tl, tr, tdim, klabel, kweight, in4, out4):
    import torch
    import torch.nn.functional as F
    n = cls.shape[0]
    t6 = tl.new_zeros(1, n, 6)
    t6[:, :, :4], t6[:, :, 4], t6[:, :, 5] = tl, tr[:, :, 0], tr[:, :, 2]
    in6, out6 = in4.new_zeros(1, n, 6), out4.new_zeros(1, n, 6)
    in6[:, :, :4], in6[:, :, 4:] = in4, in4[:, :, 0:2]
    out6[:, :, :4], out6[:, :, 4:] = out4, out4[:, :, 0:2]
    label = label.view(-1).long()
    idx = label.view(n, 1, 1)
    bbox_sel = torch.gather(bbox.view(n, -1, 6), 1, idx.expand(n, 1, 6)).squeeze(1)
    dim_sel = torch.gather(dim.view(n, -1, 5), 1, idx.expand(n, 1, 5)).squeeze(1)
    loss_cls = F.cross_entropy(cls, label)
    loss_bbox = eager_smooth_l1(bbox_sel, t6.view(-1, 6), in6.view(-1, 6), out6.view(-1, 6))
    loss_dim = eager_smooth_l1(dim_sel, tdim.view(-1, 5))
    preds = (kpts[:, :4, :].contiguous().view(-1, 4 * G), kpts[:, 4, :].contiguous().view(-1, G), kpts[:, 5, :].contiguous().view(-1, G))
    terms = []
    for i, p in enumerate(preds):
        w = kweight[:, :, i].contiguous().view(-1)
        l = F.cross_entropy(p, klabel[:, :, i].contiguous().view(-1), reduction='none')
        if float(torch.sum(w)) < 1:                                         # host wait (stereo_rcnn.py:295, 301, 307)
            terms.append(torch.sum(l * w))
        else:
            terms.append(torch.sum(l * w) / torch.sum(w))
    return loss_cls, loss_bbox, loss_dim, (terms[0] + terms[1] + terms[2]) / 3.0


def make_inputs(dev, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    A = ANCHORS
    label = torch.full((1, A), -1.0)
    pick = torch.randperm(A, generator=g)[:256]
    label.view(-1)[pick[:100]] = 1.0
    label.view(-1)[pick[100:]] = 0.0
    rpn = dict(cls=torch.randn(1, A, 2, generator=g), box=torch.randn(1, A, 6, generator=g) * 0.2, label=label,
               tl=torch.randn(1, A, 4, generator=g) * 0.2, tr=torch.randn(1, A, 4, generator=g) * 0.2,
               inside=(label == 1).float(), outside=(label >= 0).float() / 256.0)
    n = ROIS
    rl = (torch.rand(n, generator=g) < 0.25).float()
    fg = rl.view(1, n, 1)
    rcnn = dict(cls=torch.randn(n, N_CLS, generator=g), bbox=torch.randn(n, 6 * N_CLS, generator=g) * 0.3,
                dim=torch.randn(n, 5 * N_CLS, generator=g) * 0.3, kpts=torch.randn(n, 6, G, generator=g), label=rl,
                tl=torch.randn(1, n, 4, generator=g) * 0.3, tr=torch.randn(1, n, 4, generator=g) * 0.3,
                tdim=torch.randn(1, n, 5, generator=g) * 0.3,
                klabel=torch.stack((torch.randint(0, 4 * G, (n,), generator=g), torch.randint(0, G, (n,), generator=g),
                                    torch.randint(0, G, (n,), generator=g)), 1).view(1, n, 3),
                kweight=(fg * torch.ones(1, n, 3)), in4=fg * torch.ones(1, n, 4), out4=fg * torch.ones(1, n, 4))
    to = lambda d: {k: v.to(dev) for k, v in d.items()}
    return to(rpn), to(rcnn)


def child(reps):
    import torch
    from stereo_rcnn_amd.model.stereo_rcnn import losses
    dev = benchlib.device()
    rpn, rcnn = make_inputs(dev)
    cases = [
        ('rpn_losses, %d anchors (1 image), 256 labelled' % ANCHORS, rpn, ('cls', 'box'), losses.rpn_losses, eager_rpn),
        ('rcnn_losses, %d rois, %d classes, G = %d' % (ROIS, N_CLS, G), rcnn, ('cls', 'bbox', 'dim', 'kpts'), losses.rcnn_losses, eager_rcnn),
    ]
    for title, inputs, pred_names, fused_fn, eager_fn in cases:
        rest = [v for k, v in inputs.items() if k not in pred_names]
        coef = [torch.tensor(0.5 + 0.25 * i, device=dev) for i in range(4)]

        def step(fn):
            leaves = [inputs[k].detach().clone().requires_grad_(True) for k in pred_names]
            out = fn(*leaves, *rest)
            total = out[0] * coef[0]
            for i in range(1, len(out)):
                total = total + out[i] * coef[i]
            total.backward()
            return out, leaves

        a, la = step(fused_fn)
        b, lb = step(eager_fn)
        torch.cuda.synchronize()
        print(title)
        print('  losses fused %s | eager %s' % (' '.join('%.6f' % float(v) for v in a), ' '.join('%.6f' % float(v) for v in b)))
        print('  largest |gradient difference| / largest |eager gradient|: %s'
              % ' '.join('%.1e' % (float((x.grad - y.grad).abs().max()) / max(float(y.grad.abs().max()), 1e-30)) for x, y in zip(la, lb)))
        times = benchlib.alternating([('fused', lambda: step(fused_fn)), ('eager', lambda: step(eager_fn))], reps, warmup=10)
        for name, t in times.items():
            print('  %s forward + backward: median %.3f ms (min %.3f, max %.3f, %d runs)' % ((name,) + benchlib.stats(t) + (reps,)))
        print('  fused / eager = %.2f' % (benchlib.stats(times['fused'])[0] / benchlib.stats(times['eager'])[0]))


def main():
    benchlib.main(__file__, child, out='loss_bench.txt', reps=60, timeout=300,
                  header='# python tools/loss_bench.py --reps %(reps)d   (see the tool for what each line measures)')


if __name__ == '__main__':
    main()
