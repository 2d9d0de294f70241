"""Times the training step and its new kernels on the device and writes profiles/train_step_bench.txt.

  1. `training.forward_train` + backward of the six losses at the headline size (ResNet-101, 600 x 1987, B = 1, synthetic weights,
     three ground-truth boxes; cfg.TRAIN.RPN_PRE_NMS_TOP_N set to the proposal kernel's 8192) against THE SAME GRAPH COMPOSED FROM
     EAGER TORCH OPS on the device, forward + backward: F.conv2d + eval-mode F.batch_norm + F.relu, F.interpolate, strided slicing,
     F.conv_transpose2d, F.dropout, ROIAlign as F.grid_sample on the (A + 1) lattice + F.avg_pool2d(2, 1) per level, the losses of
     tools/loss_bench.py (`eager_rpn`, `eager_rcnn`, host waits included).  The eager side is handed the discrete results of one
     product run as data (sampled rois, anchor and proposal targets), so it is spared the proposal and target layers: what is
     compared is the differentiable graph.  Its grid_sample does not clamp lattice points at the map border the way the ROIAlign
     kernels do, so the two sides' losses are printed next to each other, not asserted equal.
  2. the three adjoint kernels of csrc/train_ops.hip alone at their FPN and keypoint-tower shapes, each against the eager torch op
     that computes the same adjoint and nothing else: aten.upsample_bilinear2d_backward (NCHW, torch's layout), a zero fill +
     strided-slice assignment, reshape + permute + contiguous.

Method (measuring-on-mi355x): warm-up first; the two sides ALTERNATE inside one loop; a timed window is `inner` back-to-back
launches between two device events, `inner` chosen so that a window lasts milliseconds, not microseconds; the median, minimum
and maximum of --reps windows are reported per launch.  The clocks rocm-smi shows are noted before and after.  No speed target.
Runner and timer: tools/benchlib.py.

    python tools/train_step_bench.py [--reps 30] [--step-reps 10] [--skip-step] [--out profiles/train_step_bench.txt]
    python tools/train_step_bench.py --forward-f16x3 --out profiles/train_step_f16x3_forward_bench.txt

--forward-f16x3 adds two legs that alternate with the fp32-forward step in the same rounds: forward_precision='f16x3' with the fp32
backward, and with the f16x3 backward; their six losses are printed beside the fp32 forward's.
"""
import torch
import torch.nn.functional as F

import benchlib


def _row(lines, name, shape, inner, reps, hip, eager):
    t = benchlib.alternating([('hip', hip), ('eager', eager)], reps, warmup=3, inner=inner)
    h, e = benchlib.stats(t['hip']), benchlib.stats(t['eager'])
    lines.append('%-34s %-30s %5d   %8.4f %8.4f %8.4f   %8.4f %8.4f %8.4f   %5.2f'
                 % (name, shape, inner, h[0], h[1], h[2], e[0], e[1], e[2], e[0] / h[0]))


def kernels(dev, reps, lines):
    from stereo_rcnn_amd import _lib, autograd
    L = _lib.lib()
    lines.append('kernel                             shape                          inner   HIP ms: median min max        eager ms: median min max      eager / HIP')
    for (TH, TW), (H, W), inner in (((19, 63), (38, 125), 400), ((38, 125), (75, 249), 200), ((75, 249), (150, 497), 80)):
        B, C = 2, 256
        dy = torch.randn(B, H, W, C, device=dev)
        d_top = torch.empty(B, TH, TW, C, device=dev)
        g = dy.permute(0, 3, 1, 2).contiguous()
        hip = lambda: _lib.check(L.srcnn_upsample_add_backward(dy.data_ptr(), B, H, W, C, d_top.data_ptr(), TH, TW, _lib.stream()))
        eager = lambda: torch.ops.aten.upsample_bilinear2d_backward(g, [H, W], [B, C, TH, TW], True, None, None)
        _row(lines, 'srcnn_upsample_add_backward', '(%d,%d)->(%d,%d) x %d x %d' % (TH, TW, H, W, B, C), inner, reps, hip, eager)
    B, H, W, C = 2, 19, 63, 256
    dy, dx = torch.randn(B, 10, 32, C, device=dev), torch.empty(B, H, W, C, device=dev)
    hip = lambda: _lib.check(L.srcnn_subsample2_backward(dy.data_ptr(), B, 10, 32, C, dx.data_ptr(), H, W, _lib.stream()))

    def eager_sub():
        z = torch.zeros(B, H, W, C, device=dev)
        z[:, ::2, ::2] = dy
    _row(lines, 'srcnn_subsample2_backward', '(%d,%d,%d,%d)' % (B, H, W, C), 400, reps, hip, eager_sub)
    for M, inner in ((128, 100), (512, 30)):
        x = torch.randn(M, 14, 14, 1024, device=dev)
        for inverse in (False, True):
            src = autograd.pixel_shuffle2(x, 256) if inverse else x
            hip = lambda: autograd.pixel_shuffle2(src, 256, inverse=inverse)
            if inverse:
                eager = lambda: src.reshape(M, 14, 2, 14, 2, 256).permute(0, 1, 3, 2, 4, 5).contiguous()
            else:
                eager = lambda: src.reshape(M, 14, 14, 2, 2, 256).permute(0, 1, 3, 2, 4, 5).contiguous()
            _row(lines, 'srcnn_pixel_shuffle2 inverse=%d' % inverse, '(%d,14,14,4x256)' % M, inner, reps, hip, eager)


# ---------------------------------------------------------------------------------------- the same graph from eager torch ops
def _eager_roi_feat(maps, rois, A, im_height):
    """PyramidRoI_Feat (stereo_rcnn.py:110-139) from torch ops: level routing with nonzero (host waits, as the reference), per
    level the (A + 1) x (A + 1) lattice of roi_align_kernel.cu sampled with F.grid_sample, then the 2 x 2 / stride-1 mean."""
    r = rois.reshape(-1, 5)
    h, w = r[:, 4] - r[:, 2] + 1, r[:, 3] - r[:, 1] + 1
    level = torch.clamp(torch.round(torch.log(torch.sqrt(h * w) / 224.0) + 4), 2, 5)
    feats, index = [], []
    a = A + 1
    steps = torch.arange(a, device=r.device, dtype=torch.float32)
    for i, l in enumerate(range(2, 6)):
        idx = (level == l).nonzero().view(-1)
        if idx.numel() == 0:
            continue
        m = maps[i]
        H, W = int(m.shape[2]), int(m.shape[3])
        s = H / im_height
        q = r[idx]
        sw, sh = q[:, 1] * s, q[:, 2] * s
        bw, bh = ((q[:, 3] - q[:, 1]) * s + 1) / A, ((q[:, 4] - q[:, 2]) * s + 1) / A
        px = sw.view(-1, 1) + steps.view(1, -1) * bw.view(-1, 1)
        py = sh.view(-1, 1) + steps.view(1, -1) * bh.view(-1, 1)
        gx, gy = 2 * px / max(W - 1, 1) - 1, 2 * py / max(H - 1, 1) - 1
        grid = torch.stack((gx.view(-1, 1, a).expand(-1, a, a), gy.view(-1, a, 1).expand(-1, a, a)), 3)        # (k, a, a, 2)
        for b in range(int(m.shape[0])):           # one grid_sample per image: its rois' lattices stacked along the output height
            sel = (q[:, 0] == b).nonzero().view(-1)
            if sel.numel() == 0:
                continue
            k = int(sel.numel())
            lat = F.grid_sample(m[b:b + 1], grid[sel].reshape(1, k * a, a, 2), mode='bilinear', padding_mode='zeros', align_corners=True)
            lat = lat.view(-1, k, a, a).permute(1, 0, 2, 3)
            feats.append(F.avg_pool2d(lat, 2, 1))
            index.append(idx[sel])
    order = torch.sort(torch.cat(index, 0))[1]
    return torch.cat(feats, 0)[order]


def eager_step(model, im_left, im_right, im_height, taps, fixed_blocks):
    """stereo_rcnn.py:141-324 / stereo_rpn.py:62-138 from eager torch ops in float32 NCHW; the discrete results come from `taps`."""
    import loss_bench
    B = int(im_left.shape[0])

    def bn(m, x):
        return F.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, 1e-5)

    def conv(m, x):
        return F.conv2d(x, m.weight, m.bias, m.stride, m.padding)

    def block(blk, x):
        t = F.relu(bn(blk.bn1, conv(blk.conv1, x)))
        t = F.relu(bn(blk.bn2, conv(blk.conv2, t)))
        res = x if not hasattr(blk, 'downsample') else bn(blk.downsample[1], conv(blk.downsample[0], x))
        return F.relu(bn(blk.bn3, conv(blk.conv3, t)) + res)

    with torch.no_grad():
        x = torch.cat((im_left, im_right), 0)
        x = F.max_pool2d(F.relu(bn(model.RCNN_layer0[1], conv(model.RCNN_layer0[0], x))), 3, 2, 0, ceil_mode=True)
    c = []
    for li in (1, 2, 3, 4):
        with torch.set_grad_enabled(li > fixed_blocks):
            for blk in getattr(model, 'RCNN_layer%d' % li)[0]:
                x = block(blk, x)
        c.append(x)
    c2, c3, c4, c5 = c
    up_add = lambda top, lat: F.interpolate(top, size=lat.shape[2:], mode='bilinear', align_corners=True) + lat
    p5 = conv(model.RCNN_toplayer, c5)
    p4 = conv(model.RCNN_smooth1, up_add(p5, conv(model.RCNN_latlayer1, c4)))
    p3 = conv(model.RCNN_smooth2, up_add(p4, conv(model.RCNN_latlayer2, c3)))
    p2 = conv(model.RCNN_smooth3, up_add(p3, conv(model.RCNN_latlayer3, c2)))
    p6 = p5[:, :, ::2, ::2]
    levels = [p2, p3, p4, p5, p6]
    rpn = model.RCNN_rpn
    scores, boxes = [], []
    for p in levels:
        r = F.relu(conv(rpn.RPN_Conv, p))
        cat = torch.cat((r[:B], r[B:]), 1)
        scores.append(conv(rpn.RPN_cls_score, cat).permute(0, 2, 3, 1).contiguous().view(B, -1, 2))
        boxes.append(conv(rpn.RPN_bbox_pred_left_right, cat).permute(0, 2, 3, 1).contiguous().view(B, -1, 6))
    at = taps['anchor_targets']
    rpn_losses = loss_bench.eager_rpn(torch.cat(scores, 1), torch.cat(boxes, 1), at[0], at[1], at[2], at[3], at[4])
    pt = taps['proposal_targets']
    rois_left, rois_right = pt[0], pt[1]
    n = int(rois_left.shape[0]) * int(rois_left.shape[1])
    left_maps, right_maps = [p[:B] for p in levels[:4]], [p[B:] for p in levels[:4]]
    feat = torch.cat((_eager_roi_feat(left_maps, rois_left, 7, im_height), _eager_roi_feat(right_maps, rois_right, 7, im_height)), 1)
    t = F.dropout(F.relu(conv(model.RCNN_top[0], feat)), 0.2, True)
    t = F.dropout(F.relu(conv(model.RCNN_top[3], t)), 0.2, True).mean(3).mean(2)
    lin = lambda m: F.linear(t, m.weight, m.bias)
    k = _eager_roi_feat(left_maps, rois_left, 14, im_height)
    for i in (0, 2, 4, 6, 8, 10):
        k = F.relu(conv(model.RCNN_kpts[i], k))
    up = model.RCNN_kpts[12]
    k = F.relu(F.conv_transpose2d(k, up.weight, up.bias, stride=2))
    kpts = conv(model.kpts_class, k).sum(2)
    rcnn_losses = loss_bench.eager_rcnn(lin(model.RCNN_cls_score), lin(model.RCNN_bbox_pred), lin(model.RCNN_dim_orien_pred), kpts, pt[2],
                                        pt[3].view(1, n, 4), pt[4].view(1, n, 4), pt[5].view(1, n, 5), pt[6].view(1, n, 3).long(),
                                        pt[7].view(1, n, 3), pt[8].view(1, n, 4), pt[9].view(1, n, 4))
    return list(rpn_losses) + list(rcnn_losses)


def headline_case(dev):
    """The step's model and forward_train's nine inputs at the headline size (also tools/f16x3_maxima_bench.py's)."""
    from stereo_rcnn_amd import fixture, training
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    from stereo_rcnn_amd.model.utils.config import cfg
    cfg.TRAIN.RPN_PRE_NMS_TOP_N = training.PROPOSAL_MAX_PRE_NMS
    model = resnet(('__background__', 'Car'), 101)
    model.create_architecture()
    model.load_state_dict(fixture.make_state_dict(3))
    model = model.to(dev)
    Hh, Ww = 600, 1987
    g = torch.Generator().manual_seed(5)
    im_l = (torch.randn(1, 3, Hh, Ww, generator=g) * 40).to(dev)
    im_r = torch.roll(im_l, -20, 3)
    left = torch.tensor([[[200., 250., 420., 400., 1.], [900., 260., 1300., 520., 1.], [1500., 280., 1620., 360., 1.]]])
    right = left.clone()
    right[:, :, 0] -= 30
    right[:, :, 2] -= 30
    merge = left.clone()
    merge[:, :, 0] = right[:, :, 0]
    dim = torch.tensor([[[1.5, 1.6, 3.9, 0.3, 0.9]]]).expand(1, 3, 5).contiguous()
    w = (left[:, :, 2] - left[:, :, 0]).unsqueeze(2)
    kp = left[:, :, 0:1] + w * torch.tensor([0.3, 0., 0., 0., 0.1, 0.9])
    kp[:, :, 1:4] = -1
    args = [im_l, im_r, torch.tensor([[float(Hh), float(Ww), 1.0]])] + [t.to(dev) for t in (left, right, merge, dim, kp, torch.tensor([3]))]
    return model, args


def step(dev, reps, lines, f16x3=False, forward_f16x3=False):
    from stereo_rcnn_amd import training
    from stereo_rcnn_amd.model.utils.config import cfg
    model, args = headline_case(dev)
    im_l, im_r, Hh = args[0], args[1], 600
    gen = torch.Generator(device=dev).manual_seed(1)
    taps = {}
    first = training.forward_train(model, *args, generator=gen, taps=taps)
    data = {k: taps[k] for k in ('anchor_targets', 'proposal_targets')}
    del taps

    def clear():
        for p in model.parameters():
            p.grad = None

    def product():
        clear()
        sum(training.forward_train(model, *args, generator=gen)[8:14]).backward()

    def product_f16x3():
        clear()
        sum(training.forward_train(model, *args, generator=gen, backward_precision='f16x3')[8:14]).backward()

    def product_fwd16(bp):
        def run():
            clear()
            sum(training.forward_train(model, *args, generator=gen, forward_precision='f16x3', backward_precision=bp)[8:14]).backward()
        return run

    def eager():
        clear()
        sum(eager_step(model, im_l, im_r, float(Hh), data, cfg.RESNET.FIXED_BLOCKS)).backward()

    e_losses = eager_step(model, im_l, im_r, float(Hh), data, cfg.RESNET.FIXED_BLOCKS)
    lines.append('six losses, product (one draw of the dropout masks): ' + ' '.join('%.5f' % float(v.detach()) for v in first[8:14]))
    lines.append('six losses, eager  (its own dropout draw)          : ' + ' '.join('%.5f' % float(v.detach()) for v in e_losses))
    if forward_f16x3:
        gen16 = torch.Generator(device=dev).manual_seed(1)
        first16 = training.forward_train(model, *args, generator=gen16, forward_precision='f16x3')
        lines.append('six losses, product, forward_precision=f16x3 (same seed)  : ' + ' '.join('%.5f' % float(v.detach()) for v in first16[8:14]))
        del first16
    del first, e_losses
    torch.cuda.reset_peak_memory_stats()
    product()
    torch.cuda.synchronize()
    mem_p = torch.cuda.max_memory_allocated() / 2.0 ** 30
    torch.cuda.reset_peak_memory_stats()
    eager()
    torch.cuda.synchronize()
    mem_e = torch.cuda.max_memory_allocated() / 2.0 ** 30
    versions = [('hip', product), ('eager', eager)] + ([('f16x3', product_f16x3)] if f16x3 else [])
    if forward_f16x3:
        versions += [('fwd16', product_fwd16('f32')), ('fwd16_bwd16', product_fwd16('f16x3'))]
    r = {k: benchlib.stats(v) for k, v in benchlib.alternating(versions, reps, warmup=2).items()}
    lines.append('forward + backward of the training step, ResNet-101, 600 x 1987, B = 1, %d alternating runs, ms: median (min, max)' % reps)
    lines.append('  forward_train (exact-fp32 engine, target and proposal layers included): %.1f (%.1f, %.1f); peak memory %.2f GiB'
                 % (r['hip'] + (mem_p,)))
    lines.append('  eager torch ops (differentiable graph only, targets handed over as data): %.1f (%.1f, %.1f); peak memory %.2f GiB'
                 % (r['eager'] + (mem_e,)))
    if f16x3:
        lines.append('  forward_train, backward_precision=f16x3 (same forward; conv gradients by the 3 x f16 split): %.1f (%.1f, %.1f); '
                     'f16x3 / fp32 backward step: %.3f' % (r['f16x3'] + (r['f16x3'][0] / r['hip'][0],)))
    if forward_f16x3:
        lines.append('  forward_train, forward_precision=f16x3, fp32 backward (trainable convs and linears forward by the 3 x f16 split): '
                     '%.1f (%.1f, %.1f); / fp32-forward step: %.3f' % (r['fwd16'] + (r['fwd16'][0] / r['hip'][0],)))
        lines.append('  forward_train, forward_precision=f16x3, backward_precision=f16x3: %.1f (%.1f, %.1f); / fp32-forward step: %.3f'
                     % (r['fwd16_bwd16'] + (r['fwd16_bwd16'][0] / r['hip'][0],)))


def child(reps, step_reps, skip_step, f16x3=False, forward_f16x3=False):
    # torch starts HIP with this line, before the library loads: the process keeps the hardware-queue count of its environment
    lines = ['device: %s; the two sides alternate; a window is `inner` launches between two device events' % torch.cuda.get_device_name(0)]
    dev = benchlib.device()
    lines.append('clocks before: ' + benchlib.clocks())
    kernels(dev, reps, lines)
    if not skip_step:
        step(dev, step_reps, lines, f16x3 or forward_f16x3, forward_f16x3)
    lines.append('clocks after: ' + benchlib.clocks())
    print('\n'.join(lines))


def main():
    # the time limit: a run with the default arguments took 10 to 12 s, and 68 s as the first of its kind on a box
    benchlib.main(__file__, child, out='train_step_bench.txt', reps=30, timeout=300,
                  extra=[('--step-reps', dict(type=int, default=10)), ('--skip-step', dict(action='store_true')),
                         ('--f16x3', dict(action='store_true')),      # the whole step also with backward_precision='f16x3', alternating
                         ('--forward-f16x3', dict(action='store_true'))],     # ... and with forward_precision='f16x3', both backwards
                  header='# python tools/train_step_bench.py --reps %(reps)d --step-reps %(step_reps)d   (see the tool for what each line measures)')


if __name__ == '__main__':
    main()
