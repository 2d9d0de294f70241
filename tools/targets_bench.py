"""The training target layers: the HIP kernels against the same computation composed from eager torch ops on the device.

    python tools/targets_bench.py [--out profiles/targets_bench.txt] [--reps 40]

Shapes: the anchor layer on the pyramid of a 375 x 1242 image (maps 94x311, 47x156, 24x78, 12x39, 6x20, 3 anchors per location
= 117 078 anchors), K = 30 ground-truth rows of which 8 are boxes, RPN_BATCHSIZE 512 (the config's); the proposal layer at
R = 2000 rois + K = 30, 512 rois per image, foreground fraction 0.25; both at B = 1 and B = 4.
  * hip   : stereo_rcnn_amd.model.rpn.anchor_target_layer.anchor_targets / proposal_target_layer.proposal_targets with the
            keys and u already on the device (one memset + three launches, and one launch; no host read);
  * eager : the reference's composition (anchor_target_layer.py:64-154, proposal_target_layer.py:36-333) in torch ops on the
            same device, with the kernels' sampling rule (keys ranked by (key, index), u per output row) in place of numpy's
            draws so that both sides select the same rows: the (B, N, K) overlap temporaries, nonzero, the per-image
            `sum_fg[i] > num_fg` reads, the per-image candidate counts -- the host waits the reference has.  The reference's
            Python loop over every foreground roi (:92-100) is NOT reproduced (vectorised here, which favours the eager side).
One process, warm (5 untimed runs of each); the two versions ALTERNATE, every run is timed with device events and ends in a
synchronise; medians of --reps runs, with min and max.  The two versions' labels are compared before timing.
Runner and timer: tools/benchlib.py."""
import benchlib

MAPS = [(94, 311), (47, 156), (24, 78), (12, 39), (6, 20)]
IM_H, IM_W, K, REAL, R = 375, 1242, 30, 8, 2000


def overlaps(boxes, gt):
    """bbox_overlaps_batch (bbox_transform.py:230-305): boxes (B, N, 4), gt (B, K, 4) -> (B, N, K)."""
    B, N, K_ = boxes.shape[0], boxes.shape[1], gt.shape[1]
    gx, gy = gt[:, :, 2] - gt[:, :, 0] + 1, gt[:, :, 3] - gt[:, :, 1] + 1
    ax, ay = boxes[:, :, 2] - boxes[:, :, 0] + 1, boxes[:, :, 3] - boxes[:, :, 1] + 1
    b, q = boxes.view(B, N, 1, 4), gt.view(B, 1, K_, 4)
    iw = (torch.min(b[..., 2], q[..., 2]) - torch.max(b[..., 0], q[..., 0]) + 1).clamp_(min=0)
    ih = (torch.min(b[..., 3], q[..., 3]) - torch.max(b[..., 1], q[..., 1]) + 1).clamp_(min=0)
    ua = (ax * ay).view(B, N, 1) + (gx * gy).view(B, 1, K_) - iw * ih
    ov = iw * ih / ua
    ov.masked_fill_(((gx == 1) & (gy == 1)).view(B, 1, K_), 0)
    return ov.masked_fill_(((ax == 1) & (ay == 1)).view(B, N, 1), -1)


def transform(ex, gt):
    ew, eh = ex[..., 2] - ex[..., 0] + 1.0, ex[..., 3] - ex[..., 1] + 1.0
    ecx, ecy = ex[..., 0] + 0.5 * ew, ex[..., 1] + 0.5 * eh
    gw, gh = gt[..., 2] - gt[..., 0] + 1.0, gt[..., 3] - gt[..., 1] + 1.0
    gcx, gcy = gt[..., 0] + 0.5 * gw, gt[..., 1] + 0.5 * gh
    return torch.stack(((gcx - ecx) / ew, (gcy - ecy) / eh, torch.log(gw / ew), torch.log(gh / eh)), -1)


def ranked(cand, keys_row):
    """Candidate indices in (key, index) order."""
    k = (keys_row[cand].to(torch.int64) & 0xFFFFFFFF) << 31 | cand
    return cand[torch.argsort(k)]


def eager_anchor(anchors, gt_left, gt_right, gt_merge, im_info, fg_keys, bg_keys, batch, num_fg):
    B, N = gt_left.shape[0], anchors.shape[0]
    keep = (anchors[:, 0] >= 0) & (anchors[:, 1] >= 0) & (anchors[:, 2] < int(im_info[0][1])) & (anchors[:, 3] < int(im_info[0][0]))
    inds = torch.nonzero(keep).view(-1)                                             # host waits, as the reference
    a = anchors[inds, :]
    n = inds.size(0)
    labels = gt_left.new_full((B, n), -1)
    ov = overlaps(a.view(1, n, 4).expand(B, n, 4).contiguous(), gt_merge[:, :, :4].contiguous())
    max_ov, arg = torch.max(ov, 2)
    gt_max, _ = torch.max(ov, 1)
    labels[max_ov < 0.3] = 0
    gt_max[gt_max == 0] = 1e-5
    keepn = torch.sum(ov.eq(gt_max.view(B, 1, -1).expand_as(ov)), 2)
    if torch.sum(keepn) > 0:
        labels[keepn > 0] = 1
    labels[max_ov >= 0.7] = 1
    sum_fg, sum_bg = torch.sum((labels == 1).int(), 1), torch.sum((labels == 0).int(), 1)
    for i in range(B):
        if sum_fg[i] > num_fg:
            fg = torch.nonzero(labels[i] == 1).view(-1)
            labels[i][ranked(fg, fg_keys[i][inds])[num_fg:]] = -1
        num_bg = batch - int(sum_fg[i])
        if sum_bg[i] > num_bg:
            bg = torch.nonzero(labels[i] == 0).view(-1)
            labels[i][ranked(bg, bg_keys[i][inds])[max(num_bg, 0):]] = -1
    arg = arg + (torch.arange(0, B, device=arg.device) * gt_left.size(1)).view(B, 1)
    tl = transform(a, gt_left.view(-1, 5)[arg.view(-1), :].view(B, -1, 5)[:, :, :4])
    tr = transform(a, gt_right.view(-1, 5)[arg.view(-1), :].view(B, -1, 5)[:, :, :4])
    inside = gt_left.new_zeros(B, n)
    outside = gt_left.new_zeros(B, n)
    inside[labels == 1] = 1.0
    w = 1.0 / torch.sum(labels[B - 1] >= 0)
    outside[labels == 1] = w
    outside[labels == 0] = w

    def unmap(x, fill):
        out = x.new_full((B, N) + tuple(x.shape[2:]), fill)
        out[:, inds] = x
        return out
    return unmap(labels, -1), unmap(tl, 0), unmap(tr, 0), unmap(inside, 0), unmap(outside, 0)


def eager_proposal(rois_l, rois_r, gt_l, gt_r, gt_dim, gt_kpts, keys, u, S, fgq):
    B, K_ = gt_l.shape[0], gt_l.shape[1]
    dev = gt_l.device
    app_l, app_r = torch.zeros_like(gt_l), torch.zeros_like(gt_r)
    app_l[:, :, 1:5], app_r[:, :, 1:5] = gt_l[:, :, :4], gt_r[:, :, :4]
    all_l, all_r = torch.cat([rois_l, app_l], 1), torch.cat([rois_r, app_r], 1)
    ml, al = torch.max(overlaps(all_l[:, :, 1:5].contiguous(), gt_l[:, :, :4].contiguous()), 2)
    mr, ar = torch.max(overlaps(all_r[:, :, 1:5].contiguous(), gt_r[:, :, :4].contiguous()), 2)
    labels = gt_l[:, :, 4].contiguous().view(-1)[(torch.arange(0, B, device=dev).view(-1, 1) * K_ + al).view(-1)].view(B, -1)
    lab = labels.new_zeros(B, S)
    out_l, out_r = all_l.new_zeros(B, S, 5), all_r.new_zeros(B, S, 5)
    g_l, g_r, g_dim, g_k = all_l.new_zeros(B, S, 5), all_l.new_zeros(B, S, 5), all_l.new_zeros(B, S, 5), all_l.new_zeros(B, S, 6)
    for i in range(B):
        fg = torch.nonzero((ml[i] >= 0.5) & (mr[i] >= 0.5) & (al[i] == ar[i])).view(-1)
        bg = torch.nonzero(((ml[i] < 0.5) & (ml[i] >= 0.0)) | ((mr[i] < 0.5) & (mr[i] >= 0.0))).view(-1)
        nf, nb = fg.numel(), bg.numel()                                             # host waits, as the reference
        if nf > 0 and nb > 0:
            n = min(fgq, nf)
            keep = torch.cat([ranked(fg, keys[i])[:n], bg[torch.floor(u[i, n:] * nb).long()]], 0)
        elif nf > 0:
            n, keep = S, fg[torch.floor(u[i] * nf).long()]
        else:
            n, keep = 0, bg[torch.floor(u[i] * nb).long()]
        lab[i].copy_(labels[i][keep])
        lab[i][n:] = 0
        out_l[i], out_r[i] = all_l[i][keep], all_r[i][keep]
        out_l[i, :, 0] = out_r[i, :, 0] = i
        g_l[i], g_r[i] = gt_l[i][al[i][keep]], gt_r[i][ar[i][keep]]
        g_dim[i], g_k[i] = gt_dim[i][al[i][keep]], gt_kpts[i][al[i][keep]]
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    tl = (transform(out_l[:, :, 1:5], g_l[:, :, :4]) - f((0., 0., 0., 0.))) / f((.1, .1, .2, .2))
    tr = (transform(out_r[:, :, 1:5], g_r[:, :, :4]) - f((0., 0., 0., 0.))) / f((.1, .1, .2, .2))
    dim = (g_dim - f((1.6, 1.5, 4.0, 0., 0.))) / f((.5, .5, .5, .5, .5))
    start = out_l[:, :, 1].unsqueeze(2).expand(-1, -1, 6)
    width = (out_l[:, :, 3] - out_l[:, :, 1] + 1).unsqueeze(2).expand(-1, -1, 6)
    q = (g_k - start) * 28 / width
    t = torch.trunc(q)
    t = torch.where((q - t).abs() >= 0.5, t + torch.sign(q), t)
    t[t < 0] = -225
    t[t > 27] = -225
    pos, typ = torch.max(t[:, :, :4], 2)
    kp = torch.cat((typ.float().unsqueeze(2) * 28 + pos.unsqueeze(2), t[:, :, 4:]), 2)
    kw = torch.ones_like(kp)
    kw[kp < 0] = 0
    kp[kp < 0] = 0
    pos_rows, one_rows = (lab > 0).unsqueeze(2).float(), (lab == 1).unsqueeze(2).float()
    inside = pos_rows.expand(B, S, 4).contiguous()
    return (out_l, out_r, lab, tl * pos_rows, tr * pos_rows, dim * pos_rows, (kp * one_rows).long(), kw * one_rows, inside,
            (inside > 0).float())


def make_inputs(B, dev, seed=0):
    g = torch.Generator().manual_seed(seed + B)
    rnd = lambda *s: torch.rand(*s, generator=g)
    left, right = torch.zeros(B, K, 5), torch.zeros(B, K, 5)
    x, y = rnd(B, REAL) * (IM_W - 260) + 30, rnd(B, REAL) * (IM_H - 170) + 10
    w, h = rnd(B, REAL) * 200 + 30, rnd(B, REAL) * 120 + 25
    d = rnd(B, REAL) * 25 + 3
    left[:, :REAL] = torch.stack((x, y, x + w, y + h, torch.ones(B, REAL)), 2)
    right[:, :REAL] = torch.stack((x - d, y, x + w - d, y + h, torch.ones(B, REAL)), 2)
    merge = left.clone()
    merge[:, :, 0] = torch.min(left[:, :, 0], right[:, :, 0])
    rois_l, rois_r = torch.zeros(B, R, 5), torch.zeros(B, R, 5)
    k = torch.randint(0, REAL, (B, R), generator=g)
    near = rnd(B, R, 1) < 0.2                                  # a fifth of the proposals sit on a ground-truth box
    bx, by = rnd(B, R) * (IM_W - 200), rnd(B, R) * (IM_H - 120)
    far = torch.stack((bx, by, bx + rnd(B, R) * 180 + 16, by + rnd(B, R) * 100 + 16), 2)
    jit = (rnd(B, R, 4) - 0.5) * 12
    rows = torch.arange(B).view(B, 1)
    rois_l[:, :, 1:] = torch.where(near, left[rows, k][:, :, :4] + jit, far)
    rois_r[:, :, 1:] = torch.where(near, right[rows, k][:, :, :4] + jit, far - torch.tensor([9., 0., 9., 0.]))
    dim, kpts = rnd(B, K, 5) * 2, torch.full((B, K, 6), -1.0)
    kpts[:, :REAL, 1] = left[:, :REAL, 0] + 0.37 * (left[:, :REAL, 2] - left[:, :REAL, 0])
    kpts[:, :REAL, 4], kpts[:, :REAL, 5] = left[:, :REAL, 0] + 3.3, left[:, :REAL, 2] - 4.1
    im_info = torch.tensor([[IM_H, IM_W, 1.0]] * B)
    return [t.to(dev) for t in (left, right, merge, im_info, rois_l, rois_r, dim, kpts)]


def child(reps):
    global torch                                    # (the module's functions use it; the parent process does not load it)
    import numpy as np
    import torch
    from stereo_rcnn_amd.model.rpn import anchor_target_layer as atl, proposal_target_layer as ptl
    from stereo_rcnn_amd.model.utils.config import cfg
    dev = benchlib.device()
    anchors = atl.pyramid_anchors(MAPS, dev)
    N = anchors.shape[0]
    batch, num_fg = cfg.TRAIN.RPN_BATCHSIZE, int(cfg.TRAIN.RPN_FG_FRACTION * cfg.TRAIN.RPN_BATCHSIZE)
    S, fgq = cfg.TRAIN.BATCH_SIZE, int(np.round(cfg.TRAIN.FG_FRACTION * cfg.TRAIN.BATCH_SIZE))
    g = torch.Generator(device=dev).manual_seed(1)
    for B in (1, 4):
        left, right, merge, im_info, rois_l, rois_r, dim, kpts = make_inputs(B, dev)
        fk, bk, pk = atl.draw_keys((B, N), dev, g), atl.draw_keys((B, N), dev, g), atl.draw_keys((B, R + K), dev, g)
        u = torch.rand((B, S), dtype=torch.float64, device=dev, generator=g)
        cases = [
            ('anchor targets, B = %d, %d anchors, K = %d (%d boxes), batch %d' % (B, N, K, REAL, batch),
             lambda: atl.anchor_targets(anchors, left, right, merge, im_info, fk, bk, batch, num_fg),
             lambda: eager_anchor(anchors, left, right, merge, im_info, fk, bk, batch, num_fg), 0),
            ('proposal targets, B = %d, R = %d, K = %d, %d rois per image' % (B, R, K, S),
             lambda: ptl.proposal_targets(rois_l, rois_r, left, right, dim, kpts, pk, u, S, fgq),
             lambda: eager_proposal(rois_l, rois_r, left, right, dim, kpts, pk, u, S, fgq), 2),
        ]
        for title, hip_fn, eager_fn, label_at in cases:
            a, b = hip_fn(), eager_fn()
            torch.cuda.synchronize()
            la, lb = a[label_at].long(), b[label_at].long()
            print(title)
            print('  labels equal: %s   (foreground %d, background / other %d)'
                  % (bool(torch.equal(la, lb)), int((la > 0).sum()), int((la == 0).sum())))
            assert torch.equal(la, lb), 'the two versions disagree'
            times = benchlib.alternating([('hip', hip_fn), ('eager', eager_fn)], reps, warmup=5)
            for name, t in times.items():
                print('  %s: median %.3f ms (min %.3f, max %.3f, %d runs)' % ((name,) + benchlib.stats(t) + (reps,)))
            print('  hip / eager = %.3f' % (benchlib.stats(times['hip'])[0] / benchlib.stats(times['eager'])[0]))


def main():
    benchlib.main(__file__, child, out='targets_bench.txt', reps=40, timeout=300,
                  header='# python tools/targets_bench.py --reps %(reps)d   (see the tool for what each line measures)')


if __name__ == '__main__':
    main()
