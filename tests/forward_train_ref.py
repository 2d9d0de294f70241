"""The case of tests/test_forward_train_gpu.py: inputs, the product run, and the float64 reference of the same graph.

Case: resnet(classes, 50) with fixture.make_state_dict(seed, layers=R50); B = 1, a 104 x 328 image pair (levels 26x82, 13x41,
7x21, 4x11, 2x6: every top-down step has a non-integer ratio); three synthetic ground-truth boxes with keypoints; cfg.TRAIN
RPN_BATCHSIZE 16, BATCH_SIZE 16, RPN_POST_NMS_TOP_N 40 (the sizes of tests/golden/reference_targets.npz), RPN_PRE_NMS_TOP_N 8192.

The reference is the same graph in float64 on the CPU from torch.nn.functional.  Every discrete decision is DATA taken from the
product's taps: the rois, all target-layer outputs, the dropout masks, and each ReLU as the product's own mask (a float64
forward of its own would put an activation that lies within a rounding error of zero on the other side of the ReLU).  ROIAlign
is tests/roi_align_backward_ref.py's roi_align_torch64 (the kernels' float32 lattice coordinates, a float64 blend that torch
differentiates) per level as tests/pyramid_roi_align_ref.py composes it, with that file's float64 level routing.
"""
import torch
import torch.nn.functional as F

CLASSES = ('__background__', 'Car')
H, W = 104, 328
# RPN_PRE_NMS_TOP_N: the case has 8604 anchors and srcnn_proposal_layer ranks at most 8192 candidates (training.PROPOSAL_MAX_PRE_NMS);
# the reference's 12000 would keep all of them, forward_train refuses it (test_forward_train_gpu.py checks that)
TRAIN_SIZES = {'RPN_BATCHSIZE': 16, 'BATCH_SIZE': 16, 'RPN_POST_NMS_TOP_N': 40, 'RPN_PRE_NMS_TOP_N': 8192}
LOSS_NAMES = ('rpn_loss_cls', 'rpn_loss_bbox_left_right', 'RCNN_loss_cls', 'RCNN_loss_bbox', 'RCNN_loss_dim_orien', 'RCNN_loss_kpts')


def inputs(seed=5):
    """CPU tensors: im_left, im_right, im_info, gt_boxes_left, gt_boxes_right, gt_boxes_merge, gt_dim_orien, gt_kpts, num_boxes.
    Three cars of different sizes, the right boxes shifted left by a disparity; keypoints inside the left box."""
    g = torch.Generator().manual_seed(seed)
    im_left = torch.randn(1, 3, H, W, generator=g) * 40.0
    im_right = torch.roll(im_left, -6, 3) + torch.randn(1, 3, H, W, generator=g) * 4.0
    im_info = torch.tensor([[float(H), float(W), 1.0]])
    left = torch.tensor([[20., 30., 75., 70., 1.], [120., 20., 215., 90., 1.], [250., 40., 290., 66., 1.]])
    disp = torch.tensor([8., 14., 5.])
    right = left.clone()
    right[:, 0] -= disp
    right[:, 2] -= disp
    merge = left.clone()
    merge[:, 0] = torch.min(left[:, 0], right[:, 0])
    merge[:, 2] = torch.max(left[:, 2], right[:, 2])
    dim_orien = torch.tensor([[1.5, 1.6, 3.9, 0.3, 0.9], [1.4, 1.7, 4.2, -0.5, 0.8], [1.6, 1.5, 3.6, 0.1, -0.9]])
    w = left[:, 2] - left[:, 0]
    # four perspective keypoints (one visible, -1 elsewhere as the reference's labels) + the left / right borders
    kpts = torch.full((3, 6), -1.0)
    kpts[0, 1], kpts[1, 2], kpts[2, 0] = left[0, 0] + 0.3 * w[0], left[1, 0] + 0.6 * w[1], left[2, 0] + 0.5 * w[2]
    kpts[:, 4] = left[:, 0] + 0.1 * w
    kpts[:, 5] = left[:, 0] + 0.9 * w
    u = lambda t: t.unsqueeze(0)
    return [im_left, im_right, im_info, u(left), u(right), u(merge), u(dim_orien), u(kpts), torch.tensor([3])]


def make_model(dev, seed=3):
    from stereo_rcnn_amd import fixture
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    model = resnet(CLASSES, 50)
    model.create_architecture()
    model.load_state_dict(fixture.make_state_dict(seed, layers=fixture.R50))
    return model.to(dev)


def patch_cfg(monkeypatch=None):
    from stereo_rcnn_amd.model.utils.config import cfg
    for k, v in TRAIN_SIZES.items():
        if monkeypatch is None:
            setattr(cfg.TRAIN, k, v)
        else:
            monkeypatch.setattr(cfg.TRAIN, k, v)


def run_product(dev, seed=5, model=None, gen_seed=11):
    """One forward_train + backward of the sum of the six losses.  Returns (the 15-tuple detached on the CPU, {name: grad} on the
    CPU, taps)."""
    from stereo_rcnn_amd import training
    model = make_model(dev) if model is None else model
    for p in model.parameters():
        p.grad = None
    gen = torch.Generator(device=dev).manual_seed(gen_seed)
    taps = {}
    args = [t.to(dev) if i != 2 else t for i, t in enumerate(inputs(seed))]          # im_info stays on the host
    out = training.forward_train(model, *args, generator=gen, taps=taps)
    sum(out[8:14]).backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return [o.detach().cpu() for o in out], grads, taps


# ------------------------------------------------------------------------------------------------ the reference graph
def _mean2x2(x):
    return 0.25 * (x[..., :-1, :-1] + x[..., :-1, 1:] + x[..., 1:, :-1] + x[..., 1:, 1:])


def _roi_feat(maps, rois, A, im_height, dtype):
    """PyramidRoI_Feat on NCHW maps of one eye: per level roi_align_backward_ref.roi_align_torch64 (float32 lattice coordinates
    as the kernels form them, float64 differentiable blend) on an (A + 1) lattice, then the 2x2 / stride-1 mean (RoIAlignAvg)."""
    import numpy as np
    import roi_align_backward_ref as RB
    rois = np.asarray(rois.detach().cpu().reshape(-1, 5).numpy(), np.float32)
    levels, _ = RB.pyramid_levels(rois)
    parts, order = [], []
    for l in range(4):
        idx = np.nonzero(levels == l)[0]
        if idx.size == 0:
            continue
        scale = float(np.float32(maps[l].shape[2] / float(im_height)))
        for i in idx:                                   # one roi at a time: roi_align_torch64 copies the whole map per roi
            lat = RB.roi_align_torch64(maps[l].double(), rois[i:i + 1], A + 1, A + 1, scale)
            parts.append(_mean2x2(lat).to(dtype))
            order.append(int(i))
    inv = torch.argsort(torch.tensor(order))
    return torch.cat(parts, 0)[inv]


def run_reference(state, taps, seed=5, dtype=torch.float64, trainable=()):
    """The graph of stereo_rcnn_amd.training.forward_train from torch.nn.functional on the CPU in `dtype`, every discrete
    decision taken from `taps`.  state: {name: CPU tensor} of the model; trainable: the names that get a gradient.  Returns
    (outputs dict, {name: grad})."""
    import losses_ref
    P = {k: v.detach().cpu().to(dtype).requires_grad_(k in trainable) for k, v in state.items() if v.is_floating_point()}
    cpu = lambda t: t.detach().cpu()
    im_left, im_right, im_info = inputs(seed)[:3]
    B = im_left.shape[0]

    def relu(name, t):                                  # the ReLU as the product's own mask (NHWC or (n, C) in the taps)
        m = cpu(taps[name]) > 0
        if m.dim() == 4:
            m = m.permute(0, 3, 1, 2)
        return t * m.reshape(t.shape).to(dtype)

    def bn(prefix, t):
        s = state[prefix + '.weight'].cpu().double() / torch.sqrt(state[prefix + '.running_var'].cpu().double() + 1e-5)
        sh = state[prefix + '.bias'].cpu().double() - state[prefix + '.running_mean'].cpu().double() * s
        return t * s.to(dtype).view(1, -1, 1, 1) + sh.to(dtype).view(1, -1, 1, 1)

    def conv(name, t, stride=1, pad=0):
        return F.conv2d(t, P[name + '.weight'], P.get(name + '.bias'), stride, pad)

    x = torch.cat((im_left, im_right), 0).to(dtype)
    x = relu('RCNN_layer0', bn('RCNN_layer0.1', conv('RCNN_layer0.0', x, 2, 3)))
    x = F.max_pool2d(x, 3, 2, 0, ceil_mode=True)
    c = []
    for li in (1, 2, 3, 4):
        b = 0
        while 'RCNN_layer%d.0.%d.conv1.weight' % (li, b) in P:
            p = 'RCNN_layer%d.0.%d' % (li, b)
            stride = 2 if (b == 0 and li > 1) else 1
            t = relu(p + '.conv1', bn(p + '.bn1', conv(p + '.conv1', x, stride)))
            t = relu(p + '.conv2', bn(p + '.bn2', conv(p + '.conv2', t, 1, 1)))
            res = x if p + '.downsample.0.weight' not in P else bn(p + '.downsample.1', conv(p + '.downsample.0', x, stride))
            x = relu(p + '.out', bn(p + '.bn3', conv(p + '.conv3', t)) + res)
            b += 1
        c.append(x)
    c2, c3, c4, c5 = c
    up_add = lambda top, lat: F.interpolate(top, size=lat.shape[2:], mode='bilinear', align_corners=True) + lat
    p5 = conv('RCNN_toplayer', c5)
    p4 = conv('RCNN_smooth1', up_add(p5, conv('RCNN_latlayer1', c4)), 1, 1)
    p3 = conv('RCNN_smooth2', up_add(p4, conv('RCNN_latlayer2', c3)), 1, 1)
    p2 = conv('RCNN_smooth3', up_add(p3, conv('RCNN_latlayer3', c2)), 1, 1)
    p6 = p5[:, :, ::2, ::2]
    levels = [p2, p3, p4, p5, p6]

    scores, bboxes = [], []
    for l, p in enumerate(levels):
        r = relu('RPN_Conv.%d' % l, conv('RCNN_rpn.RPN_Conv', p, 1, 1))
        cat = torch.cat((r[:B], r[B:]), 1)
        scores.append(conv('RCNN_rpn.RPN_cls_score', cat).permute(0, 2, 3, 1).reshape(B, -1, 2))
        bboxes.append(conv('RCNN_rpn.RPN_bbox_pred_left_right', cat).permute(0, 2, 3, 1).reshape(B, -1, 6))
    rpn_loss_cls, rpn_loss_box = losses_ref.rpn_losses(torch.cat(scores, 1), torch.cat(bboxes, 1),
                                                       *[cpu(t) for t in taps['anchor_targets']])

    targets = [cpu(t) for t in taps['proposal_targets']]
    rois_left, rois_right, label = targets[0], targets[1], targets[2].reshape(-1).long()
    n = label.numel()
    im_height = float(im_info[0][0])
    left_maps, right_maps = [p[:B] for p in levels[:4]], [p[B:] for p in levels[:4]]
    feat = torch.cat((_roi_feat(left_maps, rois_left, 7, im_height, dtype), _roi_feat(right_maps, rois_right, 7, im_height, dtype)), 1)
    keep = lambda name: cpu(taps[name]).to(dtype) / 0.8
    t = relu('RCNN_top.0', conv('RCNN_top.0', feat, 7).reshape(n, -1)) * keep('dropout1')
    t = relu('RCNN_top.3', conv('RCNN_top.3', t.reshape(n, -1, 1, 1)).reshape(n, -1)) * keep('dropout2')
    lin = lambda name: F.linear(t, P[name + '.weight'], P[name + '.bias'])
    bbox_all, dim_all, cls_score = lin('RCNN_bbox_pred'), lin('RCNN_dim_orien_pred'), lin('RCNN_cls_score')
    k = _roi_feat(left_maps, rois_left, 14, im_height, dtype)
    for i in (0, 2, 4, 6, 8, 10):
        k = relu('RCNN_kpts.%d' % i, conv('RCNN_kpts.%d' % i, k, 1, 1))
    k = relu('RCNN_kpts.12', F.conv_transpose2d(k, P['RCNN_kpts.12.weight'], P['RCNN_kpts.12.bias'], stride=2))
    kpts_pred_all = conv('kpts_class', k).sum(2)
    G = kpts_pred_all.shape[2]
    rcnn = losses_ref.rcnn_losses(cls_score, bbox_all, dim_all, kpts_pred_all, *targets[2:])
    all_losses = [rpn_loss_cls, rpn_loss_box] + list(rcnn)
    sum(all_losses).backward()
    sel = label.view(n, 1, 1)
    out = dict(zip(LOSS_NAMES, [l.detach().double() for l in all_losses]))
    out['cls_prob'] = F.softmax(cls_score, 1).detach()
    out['bbox_pred'] = torch.gather(bbox_all.reshape(n, -1, 6), 1, sel.expand(n, 1, 6)).squeeze(1).detach()
    out['dim_orien_pred'] = torch.gather(dim_all.reshape(n, -1, 5), 1, sel.expand(n, 1, 5)).squeeze(1).detach()
    out['kpts_prob'] = F.softmax(kpts_pred_all[:, :4, :].reshape(n, 4 * G), 1).detach()
    out['left_border_prob'] = F.softmax(kpts_pred_all[:, 4, :], 1).detach()
    out['right_border_prob'] = F.softmax(kpts_pred_all[:, 5, :], 1).detach()
    return out, {k_: v.grad.detach().double() for k_, v in P.items() if v.grad is not None}
