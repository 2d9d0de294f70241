"""torch-CPU float32 restatement of the two training target layers and of bbox_overlaps_batch / bbox_transform_batch.

Reference: lib/model/rpn/anchor_target_layer.py:64-154, lib/model/rpn/proposal_target_layer.py:36-333,
lib/model/rpn/bbox_transform.py:38-77, 220-309.  The reference's operation order is kept (the overlaps and the dx / dy targets
are claimed bit-equal by the kernels' contract, include/srcnn_hip.h "training target layers"); what is restated differently is
exactly what the contract changes: the random draws are INPUTS (uint32 keys ranked by (key, index); float64 u per output row),
torch 0.3's round is made explicit (half away from zero), labels are integers, and an image with neither foreground nor
background gives zeros and status 1 instead of raising.  tests/test_targets_ref_cpu.py holds this file against the reference's
own layers (tests/golden/reference_targets.npz).
"""
import numpy as np
import torch

DEFAULTS = dict(negative_overlap=0.3, positive_overlap=0.7, clobber_positives=False, inside_weight=1.0,
                fg_thresh=0.5, bg_thresh_hi=0.5, bg_thresh_lo=0.0, kpts_grid=28,
                bbox_means=(0.0, 0.0, 0.0, 0.0), bbox_stds=(0.1, 0.1, 0.2, 0.2), dim_means=(1.6, 1.5, 4.0, 0.0, 0.0),
                dim_stds=(0.5, 0.5, 0.5, 0.5, 0.5), inside_weights=(1.0, 1.0, 1.0, 1.0))


def pyramid_anchors_numpy(feat_shapes, scales=(32, 64, 128, 256, 512), strides=(4, 8, 16, 32, 64), ratios=(0.5, 1, 2)):
    """The pyramid anchors (N, 4) float32 in the reference's order (level, y, x, ratio): centre -/+ half size in float64."""
    root = np.sqrt(np.asarray(ratios, dtype=np.float64))
    out = []
    for scale, stride, (h, w) in zip(scales, strides, feat_shapes):
        half = np.stack((0.5 * scale * root, 0.5 * (scale / root)), 1)                       # (3, 2): w / 2, h / 2
        cy, cx = np.meshgrid(np.arange(int(h)) * float(stride), np.arange(int(w)) * float(stride), indexing='ij')
        c = np.stack((cx, cy), 2).reshape(-1, 1, 2)
        out.append(np.concatenate((c - half, c + half), 2).reshape(-1, 4))
    return np.concatenate(out, 0).astype(np.float32)


def round_half_away(x):
    t = torch.trunc(x)
    return torch.where((x - t).abs() >= 0.5, t + torch.sign(x), t)


def u32(keys):
    """uint32 values of a key tensor (any integer dtype; int32 holds bit patterns)."""
    return torch.as_tensor(np.asarray(keys)).to(torch.int64) & 0xFFFFFFFF


def overlaps(boxes, gt):
    """bbox_overlaps_batch: boxes (N, 4) or (B, N, 4), gt (B, K, >=4) -> (B, N, K), with the zero-area masks."""
    B, K = gt.shape[0], gt.shape[1]
    if boxes.dim() == 2:
        boxes = boxes.unsqueeze(0).expand(B, -1, 4)
    boxes, gt = boxes.contiguous().float(), gt[:, :, :4].contiguous().float()
    N = boxes.shape[1]
    gx, gy = gt[:, :, 2] - gt[:, :, 0] + 1, gt[:, :, 3] - gt[:, :, 1] + 1
    garea = (gx * gy).view(B, 1, K)
    ax, ay = boxes[:, :, 2] - boxes[:, :, 0] + 1, boxes[:, :, 3] - boxes[:, :, 1] + 1
    aarea = (ax * ay).view(B, N, 1)
    b, q = boxes.view(B, N, 1, 4), gt.view(B, 1, K, 4)
    iw = torch.min(b[..., 2], q[..., 2]) - torch.max(b[..., 0], q[..., 0]) + 1
    iw = torch.where(iw < 0, torch.zeros_like(iw), iw)
    ih = torch.min(b[..., 3], q[..., 3]) - torch.max(b[..., 1], q[..., 1]) + 1
    ih = torch.where(ih < 0, torch.zeros_like(ih), ih)
    ua = aarea + garea - iw * ih
    ov = iw * ih / ua
    ov = ov.masked_fill(((gx == 1) & (gy == 1)).view(B, 1, K), 0.0)
    return ov.masked_fill(((ax == 1) & (ay == 1)).view(B, N, 1), -1.0)


def first_max(x, dim):
    """(max, FIRST argmax): what torch.max gives on the CPU, stated so that it does not depend on that."""
    m = x.max(dim, keepdim=True).values
    n = x.shape[dim]
    idx = torch.arange(n).view([-1 if d == (dim % x.dim()) else 1 for d in range(x.dim())]).expand_as(x)
    return m.squeeze(dim), torch.where(x == m, idx, torch.full_like(idx, n)).min(dim).values


def box_transform(ex, gt):
    """bbox_transform_batch: ex (N, 4) or (B, N, 4), gt (B, N, 4) -> (B, N, 4)."""
    ex, gt = ex.float(), gt.float()
    ew, eh = ex[..., 2] - ex[..., 0] + 1.0, ex[..., 3] - ex[..., 1] + 1.0
    ecx, ecy = ex[..., 0] + 0.5 * ew, ex[..., 1] + 0.5 * eh
    gw, gh = gt[..., 2] - gt[..., 0] + 1.0, gt[..., 3] - gt[..., 1] + 1.0
    gcx, gcy = gt[..., 0] + 0.5 * gw, gt[..., 1] + 0.5 * gh
    return torch.stack(((gcx - ecx) / ew, (gcy - ecy) / eh, torch.log(gw / ew), torch.log(gh / eh)), -1)


def lowest_ranked(cand_idx, keys_row, quota):
    """The `quota` lowest candidates by (key, index), as a sorted index tensor."""
    k = u32(keys_row)[cand_idx]
    order = sorted(range(len(cand_idx)), key=lambda j: (int(k[j]), int(cand_idx[j])))
    return cand_idx[torch.as_tensor(sorted(order[:max(quota, 0)]), dtype=torch.long)]


def anchor_targets(anchors, gt_left, gt_right, gt_merge, im_info, fg_keys, bg_keys, batch_size, num_fg, **kw):
    """-> dict(labels (B, N) int32, targets_left, targets_right (B, N, 4), inside_w, outside_w (B, N), max_overlaps (B, N),
    candidates_fg / candidates_bg (B, N) bool: the labels before any subsampling)."""
    P = dict(DEFAULTS, **kw)
    anchors, gt_left, gt_right, gt_merge = anchors.float(), gt_left.float(), gt_right.float(), gt_merge.float()
    B, K, N = gt_left.shape[0], gt_left.shape[1], anchors.shape[0]
    im_w, im_h = float(int(im_info[0][1])), float(int(im_info[0][0]))
    inside = (anchors[:, 0] >= 0) & (anchors[:, 1] >= 0) & (anchors[:, 2] < im_w) & (anchors[:, 3] < im_h)
    inds = torch.nonzero(inside).view(-1)
    a = anchors[inds]
    n = inds.numel()
    labels = torch.full((B, n), -1, dtype=torch.int32)
    ov = overlaps(a, gt_merge)
    max_ov, arg = first_max(ov, 2)
    gt_max = ov.max(1).values.clone()
    neg, pos = np.float32(P['negative_overlap']), np.float32(P['positive_overlap'])
    if not P['clobber_positives']:
        labels[max_ov < neg] = 0
    gt_max[gt_max == 0] = 1e-5
    keep = (ov == gt_max.view(B, 1, K)).sum(2)
    labels[keep > 0] = 1
    labels[max_ov >= pos] = 1
    if P['clobber_positives']:
        labels[max_ov < neg] = 0
    cand_fg, cand_bg = labels == 1, labels == 0
    sum_fg, sum_bg = cand_fg.sum(1), cand_bg.sum(1)
    for i in range(B):
        if int(sum_fg[i]) > num_fg:
            fg = torch.nonzero(cand_fg[i]).view(-1)
            labels[i, fg] = -1
            labels[i, lowest_ranked(fg, fg_keys[i][inds], num_fg)] = 1
        num_bg = batch_size - int(sum_fg[i])               # sum_fg BEFORE the foreground subsample, as the reference
        if int(sum_bg[i]) > num_bg:
            bg = torch.nonzero(cand_bg[i]).view(-1)
            labels[i, bg] = -1
            labels[i, lowest_ranked(bg, bg_keys[i][inds], num_bg)] = 0
    rows = torch.arange(B).view(B, 1)
    tl = box_transform(a, gt_left[rows, arg][:, :, :4])
    tr = box_transform(a, gt_right[rows, arg][:, :, :4])
    inside_w = torch.zeros(B, n)
    inside_w[labels == 1] = P['inside_weight']
    num_examples = (labels[B - 1] >= 0).sum()              # the loop's leftover `i`: the LAST image
    w = (torch.ones((), dtype=torch.float32) / num_examples.float())
    outside_w = torch.zeros(B, n)
    outside_w[labels >= 0] = w

    def unmap(x, fill):
        out = torch.full((B, N) + tuple(x.shape[2:]), fill, dtype=x.dtype)
        out[:, inds] = x
        return out
    return dict(labels=unmap(labels, -1), targets_left=unmap(tl, 0.0), targets_right=unmap(tr, 0.0), inside_w=unmap(inside_w, 0.0),
                outside_w=unmap(outside_w, 0.0), max_overlaps=unmap(max_ov, -2.0), candidates_fg=unmap(cand_fg, False),
                candidates_bg=unmap(cand_bg, False))


def with_replacement(u_rows, count):
    return torch.as_tensor(np.floor(np.asarray(u_rows, dtype=np.float64) * count), dtype=torch.long).clamp(0, max(count - 1, 0))


def proposal_targets(rois_left, rois_right, gt_left, gt_right, gt_dim_orien, gt_kpts, fg_keys, u, rois_per_image, fg_rois_per_image,
                     **kw):
    """-> dict of the ten outputs (labels, kpts_targets int32), status (B) int32, keep_inds (B, S) long, and the candidate sets
    fg_candidates / bg_candidates (B, R + K) bool."""
    P = dict(DEFAULTS, **kw)
    f = lambda t: torch.as_tensor(np.asarray(t)).float()
    rois_left, rois_right, gt_left, gt_right, gt_dim_orien, gt_kpts = (f(t) for t in (rois_left, rois_right, gt_left, gt_right,
                                                                                   gt_dim_orien, gt_kpts))
    B, R, K, S = rois_left.shape[0], rois_left.shape[1], gt_left.shape[1], rois_per_image
    app_l, app_r = torch.zeros_like(gt_left), torch.zeros_like(gt_right)
    app_l[:, :, 1:5], app_r[:, :, 1:5] = gt_left[:, :, :4], gt_right[:, :, :4]
    all_l, all_r = torch.cat((rois_left, app_l), 1), torch.cat((rois_right, app_r), 1)
    ml, al = first_max(overlaps(all_l[:, :, 1:5], gt_left), 2)
    mr, ar = first_max(overlaps(all_r[:, :, 1:5], gt_right), 2)
    fg_t, hi, lo = np.float32(P['fg_thresh']), np.float32(P['bg_thresh_hi']), np.float32(P['bg_thresh_lo'])
    fg_c = (ml >= fg_t) & (mr >= fg_t) & (al == ar)
    bg_c = ((ml < hi) & (ml >= lo)) | ((mr < hi) & (mr >= lo))
    keep = torch.zeros(B, S, dtype=torch.long)
    fg_rows = [0] * B
    status = torch.zeros(B, dtype=torch.int32)
    for i in range(B):
        fg, bg = torch.nonzero(fg_c[i]).view(-1), torch.nonzero(bg_c[i]).view(-1)
        if len(fg) and len(bg):
            n = min(fg_rois_per_image, len(fg))
            k = u32(fg_keys[i])[fg]
            order = sorted(range(len(fg)), key=lambda j: (int(k[j]), int(fg[j])))
            keep[i, :n] = fg[torch.as_tensor(order[:n], dtype=torch.long)]
            keep[i, n:] = bg[with_replacement(u[i][n:], len(bg))]
            fg_rows[i] = n
        elif len(fg):
            keep[i], fg_rows[i] = fg[with_replacement(u[i], len(fg))], S
        elif len(bg):
            keep[i] = bg[with_replacement(u[i], len(bg))]
        else:
            status[i] = 1
    rows = torch.arange(B).view(B, 1)
    sl, sr = all_l[rows, keep].clone(), all_r[rows, keep].clone()
    sl[:, :, 0] = sr[:, :, 0] = rows.float()
    a_l, a_r = al[rows, keep], ar[rows, keep]
    cls = gt_left[:, :, 4][rows, a_l].clone()
    for i in range(B):
        cls[i, fg_rows[i]:] = 0
    tl = (box_transform(sl[:, :, 1:5], gt_left[rows, a_l][:, :, :4]) - f(P['bbox_means'])) / f(P['bbox_stds'])
    tr = (box_transform(sr[:, :, 1:5], gt_right[rows, a_r][:, :, :4]) - f(P['bbox_means'])) / f(P['bbox_stds'])
    dim = (gt_dim_orien[rows, a_l] - f(P['dim_means'])) / f(P['dim_stds'])
    grid = P['kpts_grid']
    start, width = sl[:, :, 1:2], (sl[:, :, 3] - sl[:, :, 1] + 1).unsqueeze(2)
    t = round_half_away((gt_kpts[rows, a_l] - start) * grid / width)
    t = torch.where(t < 0, torch.full_like(t, -225.0), t)
    t = torch.where(t > grid - 1, torch.full_like(t, -225.0), t)
    pos, typ = first_max(t[:, :, :4], 2)
    kp = torch.cat(((typ.float() * grid + pos).unsqueeze(2), t[:, :, 4:]), 2)
    kw_ = torch.where(kp < 0, torch.zeros_like(kp), torch.ones_like(kp))
    kp = torch.where(kp < 0, torch.zeros_like(kp), kp)
    pos_rows, one_rows = (cls > 0).unsqueeze(2), (cls == 1).unsqueeze(2)
    zero = lambda x, m: torch.where(m, x, torch.zeros_like(x))
    inside = zero(f(P['inside_weights']).expand(B, S, 4), pos_rows)
    out = dict(rois_left=sl, rois_right=sr, labels=cls.to(torch.int32), bbox_targets_left=zero(tl, pos_rows),
               bbox_targets_right=zero(tr, pos_rows), dim_orien_targets=zero(dim, pos_rows),
               kpts_targets=zero(kp, one_rows).to(torch.int32), kpts_weight=zero(kw_, one_rows), inside_w=inside,
               outside_w=(inside > 0).float(), status=status, keep_inds=keep, fg_candidates=fg_c, bg_candidates=bg_c)
    for i in range(B):
        if status[i]:
            for name in ('rois_left', 'rois_right', 'labels', 'bbox_targets_left', 'bbox_targets_right', 'dim_orien_targets',
                         'kpts_targets', 'kpts_weight', 'inside_w', 'outside_w', 'keep_inds'):
                out[name][i] = 0
    return out


# ---------------------------------------------------------------- the reference's recorded numpy draws -> keys and u
def anchor_keys_from_permutation(cand_idx, perm, N):
    """anchor_target_layer.py:115-117 / :126-128 disables candidates perm[:n - quota]: any map that DEcreases along the
    permutation makes those the highest-ranked.  cand_idx: the candidates' anchor indices in ascending order."""
    keys = np.zeros(N, dtype=np.int64)
    n = len(perm)
    keys[np.asarray(cand_idx)[np.asarray(perm)]] = n - 1 - np.arange(n)
    return keys


def proposal_keys_from_permutation(fg_idx, perm, M):
    """proposal_target_layer.py:254-255 keeps fg_inds[perm[:n]] in that order: key[fg_inds[perm[j]]] = j."""
    keys = np.zeros(M, dtype=np.int64)
    keys[np.asarray(fg_idx)[np.asarray(perm)]] = np.arange(len(perm))
    return keys


def u_from_rand(rand, first_row, S):
    """np.random.rand(S - first_row) feeds output rows first_row .. S-1."""
    u = np.zeros(S, dtype=np.float64)
    u[first_row:] = np.asarray(rand, dtype=np.float64)
    return u


def split_draws(flat, lengths):
    """The golden file keeps the recorded draws as one float64 vector and the length of each call, in call order."""
    out, o = [], 0
    for n in lengths:
        out.append(np.asarray(flat[o:o + int(n)]))
        o += int(n)
    return out


def anchor_keys_from_draws(cand_fg, cand_bg, draws, batch_size, num_fg):
    """Replays anchor_target_layer.py:107-128's calls to np.random.permutation (draws: their results in call order) as
    (fg_keys, bg_keys) (B, N) int64.  cand_*: (B, N) bool, the labels before subsampling."""
    cand_fg, cand_bg = np.asarray(cand_fg), np.asarray(cand_bg)
    B, N = cand_fg.shape
    fg_keys, bg_keys = np.zeros((B, N), dtype=np.int64), np.zeros((B, N), dtype=np.int64)
    draws = list(draws)
    for i in range(B):
        fg, bg = np.nonzero(cand_fg[i])[0], np.nonzero(cand_bg[i])[0]
        if len(fg) > num_fg:
            fg_keys[i] = anchor_keys_from_permutation(fg, draws.pop(0).astype(np.int64), N)
        if len(bg) > batch_size - len(fg):
            bg_keys[i] = anchor_keys_from_permutation(bg, draws.pop(0).astype(np.int64), N)
    assert not draws, "every recorded draw is used"
    return fg_keys, bg_keys


def proposal_inputs_from_draws(fg_c, bg_c, draws, S, fg_quota):
    """Replays proposal_target_layer.py:246-283's calls to np.random (draws in call order) as (fg_keys (B, M) int64, u (B, S))."""
    fg_c, bg_c = np.asarray(fg_c), np.asarray(bg_c)
    B, M = fg_c.shape
    keys, u = np.zeros((B, M), dtype=np.int64), np.zeros((B, S), dtype=np.float64)
    draws = list(draws)
    for i in range(B):
        fg, nbg = np.nonzero(fg_c[i])[0], int(bg_c[i].sum())
        if len(fg) and nbg:
            keys[i] = proposal_keys_from_permutation(fg, draws.pop(0).astype(np.int64), M)
            u[i] = u_from_rand(draws.pop(0), min(fg_quota, len(fg)), S)
        elif len(fg) or nbg:
            u[i] = u_from_rand(draws.pop(0), 0, S)
    assert not draws, "every recorded draw is used"
    return keys, u
