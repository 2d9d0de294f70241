"""Generates tests/golden/reference_targets.npz by running the REFERENCE's own _AnchorTargetLayer and _ProposalTargetLayer
(lib/model/rpn/anchor_target_layer.py, proposal_target_layer.py of the reference tree) on the CPU under reference_shims.install(...).
Runs where the reference is present only; the tests read the .npz.

Added in memory for these two layers (nothing of the reference is edited or copied):
  * `long = int` in the anchor layer's namespace (py2 builtin, anchor_target_layer.py:70-71);
  * `Tensor.index(i)` as indexing (torch 0.3 method, proposal_target_layer.py:214);
  * the modules' `np` is a proxy whose `random.permutation` / `random.rand` record every draw and forward to numpy.
cfg is set in memory to the small test configuration (RPN_BATCHSIZE 16, BATCH_SIZE 16).  The file holds data only: inputs, the
recorded draws (one vector + the length of each call, in call order; the anchor layer's are all permutations: int32) and every output.
torch.round is half-to-even today and was half-away-from-zero in torch 0.3: asserted below that no keypoint quotient of these
inputs lies within 1e-3 of a .5 tie, so the two rules agree here.
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
warnings.filterwarnings('ignore')

import numpy as np   # noqa: E402
import torch         # noqa: E402

from oracle import ops as oracle_ops          # noqa: E402
import reference_shims                        # noqa: E402

reference_shims.install(oracle_ops)
import targets_ref                            # noqa: E402

FEAT_SHAPES = [(48, 80), (24, 40), (12, 20), (6, 10), (3, 5)]       # a 192 x 320 image
IM_H, IM_W, K = 192, 320, 6
RPN_BATCHSIZE, BATCH_SIZE, R = 16, 16, 40


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def permutation(self, n):
        out = np.random.permutation(n)
        self.calls.append(np.asarray(out, dtype=np.float64))
        return out

    def rand(self, *shape):
        out = np.random.rand(*shape)
        self.calls.append(np.asarray(out, dtype=np.float64).reshape(-1))
        return out

    def take(self):
        calls, self.calls = self.calls, []
        flat = np.concatenate(calls) if calls else np.zeros(0)
        return flat, np.asarray([len(c) for c in calls], dtype=np.int64)


class _NumpyProxy(object):
    def __init__(self, recorder):
        self.random = recorder

    def __getattr__(self, name):
        return getattr(np, name)


def ground_truth():
    """(B = 2, K, 5) left / right / merge, zero-padded: image 0 has three boxes, image 1 none (anchor case) or one (proposals)."""
    left = np.zeros((2, K, 5), dtype=np.float32)
    left[0, 0] = [100, 60, 131, 91, 1]
    left[0, 1] = [201.3, 40.2, 262.7, 101.9, 1]
    left[0, 2] = [36.5, 52.25, 150.75, 168.5, 2]
    right = left.copy()
    for k, d in enumerate((6.0, 9.5, 14.25)):
        right[0, k, 0] -= d
        right[0, k, 2] -= d
    merge = left.copy()
    merge[0, :3, 0] = np.minimum(left[0, :3, 0], right[0, :3, 0])
    merge[0, :3, 2] = np.maximum(left[0, :3, 2], right[0, :3, 2])
    return left, right, merge


def anchor_case(rec, d):
    import model.rpn.anchor_target_layer as atl
    from model.utils.config import cfg
    atl.long, atl.np = int, _NumpyProxy(rec)
    cfg.TRAIN.RPN_BATCHSIZE = RPN_BATCHSIZE
    left, right, merge = ground_truth()
    im_info = np.asarray([[IM_H, IM_W, 1.0]] * 2, dtype=np.float32)
    layer = atl._AnchorTargetLayer(cfg.FEAT_STRIDE, cfg.ANCHOR_RATIOS)
    np.random.seed(11)
    t = torch.from_numpy
    out = layer((torch.zeros(1), t(left), t(right), t(merge), t(im_info), None, FEAT_SHAPES))
    flat, lengths = rec.take()
    labels = out[0].numpy()
    num_fg = int(cfg.TRAIN.RPN_FG_FRACTION * RPN_BATCHSIZE)
    # what the golden must contain
    anchors = atl.generate_anchors_all_pyramids(np.array(cfg.FPN_ANCHOR_SCALES), cfg.ANCHOR_RATIOS, FEAT_SHAPES,
                                                np.array(cfg.FPN_FEAT_STRIDES), cfg.FPN_ANCHOR_STRIDE).astype(np.float32)
    ref = targets_ref.anchor_targets(t(anchors), t(left), t(right), t(merge), t(im_info), torch.zeros(2, len(anchors)),
                                     torch.zeros(2, len(anchors)), RPN_BATCHSIZE, num_fg)
    sum_fg = ref['candidates_fg'].sum(1).tolist()
    print('anchors', anchors.shape, 'fg candidates', sum_fg, 'bg candidates', ref['candidates_bg'].sum(1).tolist(),
          'kept fg', (labels == 1).sum(1), 'kept bg', (labels == 0).sum(1), 'draw lengths', lengths)
    assert sum_fg[0] > num_fg, "more foreground candidates than the quota"
    assert sum_fg[1] < num_fg, "fewer foreground candidates than the quota"
    assert RPN_BATCHSIZE - sum_fg[0] > 0, "image 0 keeps a positive background quota"
    assert (left[0, 3:] == 0).all() and (left[1] == 0).all(), "zero-padded rows and an image with no ground truth"
    inside = ref['max_overlaps'][0] > -2
    levels = np.cumsum([0] + [3 * h * w for h, w in FEAT_SHAPES])
    per_level = [int(inside[levels[i]:levels[i + 1]].sum()) for i in range(5)]
    assert all(per_level[:3]) and per_level[3:] == [0, 0], per_level
    # the (B, N, 4) targets are kept at every labelled anchor and at every 37th anchor (inside or not); anchors outside are zero
    tl, tr = out[1].numpy(), out[2].numpy()
    assert not tl[:, ~inside.numpy()].any() and not tr[:, ~inside.numpy()].any()
    pick = np.zeros(labels.shape, dtype=bool)
    pick[:, ::37] = True
    pick |= labels >= 0
    idx = np.nonzero(pick.reshape(-1))[0].astype(np.int64)
    assert np.array_equal(anchors, targets_ref.pyramid_anchors_numpy(FEAT_SHAPES)), "the anchors are rebuilt by the tests, not stored"
    d.update(a_gt_left=left, a_gt_right=right, a_gt_merge=merge, a_im_info=im_info,
             a_feat_shapes=np.asarray(FEAT_SHAPES, dtype=np.int64), a_rpn_batchsize=np.int64(RPN_BATCHSIZE), a_num_fg=np.int64(num_fg),
             a_draws=flat.astype(np.int32), a_draw_lengths=lengths, a_labels=labels.astype(np.int8), a_target_idx=idx,
             a_targets_left=tl.reshape(-1, 4)[idx], a_targets_right=tr.reshape(-1, 4)[idx],
             a_inside_w=out[3].numpy(), a_outside_w=out[4].numpy())


def proposal_case(rec, d):
    import model.rpn.proposal_target_layer as ptl
    from model.utils.config import cfg
    ptl.np = _NumpyProxy(rec)
    torch.Tensor.index = lambda self, idx: self[idx]
    cfg.TRAIN.BATCH_SIZE = BATCH_SIZE
    left, right, _ = ground_truth()
    left[1, 0] = [150.4, 70.3, 229.2, 139.6, 1]           # image 1: one box
    right[1, 0] = left[1, 0] - np.float32([11.5, 0, 11.5, 0, 0])
    rng = np.random.RandomState(5)
    dim_orien = np.zeros((2, K, 5), dtype=np.float32)
    kpts = np.zeros((2, K, 6), dtype=np.float32)
    for b, k in ((0, 0), (0, 1), (0, 2), (1, 0)):
        x1, x2 = left[b, k, 0], left[b, k, 2]
        w = x2 - x1 + 1
        dim_orien[b, k] = [1.5 + rng.rand(), 1.4 + 0.3 * rng.rand(), 3.5 + rng.rand(), rng.rand() * 2 - 1, rng.rand() * 2 - 1]
        kpts[b, k, :4] = -1
        kpts[b, k, rng.randint(4)] = x1 + (0.13 + 0.7 * rng.rand()) * w
        kpts[b, k, 4], kpts[b, k, 5] = x1 + 0.07 * w, x1 + 0.91 * w
    rois_l = np.zeros((2, R, 5), dtype=np.float32)
    rois_r = np.zeros((2, R, 5), dtype=np.float32)
    for b in range(2):
        rois_l[b, :, 0] = rois_r[b, :, 0] = b
        real = [k for k in range(K) if left[b, k, 4] > 0]
        n_near = 9 if b == 0 else 1
        for r in range(R):
            if r < n_near:                                 # near a ground-truth box on both sides: foreground
                k = real[r % len(real)]
                j = rng.uniform(-3, 3, 4).astype(np.float32)
                rois_l[b, r, 1:] = left[b, k, :4] + j
                rois_r[b, r, 1:] = right[b, k, :4] + j
            else:                                          # anywhere: mostly background
                x, y = rng.uniform(0, IM_W - 60), rng.uniform(0, IM_H - 60)
                w, h = rng.uniform(20, 120), rng.uniform(20, 100)
                box = np.float32([x, y, min(x + w, IM_W - 1), min(y + h, IM_H - 1)])
                rois_l[b, r, 1:] = box
                rois_r[b, r, 1:] = box - np.float32([8, 0, 8, 0])
        # a roi whose left side sits on box 0 and whose right side sits on box 1: the assignments disagree
    rois_l[0, 9, 1:] = left[0, 0, :4] + np.float32([1, -1, 2, 1])
    rois_r[0, 9, 1:] = right[0, 1, :4] + np.float32([-1, 1, 1, -2])
    t = torch.from_numpy
    layer = ptl._ProposalTargetLayer(2)
    np.random.seed(12)
    out = layer(t(rois_l), t(rois_r), t(left), t(right), t(dim_orien), t(kpts), None)
    flat, lengths = rec.take()
    fg_quota = int(np.round(cfg.TRAIN.FG_FRACTION * BATCH_SIZE))
    ref = targets_ref.proposal_targets(rois_l, rois_r, left, right, dim_orien, kpts, np.zeros((2, R + K), dtype=np.int64),
                                       np.zeros((2, BATCH_SIZE)), BATCH_SIZE, fg_quota)
    n_fg = ref['fg_candidates'].sum(1).tolist()
    print('fg candidates', n_fg, 'bg candidates', ref['bg_candidates'].sum(1).tolist(), 'draw lengths', lengths)
    assert n_fg[0] > fg_quota, "more foreground candidates than the quota"
    assert 0 < n_fg[1] < fg_quota, "fewer foreground candidates than the quota"
    assert (left[0, 3:] == 0).all() and (left[1, 1:] == 0).all(), "zero-padded ground-truth rows"
    all_l = torch.cat((t(rois_l)[:, :, 1:], t(left)[:, :, :4]), 1)
    all_r = torch.cat((t(rois_r)[:, :, 1:], t(right)[:, :, :4]), 1)
    ml, al = targets_ref.first_max(targets_ref.overlaps(all_l, t(left)), 2)
    mr, ar = targets_ref.first_max(targets_ref.overlaps(all_r, t(right)), 2)
    assert bool(((ml >= 0.5) & (mr >= 0.5) & (al != ar)).any()), "a roi whose left and right assignments disagree"
    # no keypoint quotient near a .5 tie (torch.round today vs. torch 0.3)
    for b in range(2):
        for k in range(K):
            if left[b, k, 4] <= 0:
                continue
            x1 = all_l[b, :, 0:1]
            q = (t(kpts)[b, k].view(1, 6) - x1) * 28 / (all_l[b, :, 2:3] - x1 + 1)
            frac = (q - torch.floor(q) - 0.5).abs()
            sel = (al[b] == k) & ref['fg_candidates'][b]
            assert float(frac[sel].min()) > 1e-3, "a keypoint quotient within 1e-3 of a .5 tie"
    names = ('rois_left', 'rois_right', 'labels', 'bbox_targets_left', 'bbox_targets_right', 'dim_orien_targets', 'kpts_targets',
             'kpts_weight', 'inside_w', 'outside_w')
    d.update(p_rois_left=rois_l, p_rois_right=rois_r, p_gt_left=left, p_gt_right=right, p_gt_dim_orien=dim_orien, p_gt_kpts=kpts,
             p_rois_per_image=np.int64(BATCH_SIZE), p_fg_rois_per_image=np.int64(fg_quota), p_draws=flat, p_draw_lengths=lengths)
    for name, o in zip(names, out):
        d['p_out_' + name] = o.numpy().astype(np.float32)


def main():
    rec, d = _Recorder(), {}
    with torch.no_grad():
        anchor_case(rec, d)
        proposal_case(rec, d)
    path = os.path.join(HERE, 'reference_targets.npz')
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
