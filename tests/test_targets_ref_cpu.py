"""CPU: the float32 restatement of the two training target layers (tests/targets_ref.py) against the reference's own layers
(tests/golden/reference_targets.npz: inputs, recorded numpy draws, outputs), and direct cases against hand-computed values."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import targets_ref as ref      # noqa: E402

G = np.load(os.path.join(HERE, 'golden', 'reference_targets.npz'))
t = torch.from_numpy


def _bits(x):
    return x.contiguous().view(torch.int32)


def test_anchor_restatement_reproduces_the_reference():
    shapes = [tuple(int(v) for v in s) for s in G['a_feat_shapes']]
    anchors = t(ref.pyramid_anchors_numpy(shapes))
    assert anchors.shape == (15345, 4)
    ins = dict(anchors=anchors, gt_left=t(G['a_gt_left']), gt_right=t(G['a_gt_right']), gt_merge=t(G['a_gt_merge']), im_info=t(G['a_im_info']))
    batch, num_fg = int(G['a_rpn_batchsize']), int(G['a_num_fg'])
    zeros = torch.zeros(2, anchors.shape[0], dtype=torch.int64)
    first = ref.anchor_targets(fg_keys=zeros, bg_keys=zeros, batch_size=batch, num_fg=num_fg, **ins)
    fk, bk = ref.anchor_keys_from_draws(first['candidates_fg'], first['candidates_bg'],
                                        ref.split_draws(G['a_draws'], G['a_draw_lengths']), batch, num_fg)
    r = ref.anchor_targets(fg_keys=t(fk), bg_keys=t(bk), batch_size=batch, num_fg=num_fg, **ins)
    assert torch.equal(r['labels'], t(G['a_labels']).int())
    assert torch.equal(r['inside_w'], t(G['a_inside_w'])) and torch.equal(r['outside_w'], t(G['a_outside_w']))
    idx = t(G['a_target_idx'])
    for side in ('targets_left', 'targets_right'):          # dx, dy and (torch's CPU log on both sides) dw, dh: bit-equal
        assert torch.equal(_bits(r[side].reshape(-1, 4)[idx]), _bits(t(G['a_' + side]))), side
    # what the golden contains: more candidates than the quota in image 0, none in image 1 (no ground truth), and both kept counts
    assert first['candidates_fg'].sum(1).tolist() == [11, 0] and (r['labels'] == 1).sum(1).tolist() == [num_fg, 0]
    assert (r['labels'] == 0).sum(1).tolist() == [batch - 11, batch]
    assert float(r['outside_w'].max()) == 1.0 / batch       # the LAST image keeps `batch` examples; image 0 keeps 13


def test_proposal_restatement_reproduces_the_reference():
    ins = {k: t(G['p_' + k]) for k in ('rois_left', 'rois_right', 'gt_left', 'gt_right', 'gt_dim_orien', 'gt_kpts')}
    S, fgq = int(G['p_rois_per_image']), int(G['p_fg_rois_per_image'])
    M = ins['rois_left'].shape[1] + ins['gt_left'].shape[1]
    first = ref.proposal_targets(fg_keys=np.zeros((2, M), dtype=np.int64), u=np.zeros((2, S)), rois_per_image=S,
                                 fg_rois_per_image=fgq, **ins)
    keys, u = ref.proposal_inputs_from_draws(first['fg_candidates'], first['bg_candidates'],
                                             ref.split_draws(G['p_draws'], G['p_draw_lengths']), S, fgq)
    r = ref.proposal_targets(fg_keys=t(keys), u=t(u), rois_per_image=S, fg_rois_per_image=fgq, **ins)
    for name in ('rois_left', 'rois_right', 'labels', 'bbox_targets_left', 'bbox_targets_right', 'dim_orien_targets', 'kpts_targets',
                 'kpts_weight', 'inside_w', 'outside_w'):
        assert torch.equal(r[name].float(), t(G['p_out_' + name])), name
    assert r['status'].tolist() == [0, 0]
    assert first['fg_candidates'].sum(1).tolist() == [13, 2] and (r['labels'] > 0).sum(1).tolist() == [fgq, 2]
    assert 2 in r['labels'][0].tolist()                     # a class-2 row: boxes expanded, keypoints not
    row = r['labels'][0].tolist().index(2)
    assert r['inside_w'][0, row].tolist() == [1.0] * 4 and not r['kpts_weight'][0, row].any()


def _one_anchor_problem(boxes, gt, batch_size, num_fg, B=1, im=(100, 100), **kw):
    anchors = torch.tensor(boxes, dtype=torch.float32)
    g = torch.zeros(B, 2, 5)
    for b, rows in enumerate(gt):
        for k, row in enumerate(rows):
            g[b, k, :4] = torch.tensor(row, dtype=torch.float32)
    N = anchors.shape[0]
    keys = kw.pop('keys', torch.arange(N).repeat(B, 1))
    return ref.anchor_targets(anchors, g, g, g, torch.tensor([[im[0], im[1], 1.0]] * B), keys, keys, batch_size, num_fg, **kw)


def test_gt_max_zero_becomes_1e_5():
    # the one ground-truth box touches no anchor: its column maximum is 0; without the rule `overlaps == gt_max` would hold for
    # EVERY anchor (0 == 0) and all would be foreground; with it none is, and all are background (0 < 0.3)
    r = _one_anchor_problem([[0, 0, 9, 9], [20, 20, 29, 29]], [[[60, 60, 79, 79]]], 8, 4)
    assert r['labels'].tolist() == [[0, 0]] and r['max_overlaps'].tolist() == [[0.0, 0.0]]
    # and the zero-padded second row (overlap 0 by the zero-area mask) never makes an anchor foreground either
    r = _one_anchor_problem([[0, 0, 9, 9], [60, 60, 79, 79]], [[[60, 60, 79, 79]]], 8, 4)
    assert r['labels'].tolist() == [[0, 1]] and r['max_overlaps'].tolist() == [[0.0, 1.0]]
    assert r['inside_w'].tolist() == [[0.0, 1.0]] and r['outside_w'].tolist() == [[0.5, 0.5]]


def test_negative_num_bg_disables_every_background_anchor():
    # three anchors sit exactly on ground-truth boxes (3 foreground candidates), batch 2, quota 1: num_bg = 2 - 3 = -1
    boxes = [[0, 0, 9, 9], [20, 20, 29, 29], [40, 40, 49, 49], [70, 70, 79, 79], [80, 0, 89, 9]]
    g = torch.zeros(1, 3, 5)
    g[0, :, :4] = torch.tensor(boxes[:3], dtype=torch.float32)
    keys = torch.tensor([[5, 3, 9, 1, 2]])
    r = ref.anchor_targets(torch.tensor(boxes, dtype=torch.float32), g, g, g, torch.tensor([[100., 100., 1.]]), keys, keys, 2, 1)
    assert r['candidates_fg'].tolist() == [[True, True, True, False, False]]
    assert r['labels'].tolist() == [[-1, 1, -1, -1, -1]]              # the lowest key of the three stays; no background at all
    assert r['outside_w'].tolist() == [[0.0, 1.0, 0.0, 0.0, 0.0]]     # one example in the (only = last) image


def test_num_examples_is_the_last_images():
    # image 0: one foreground + three background anchors kept (4 examples); image 1: no ground truth, 4 background, quota keeps 2
    boxes = [[0, 0, 9, 9], [20, 20, 29, 29], [40, 40, 49, 49], [70, 70, 79, 79]]
    r = _one_anchor_problem(boxes, [[[0, 0, 9, 9]], []], 2, 1, B=2)
    # num_bg = 2 - sum_fg: image 0 keeps 1 fg + 1 bg, image 1 keeps 2 bg; the weights of BOTH images are 1 / 2 (image 1's count)
    assert r['labels'].tolist() == [[1, 0, -1, -1], [0, 0, -1, -1]]
    assert r['outside_w'].tolist() == [[0.5, 0.5, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0]]
    r = _one_anchor_problem(boxes, [[], [[0, 0, 9, 9]]], 4, 1, B=2)
    # image 0 keeps 4 bg, image 1 (the last) 1 fg + 3 bg = 4 -> 1 / 4 everywhere; with batch 3 the last image keeps 3 -> 1 / 3
    assert set(r['outside_w'].view(-1).tolist()) == {0.25}
    r = _one_anchor_problem(boxes, [[], [[0, 0, 9, 9]]], 3, 1, B=2)
    assert r['labels'].tolist() == [[0, 0, 0, -1], [1, 0, 0, -1]]
    assert set(r['outside_w'][r['labels'] >= 0].tolist()) == {float(np.float32(1.0) / np.float32(3.0))}


def test_outside_anchors_and_the_long_cast():
    # im_w = 50.9 -> (long) 50: x2 = 50 is outside (50 < 50 fails), x2 = 49 inside
    r = _one_anchor_problem([[40, 0, 49, 9], [41, 0, 50, 9], [-1, 0, 8, 9]], [[[40, 0, 49, 9]]], 4, 2, im=(100, 50.9))
    assert r['labels'].tolist() == [[1, -1, -1]] and r['max_overlaps'].tolist() == [[1.0, -2.0, -2.0]]
    assert not r['targets_left'][0, 1:].any()


def test_round_half_away_from_zero():
    x = torch.tensor([0.5, 1.5, 2.5, -0.5, -2.5, 2.4999998, 0.49999997, 13.0, -0.0])
    assert ref.round_half_away(x).tolist() == [1.0, 2.0, 3.0, -1.0, -3.0, 2.0, 0.0, 13.0, 0.0]
    assert torch.round(x).tolist()[:3] == [0.0, 2.0, 2.0]              # today's torch.round: half to even


def test_keypoint_tie_and_status():
    # one roi = the ground-truth box [0, 0, 55, 27] (width 56): a keypoint at x = 1 gives 1 * 28 / 56 = 0.5 -> 1 (half away; 0 if even)
    gt = torch.zeros(2, 2, 5)
    gt[0, 0] = torch.tensor([0., 0., 55., 27., 1.])
    rois = torch.zeros(2, 1, 5)
    rois[0, 0, 1:] = gt[0, 0, :4]
    rois[1, 0, 1:] = torch.tensor([3., 3., 3., 3.])                    # image 1: a zero-area roi and no ground truth
    kpts = torch.full((2, 2, 6), -1.0)
    kpts[0, 0] = torch.tensor([-1., 1., -1., -1., 5., 49.])
    r = ref.proposal_targets(rois, rois, gt, gt, torch.zeros(2, 2, 5), kpts, torch.zeros(2, 3, dtype=torch.int64),
                             np.full((2, 4), 0.99), 4, 1)
    assert r['status'].tolist() == [0, 1]
    assert r['labels'][0].tolist() == [1, 1, 1, 1]                     # fg only (no roi is background): drawn with replacement
    assert r['kpts_targets'][0, 0].tolist() == [1 * 28 + 1, 3, 25]     # type 1, pos round(0.5) = 1; 5 * 28 / 56 = 2.5 -> 3; 24.5 -> 25
    assert r['kpts_weight'][0, 0].tolist() == [1.0, 1.0, 1.0]
    for name in ('rois_left', 'labels', 'bbox_targets_left', 'dim_orien_targets', 'kpts_targets', 'kpts_weight', 'inside_w', 'outside_w'):
        assert not r[name][1].any(), name


def test_draw_conversion_helpers():
    cand = np.array([3, 5, 8, 9])
    perm = np.array([2, 0, 3, 1])
    keys = ref.anchor_keys_from_permutation(cand, perm, 12)
    # the reference disables cand[perm[:n - quota]]: with quota 1 that is everything but cand[perm[-1]] = 5, the lowest key
    kept = ref.lowest_ranked(t(cand), t(keys), 1)
    assert kept.tolist() == [5]
    assert sorted(ref.lowest_ranked(t(cand), t(keys), 2).tolist()) == sorted([5, 9])
    keys = ref.proposal_keys_from_permutation(cand, perm, 12)
    order = sorted(range(4), key=lambda j: keys[cand[j]])
    assert cand[order].tolist() == cand[perm].tolist()
    assert ref.u_from_rand([0.25, 0.75], 2, 4).tolist() == [0.0, 0.0, 0.25, 0.75]
    assert ref.with_replacement([0.0, 0.999999, 0.5], 7).tolist() == [0, 6, 3]
