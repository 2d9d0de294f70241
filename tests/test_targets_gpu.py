"""GPU: the anchor and proposal target layers (csrc/targets.hip) against the reference's own layers
(tests/golden/reference_targets.npz, made by tests/golden/make_targets_golden.py) and the float32 CPU restatement
(tests/targets_ref.py).  Discrete results and everything made of +, -, *, / only are compared exactly; dw / dh, which go through
the device's logf, within tests/target_tolerances.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_tolerances as LT       # noqa: E402
import target_tolerances as TT     # noqa: E402
import targets_ref as ref          # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(HERE, 'golden', 'reference_targets.npz'))
P_NAMES = ('rois_left', 'rois_right', 'labels', 'bbox_targets_left', 'bbox_targets_right', 'dim_orien_targets', 'kpts_targets',
           'kpts_weight', 'inside_w', 'outside_w')


@pytest.fixture(scope='module')
def mods():
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd.model.rpn import anchor_target_layer, proposal_target_layer
    return anchor_target_layer, proposal_target_layer


@pytest.fixture(scope='module')
def anchor_case():
    """Golden inputs, the keys replayed from the reference's recorded permutations, and the restatement's result (computed once)."""
    t = torch.from_numpy
    shapes = [tuple(int(v) for v in s) for s in G['a_feat_shapes']]
    anchors = t(ref.pyramid_anchors_numpy(shapes))
    ins = dict(anchors=anchors, gt_left=t(G['a_gt_left']), gt_right=t(G['a_gt_right']), gt_merge=t(G['a_gt_merge']),
               im_info=t(G['a_im_info']))
    batch, num_fg = int(G['a_rpn_batchsize']), int(G['a_num_fg'])
    zeros = torch.zeros(2, anchors.shape[0], dtype=torch.int64)
    first = ref.anchor_targets(fg_keys=zeros, bg_keys=zeros, batch_size=batch, num_fg=num_fg, **ins)
    fk, bk = ref.anchor_keys_from_draws(first['candidates_fg'], first['candidates_bg'],
                                        ref.split_draws(G['a_draws'], G['a_draw_lengths']), batch, num_fg)
    fk, bk = t(fk), t(bk)
    return dict(ins=ins, shapes=shapes, batch=batch, num_fg=num_fg, fg_keys=fk, bg_keys=bk,
                ref=ref.anchor_targets(fg_keys=fk, bg_keys=bk, batch_size=batch, num_fg=num_fg, **ins))


@pytest.fixture(scope='module')
def proposal_case():
    ins = {k: torch.from_numpy(G['p_' + k]) for k in ('rois_left', 'rois_right', 'gt_left', 'gt_right', 'gt_dim_orien', 'gt_kpts')}
    S, fgq = int(G['p_rois_per_image']), int(G['p_fg_rois_per_image'])
    M = ins['rois_left'].shape[1] + ins['gt_left'].shape[1]
    first = ref.proposal_targets(fg_keys=np.zeros((2, M), dtype=np.int64), u=np.zeros((2, S)), rois_per_image=S,
                                 fg_rois_per_image=fgq, **ins)
    keys, u = ref.proposal_inputs_from_draws(first['fg_candidates'], first['bg_candidates'],
                                             ref.split_draws(G['p_draws'], G['p_draw_lengths']), S, fgq)
    keys, u = torch.from_numpy(keys), torch.from_numpy(u)
    return dict(ins=ins, S=S, fgq=fgq, M=M, fg_keys=keys, u=u,
                ref=ref.proposal_targets(fg_keys=keys, u=u, rois_per_image=S, fg_rois_per_image=fgq, **ins))


def _dev(d):
    return {k: v.cuda() for k, v in d.items()}


def _run_anchor(mods, c, fg_keys=None, bg_keys=None, **kw):
    a = mods[0]
    ins = _dev(c['ins'])
    out = a.anchor_targets(ins['anchors'], ins['gt_left'], ins['gt_right'], ins['gt_merge'], ins['im_info'],
                           (c['fg_keys'] if fg_keys is None else fg_keys).cuda(), (c['bg_keys'] if bg_keys is None else bg_keys).cuda(),
                           kw.pop('batch', c['batch']), kw.pop('num_fg', c['num_fg']), want_max_overlaps=True, **kw)
    return dict(zip(('labels', 'targets_left', 'targets_right', 'inside_w', 'outside_w', 'max_overlaps'), (o.cpu() for o in out)))


def _run_proposal(mods, c, ins=None, fg_keys=None, u=None):
    ins = _dev(c['ins'] if ins is None else ins)
    out = mods[1].proposal_targets(ins['rois_left'], ins['rois_right'], ins['gt_left'], ins['gt_right'], ins['gt_dim_orien'],
                                   ins['gt_kpts'], (c['fg_keys'] if fg_keys is None else fg_keys).cuda(),
                                   (c['u'] if u is None else u).cuda(), c['S'], c['fgq'], want_keep_inds=True)
    return dict(zip(P_NAMES + ('status', 'keep_inds'), (o.cpu() for o in out)))


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check_anchor(got, want, tol):
    for name in ('labels', 'inside_w', 'outside_w'):
        assert torch.equal(got[name], want[name]), name
    assert torch.equal(_bits(got['max_overlaps']), _bits(want['max_overlaps'])), 'max_overlaps bit-equal'
    for side in ('targets_left', 'targets_right'):
        assert torch.equal(_bits(got[side][..., :2]), _bits(want[side][..., :2])), side + ' dx dy bit-equal'
        err = float((got[side][..., 2:] - want[side][..., 2:]).abs().max())
        print('%s dw/dh max |kernel - restatement| = %.3e' % (side, err))
        assert err <= tol, (side, err)


def _check_proposal(got, want, tol):
    for name in ('rois_left', 'rois_right', 'labels', 'kpts_targets', 'kpts_weight', 'inside_w', 'outside_w', 'status',
                 'dim_orien_targets'):
        assert torch.equal(got[name], want[name]), name
    assert torch.equal(got['keep_inds'].long(), want['keep_inds']), 'selected roi rows'
    for side in ('bbox_targets_left', 'bbox_targets_right'):
        assert torch.equal(got[side][..., :2], want[side][..., :2]), side + ' dx dy'
        err = float((got[side][..., 2:] - want[side][..., 2:]).abs().max())
        print('%s dw/dh max |kernel - restatement| = %.3e' % (side, err))
        assert err <= tol, (side, err)


def test_anchor_golden(mods, anchor_case):
    """The reference's own layer, its permutations replayed as keys: labels, weights exactly; targets at the stored anchors."""
    got = _run_anchor(mods, anchor_case)
    assert torch.equal(got['labels'], torch.from_numpy(G['a_labels']).int())
    assert torch.equal(got['inside_w'], torch.from_numpy(G['a_inside_w']))
    assert torch.equal(got['outside_w'], torch.from_numpy(G['a_outside_w']))
    idx = torch.from_numpy(G['a_target_idx'])
    for side in ('targets_left', 'targets_right'):
        g, w = got[side].reshape(-1, 4)[idx], torch.from_numpy(G['a_' + side])
        assert torch.equal(_bits(g[:, :2]), _bits(w[:, :2])), side
        assert float((g[:, 2:] - w[:, 2:]).abs().max()) <= TT.ANCHOR_DWDH_ATOL
    _check_anchor(got, anchor_case['ref'], TT.ANCHOR_DWDH_ATOL)
    assert int((got['max_overlaps'] == -2).sum()) == int((anchor_case['ref']['max_overlaps'] == -2).sum()) > 0


def test_proposal_golden(mods, proposal_case):
    got = _run_proposal(mods, proposal_case)
    for name in ('rois_left', 'rois_right', 'labels', 'kpts_targets', 'kpts_weight', 'inside_w', 'outside_w'):
        assert torch.equal(got[name].float(), torch.from_numpy(G['p_out_' + name])), name
    for name in ('bbox_targets_left', 'bbox_targets_right', 'dim_orien_targets'):
        w = torch.from_numpy(G['p_out_' + name])
        assert float((got[name] - w).abs().max()) <= TT.PROPOSAL_DWDH_ATOL, name
        assert torch.equal(got[name][..., :2], w[..., :2]), name
    assert got['status'].tolist() == [0, 0]
    _check_proposal(got, proposal_case['ref'], TT.PROPOSAL_DWDH_ATOL)


def test_anchor_odd_size_and_noop_quota(mods, anchor_case):
    """N = 15345 - 7 is no multiple of any workgroup size; a quota above every candidate set: nothing is disabled."""
    c = dict(anchor_case)
    n = c['ins']['anchors'].shape[0] - 7
    c['ins'] = dict(c['ins'], anchors=c['ins']['anchors'][:n].clone())
    fk, bk = c['fg_keys'][:, :n].contiguous(), c['bg_keys'][:, :n].contiguous()
    want = ref.anchor_targets(fg_keys=fk, bg_keys=bk, batch_size=40000, num_fg=20000, **c['ins'])
    assert torch.equal(want['labels'] == 1, want['candidates_fg']) and torch.equal(want['labels'] == 0, want['candidates_bg'])
    got = _run_anchor(mods, c, fg_keys=fk, bg_keys=bk, batch=40000, num_fg=20000)
    _check_anchor(got, want, TT.ANCHOR_DWDH_ATOL)
    got = _run_anchor(mods, c, fg_keys=fk, bg_keys=bk)                    # and the golden quotas at the odd size
    _check_anchor(got, ref.anchor_targets(fg_keys=fk, bg_keys=bk, batch_size=c['batch'], num_fg=c['num_fg'], **c['ins']),
                  TT.ANCHOR_DWDH_ATOL)


def test_key_ties_keep_the_lowest_indices(mods, anchor_case, proposal_case):
    c = anchor_case
    same = torch.full_like(c['fg_keys'], 0x9ABCDEF0)
    got = _run_anchor(mods, c, fg_keys=same, bg_keys=same)
    cand_fg, cand_bg = c['ref']['candidates_fg'], c['ref']['candidates_bg']
    for b in range(2):
        fg, bg = torch.nonzero(cand_fg[b]).view(-1), torch.nonzero(cand_bg[b]).view(-1)
        n_fg = min(len(fg), c['num_fg'])
        assert torch.equal(torch.nonzero(got['labels'][b] == 1).view(-1), fg[:n_fg])
        assert torch.equal(torch.nonzero(got['labels'][b] == 0).view(-1), bg[:c['batch'] - len(fg)])
    p = proposal_case
    same = torch.full_like(p['fg_keys'], 7)
    got = _run_proposal(mods, p, fg_keys=same)
    want = ref.proposal_targets(fg_keys=same, u=p['u'], rois_per_image=p['S'], fg_rois_per_image=p['fgq'], **p['ins'])
    fg0 = torch.nonzero(want['fg_candidates'][0]).view(-1)
    assert got['keep_inds'][0, :p['fgq']].tolist() == fg0[:p['fgq']].tolist()
    _check_proposal(got, want, TT.PROPOSAL_DWDH_ATOL)


def test_proposal_branches_and_status(mods, proposal_case):
    """bg only (no ground truth), fg only, and neither (all-zero batch, status 1) in one batch of three images."""
    p = proposal_case
    K, R = 6, 5
    gt = torch.zeros(3, K, 5)
    gt[1, 0] = torch.tensor([50., 40., 149., 119., 1.])
    gt[2, 0] = torch.tensor([50., 40., 149., 119., 1.])
    rois = torch.zeros(3, R, 5)
    rois[0, :, 1:] = torch.tensor([10., 10., 60., 50.])                  # image 0: no ground truth -> every roi background
    rois[1, :, 1:] = torch.tensor([52., 41., 150., 118.])                # image 1: every roi foreground, none background
    rois[2, :, 1:] = torch.tensor([7., 7., 7., 7.])                      # image 2: zero-area rois (overlap -1) ...
    gt2 = gt.clone()
    gt2[2] = 0                                                           # ... and no ground truth: neither set exists
    ins = dict(rois_left=rois, rois_right=rois.clone(), gt_left=gt2, gt_right=gt2.clone(), gt_dim_orien=torch.rand(3, K, 5),
               gt_kpts=torch.rand(3, K, 6) * 100)
    keys = torch.arange(3 * (R + K)).view(3, R + K) * 977 % 31
    u = torch.rand(3, p['S'], dtype=torch.float64)
    c = dict(p, fg_keys=keys, u=u)
    want = ref.proposal_targets(fg_keys=keys, u=u, rois_per_image=p['S'], fg_rois_per_image=p['fgq'], **ins)
    assert want['status'].tolist() == [0, 0, 1] and int(want['labels'][1].min()) == 1 and int(want['labels'][0].max()) == 0
    got = _run_proposal(mods, c, ins=ins)
    _check_proposal(got, want, TT.PROPOSAL_DWDH_ATOL)
    assert not got['rois_left'][2].any() and not got['outside_w'][2].any()


def _layer_inputs(anchor_case):
    ins = _dev(anchor_case['ins'])
    return (torch.zeros(1, device='cuda'), ins['gt_left'], ins['gt_right'], ins['gt_merge'], ins['im_info'], None, anchor_case['shapes'])


def test_generator_modules(mods, anchor_case, proposal_case):
    a, p = mods
    layer = a._AnchorTargetLayer([16], [0.5, 1, 2], rpn_batchsize=anchor_case['batch'])
    inp = _layer_inputs(anchor_case)
    g = torch.Generator(device='cuda')
    runs = []
    for seed in (5, 5, 6):
        g.manual_seed(seed)
        runs.append([o.cpu() for o in layer(inp, generator=g)])
    assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[1])), "same seed, same outputs"
    assert not torch.equal(runs[0][0], runs[2][0]), "another seed, another selection"
    cand_fg, cand_bg = anchor_case['ref']['candidates_fg'], anchor_case['ref']['candidates_bg']
    for labels in (runs[0][0], runs[2][0]):
        for b in range(2):
            n_fg = int(cand_fg[b].sum())
            assert int((labels[b] == 1).sum()) == min(n_fg, anchor_case['num_fg'])
            assert int((labels[b] == 0).sum()) == min(int(cand_bg[b].sum()), anchor_case['batch'] - n_fg)
            assert bool(cand_fg[b][labels[b] == 1].all()) and bool(cand_bg[b][labels[b] == 0].all())
    player = p._ProposalTargetLayer(2, batch_size=proposal_case['S'])
    ins = _dev(proposal_case['ins'])
    args = (ins['rois_left'], ins['rois_right'], ins['gt_left'], ins['gt_right'], ins['gt_dim_orien'], ins['gt_kpts'], None)
    runs = []
    for seed in (5, 5, 6):
        g.manual_seed(seed)
        out = player(*args, generator=g, want_keep_inds=True)
        runs.append([o.cpu() for o in out] + [player.keep_inds.cpu()])
    assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[1]))
    assert not torch.equal(runs[0][-1], runs[2][-1])
    player.check_status()
    fg_c, bg_c = proposal_case['ref']['fg_candidates'], proposal_case['ref']['bg_candidates']
    for run in (runs[0], runs[2]):
        keep, labels = run[-1].long(), run[2]
        for b in range(2):
            n = min(int(fg_c[b].sum()), proposal_case['fgq'])
            assert int((labels[b] > 0).sum()) == n and len(set(keep[b, :n].tolist())) == n
            assert bool(fg_c[b][keep[b, :n]].all()) and bool(bg_c[b][keep[b, n:]].all())


def test_side_stream_and_graph_replay(mods, anchor_case, proposal_case):
    """Both layers on a non-default stream; one call of each captured as a single chain replays equal outputs."""
    a, p = mods
    ai, pi = _dev(anchor_case['ins']), _dev(proposal_case['ins'])
    fk, bk = a.as_key_bits(anchor_case['fg_keys'].cuda()), a.as_key_bits(anchor_case['bg_keys'].cuda())
    pk, u = a.as_key_bits(proposal_case['fg_keys'].cuda()), proposal_case['u'].cuda()

    def both():
        x = a.anchor_targets(ai['anchors'], ai['gt_left'], ai['gt_right'], ai['gt_merge'], ai['im_info'], fk, bk, anchor_case['batch'],
                             anchor_case['num_fg'], want_max_overlaps=True)
        y = p.proposal_targets(pi['rois_left'], pi['rois_right'], pi['gt_left'], pi['gt_right'], pi['gt_dim_orien'], pi['gt_kpts'],
                               pk, u, proposal_case['S'], proposal_case['fgq'], want_keep_inds=True)
        return list(x) + list(y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = both()
        eager = [o.clone() for o in eager]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            captured = both()
        for o in captured:
            o.fill_(0) if o.dtype != torch.int32 else o.fill_(-7)
        graph.replay()
    s.synchronize()
    for e, c in zip(eager, captured):
        assert torch.equal(e.cpu(), c.cpu())
    _check_anchor(dict(zip(('labels', 'targets_left', 'targets_right', 'inside_w', 'outside_w', 'max_overlaps'),
                           (o.cpu() for o in eager[:6]))), anchor_case['ref'], TT.ANCHOR_DWDH_ATOL)


def test_hand_off_to_the_losses(mods, anchor_case, proposal_case):
    """The layers' outputs go straight into rpn_losses / rcnn_losses; the losses equal those from the restatement's targets."""
    from stereo_rcnn_amd.model.stereo_rcnn import losses
    a, p = mods
    g = torch.Generator().manual_seed(3)
    ins = _dev(anchor_case['ins'])
    B, N = 2, ins['anchors'].shape[0]
    got = a.anchor_targets(ins['anchors'], ins['gt_left'], ins['gt_right'], ins['gt_merge'], ins['im_info'],
                           anchor_case['fg_keys'].cuda(), anchor_case['bg_keys'].cuda(), anchor_case['batch'], anchor_case['num_fg'])
    cls, box = torch.randn(B, N, 2, generator=g).cuda(), torch.randn(B, N, 6, generator=g).cuda()
    w = anchor_case['ref']
    l_got = losses.rpn_losses(cls, box, *got[:5])
    l_ref = losses.rpn_losses(cls, box, w['labels'].cuda(), w['targets_left'].cuda(), w['targets_right'].cuda(), w['inside_w'].cuda(),
                              w['outside_w'].cuda())
    tol = LT.MODULE_VALUE_REL
    for x, y in zip(l_got, l_ref):
        assert abs(float(x) - float(y)) <= tol * abs(float(y)), (float(x), float(y))
    pi = _dev(proposal_case['ins'])
    S = proposal_case['S']
    out = p.proposal_targets(pi['rois_left'], pi['rois_right'], pi['gt_left'], pi['gt_right'], pi['gt_dim_orien'], pi['gt_kpts'],
                             proposal_case['fg_keys'].cuda(), proposal_case['u'].cuda(), S, proposal_case['fgq'])
    n, n_cls = 2 * S, 3
    preds = (torch.randn(n, n_cls, generator=g).cuda(), torch.randn(n, 6 * n_cls, generator=g).cuda(),
             torch.randn(n, 5 * n_cls, generator=g).cuda(), torch.randn(n, 6, 28, generator=g).cuda())
    r = proposal_case['ref']
    l_got = losses.rcnn_losses(*preds, out[2], out[3], out[4], out[5], out[6], out[7], out[8], out[9])
    l_ref = losses.rcnn_losses(*preds, *(r[k].cuda() for k in ('labels', 'bbox_targets_left', 'bbox_targets_right', 'dim_orien_targets',
                                                               'kpts_targets', 'kpts_weight', 'inside_w', 'outside_w')))
    for x, y in zip(l_got, l_ref):
        assert abs(float(x) - float(y)) <= tol * abs(float(y)), (float(x), float(y))
