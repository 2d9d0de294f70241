"""tests/proposal_ref.py pinned on the CPU: its five stages chained equal oracle.proposal.proposal_layer exactly, the decode bound
of tests/proposal_tolerances.py holds for the oracle's float32 path and cannot hide the classic index / formula slips, and every
input generator of tests/test_proposal_stages_gpu.py has the property it exists for."""
import numpy as np
import pytest
import torch

from oracle import proposal as oprop
import proposal_ref as ref
import proposal_tolerances as ptol

KITTI = [[38, 125], [19, 63], [10, 32], [5, 16], [3, 8]]


def _existing_inputs(which):
    """The inputs of test_ops_gpu.py's two proposal tests, draw for draw."""
    A = ref.num_anchors(KITTI)
    if which == 'batched':
        g = torch.Generator().manual_seed(11)
        sc = torch.rand(3, A, generator=g)
        sc[1] = torch.round(sc[1] / 0.01) * 0.01
        sc[2] = 0.5
        deltas = (torch.randn(3, A, 6, generator=g) * 0.3).contiguous()
        return sc, deltas, torch.tensor([[600.0, 1987.0, 1.6]] * 3), 1000, 150
    pre, quant = which
    g = torch.Generator().manual_seed(pre)
    sc = torch.rand(1, A, generator=g)
    sc = torch.round(sc / quant) * quant if quant < 1.0 else torch.full_like(sc, 0.75)
    deltas = (torch.randn(1, A, 6, generator=g) * 0.3).contiguous()
    return sc, deltas, torch.tensor([[600.0, 1987.0, 1.6]]), pre, 120


@pytest.mark.parametrize("which", [(500, 0.01), (1000, 0.001), (6000, 0.05), (300, 1.0), 'batched'], ids=str)
def test_chained_stages_equal_the_oracle_exactly(which):
    """Order, float32 dets, both keep lists, the RoIs and the padding, B = 1 and B = 3."""
    sc, deltas, info, pre, post = _existing_inputs(which)
    probs = torch.stack((1 - sc, sc), 2).contiguous()
    rl, rr, ex = oprop.proposal_layer(probs, deltas, info, KITTI, pre_nms_top_n=pre, post_nms_top_n=post)
    got = ref.layer(sc.numpy(), deltas.numpy(), info.numpy(), KITTI, pre, post)
    for b in range(sc.shape[0]):
        assert np.array_equal(got['order'][b], ex['order'][b].numpy())
        assert np.array_equal(got['dets_left'][b], ex['dets_left'][b].numpy())
        assert np.array_equal(got['dets_right'][b], ex['dets_right'][b].numpy())
        assert np.array_equal(got['keep_left'][b], ex['keep_left'][b]) and np.array_equal(got['keep_right'][b], ex['keep_right'][b])
        assert got['count'][b] == len(ex['keep'][b])
        assert (got['rois_left'][b, got['count'][b]:] == np.array([b, 0, 0, 0, 0], np.float32)).all()
    assert np.array_equal(got['rois_left'], rl.numpy()) and np.array_equal(got['rois_right'], rr.numpy())


def test_restated_anchors_equal_the_oracle_anchors():
    for shapes in list(ref.TINY_LEVELS.values()) + [KITTI, ref.RANK, ref.LIMIT, ref.UNDER]:
        assert np.array_equal(ref.anchors_f32_restated(shapes), ref.anchors(shapes))


def test_torch_float32_exp_is_within_the_assumed_expf_error():
    """The CPU path of the bound's one assumed constant: float32 exp within EXPF_ULPS ulps of float64 exp."""
    x = np.concatenate([np.linspace(-100, 88.7, 200001), np.random.default_rng(0).normal(0, 3, 100000)]).astype(np.float32)
    got = torch.exp(torch.from_numpy(x)).numpy().astype(np.float64)
    want = np.exp(x.astype(np.float64))
    ok = want > 2.0 ** -126                                     # below: the flush term of the bound
    ulps = np.abs(got - want)[ok] / np.spacing(want[ok].astype(np.float32)).astype(np.float64)
    print("torch float32 exp: %.3f ulps at most (assumed for the device: %.1f)" % (ulps.max(), ptol.EXPF_ULPS))
    assert ulps.max() <= ptol.EXPF_ULPS
    assert (np.abs(got - want)[~ok] <= ptol.TINY).all()


def _all_decodes(c):
    """Every anchor of every image of a case: (float64 Decoded, float32 left, float32 right, image)."""
    anc = ref.anchors(c.shapes)
    A = anc.shape[0]
    for b in range(c.scores.shape[0]):
        o = np.arange(A)
        f32l, f32r = ref.decode_f32(anc, c.deltas[b], c.im_info[b], o, c.scores[b])
        yield ref.decode(anc, c.deltas[b], c.im_info[b], o, c.scores[b]), f32l, f32r, b


DECODE_CASES = ref.RANK_CASES + ref.LIMIT_CASES + ref.BATCH_CASES + ['right:300', 'rich:2048:1', 'poor:2048:2000'] + ref.TINY_CASES


def test_decode_bound_holds_for_the_oracle_float32_path():
    """On every input set of the GPU tests: the float32 decode lies within the derived bound of the float64 one, coordinates
    that are clipped for sure (an infinite width included) are the limit itself, the score column is the gathered score.  The
    bound is worst case; the share of it the float32 path uses is printed and must not be negligible, or the bound would check
    nothing: all six to eight roundings of a coordinate aligned cost at most 16 times their typical sum."""
    worst = 0.0
    for name in DECODE_CASES:
        c = ref.case(name)
        for dec, f32l, f32r, b in _all_decodes(c):
            for d64, bound, raw, f32 in ((dec.left, dec.bound_left, dec.raw_left, f32l), (dec.right, dec.bound_right, dec.raw_right, f32r)):
                err = np.abs(f32[:, :4].astype(np.float64) - d64[:, :4])
                assert np.isfinite(f32).all() and np.isfinite(d64).all()
                assert (err <= bound).all(), (name, b, float((err / bound).max()))
                sure = ref.surely_clipped(raw, bound, c.im_info[b])
                assert np.array_equal(f32[:, :4][sure].astype(np.float64), d64[:, :4][sure]), (name, b)
                assert np.array_equal(f32[:, 4], c.scores[b])
                free = ~sure & (bound > 0) & (d64[:, :4] > 0)
                if free.any():
                    worst = max(worst, float((err[free] / bound[free]).max()))
    print("oracle float32 decode uses at most %.3f of the bound" % worst)
    assert 1.0 / 16 <= worst <= 1.0


@pytest.mark.parametrize("mistake", ref.MISTAKES)
@pytest.mark.parametrize("name", ['batch:mixed', 'batch:five'])
def test_bound_cannot_hide_a_planted_mistake(name, mistake):
    """A float32 restatement with one slip moves at least one coordinate by more than 100 times the bound there."""
    c = ref.case(name)
    anc = ref.anchors(c.shapes)
    o = np.arange(anc.shape[0])
    B = c.scores.shape[0]
    most = 0.0
    for b in range(B):
        dec = ref.decode(anc, c.deltas[b], c.im_info[b], o, c.scores[b])
        bad = ref.decode_f32(ref.anchors_f32_restated(c.shapes, mistake), c.deltas[b], c.im_info[b], o, c.scores[b], mistake=mistake,
                             other_info=c.im_info[(b + 1) % B])
        for d64, bound, got in ((dec.left, dec.bound_left, bad[0]), (dec.right, dec.bound_right, bad[1])):
            err = np.abs(got[:, :4].astype(np.float64) - d64[:, :4])
            most = max(most, float((err / np.maximum(bound, 1e-300)).max()))
    print("%s on %s: %.3g times the bound" % (mistake, name, most))
    assert most > 100.0


# ------------------------------------------------------------------ the generators' properties
def _kth(s, n):
    return np.sort(s)[::-1][n - 1]


@pytest.mark.parametrize("name,b", [('rank:1023:log_uniform', 0), ('limit:8192', 0), ('limit:under', 0), ('batch:mixed', 0), ('batch:five', 0),
                                    ('right:300', 0), ('rich:2048:1', 0), ('rich:8192:1', 0), ('poor:2048:2000', 0), ('richpoor', 1)])
def test_log_uniform_spreads_over_the_first_pass(name, b):
    """At least 200 distinct first-pass digits, and the K-th score's digit in another 32-bin group (another lane of the picking
    wave) than the top score's: the cross-lane prefix and the walk down from the top bin have work to do."""
    c = ref.case(name)
    s = c.scores[b]
    n = ref.n_selected(c.pre, s.shape[0])
    assert 120.0 * n / s.shape[0] >= 16          # the cut at least two 8-exponent groups down, by construction
    dig = ref.first_digit(s)
    assert len(np.unique(dig)) >= 200
    assert int(ref.first_digit(_kth(s, n))) >> 5 != int(dig.max()) >> 5
    assert len(np.unique(dig >> 5)) >= 12


@pytest.mark.parametrize("name,b,value", [('rank:1000:saturated', 0, 1.0), ('rank:2500:saturated', 0, 0.0), ('batch:mixed', 1, 1.0)])
def test_saturated_cut_falls_inside_the_tie_group(name, b, value):
    c = ref.case(name)
    s = c.scores[b]
    A = s.shape[0]
    assert (s == 1.0).sum() == int(0.4 * A) and (s == 0.0).sum() == int(0.4 * A)
    assert ((s > 0) & (s < 2.0 ** -126)).sum() == 3                   # subnormals
    srt = np.sort(s)[::-1]
    assert srt[c.pre - 1] == value and srt[c.pre] == value            # the cut has the same score on both sides
    assert not np.signbit(s).any()


def test_low_bits_leave_the_decision_to_one_pass():
    lo, mid = ref.case('rank:1024:low').scores[0], ref.case('rank:1025:mid').scores[0]
    k = ref.score_key(lo)
    assert len(np.unique(k >> np.uint32(10))) == 1 and len(np.unique(k & np.uint32(0x3FF))) > 900
    k = ref.score_key(mid)
    assert len(np.unique(k >> np.uint32(21))) == 1 and len(np.unique(k & np.uint32(0x3FF))) == 1
    assert len(np.unique((k >> np.uint32(10)) & np.uint32(0x7FF))) > 1500
    assert 0.5 <= min(lo.min(), mid.min()) and max(lo.max(), mid.max()) < 1.0


def test_tie_group_straddles_an_index_digit_with_the_cut_inside():
    c = ref.case('rank:1000:tie')
    s = c.scores[0]
    order = ref.select(c.scores, c.pre)[0]
    t = s[order[-1]]
    tied = np.nonzero(s == t)[0]
    taken = order[s[order] == t]
    assert 0 < len(taken) < len(tied) and np.array_equal(taken, tied[:len(taken)])
    assert tied.min() < 2048 <= tied.max()
    limit = int(taken.max())
    assert limit >= 2048 and (limit & 2047) not in (0, 2047)
    assert (s[order[:-len(taken)]] > t).all()


def _full_keeps(name):
    c = ref.case(name)
    n = ref.n_selected(c.pre, c.scores.shape[1])
    return c, ref.layer(c.scores, c.deltas, c.im_info, c.shapes, c.pre, n, c.thresh)


def test_independent_right_deltas_make_the_keep_lists_differ():
    c, r = _full_keeps('right:300')
    kl, kr = r['keep_left'][0], r['keep_right'][0]
    common = len(np.intersect1d(kl, kr))
    print("right: %d left, %d right, %d common" % (len(kl), len(kr), common))
    assert common < 0.5 * min(len(kl), len(kr))
    assert common < c.post                      # 'right:300': both scans run to the end
    early = ref.case('right:32')                # 'right:32': the stop comes when each eye alone has long kept more than post
    assert np.array_equal(early.scores, c.scores) and np.array_equal(early.deltas, c.deltas) and early.thresh == c.thresh
    row = np.intersect1d(kl, kr)[early.post - 1]
    assert common > early.post and min((kl <= row).sum(), (kr <= row).sum()) > early.post


@pytest.mark.parametrize("pre", [2048, 8192])
def test_survivor_rich_input_has_more_than_2000_common_survivors(pre):
    c, r = _full_keeps('rich:%d:2000' % pre)
    common = np.intersect1d(r['keep_left'][0], r['keep_right'][0])
    print("rich %d: %d common survivors, the 2000th at row %d" % (pre, len(common), common[1999]))
    assert len(common) > 2000
    if pre == 8192:
        assert common[1999] < pre - 64 * 8      # the joint stop leaves whole blocks unscanned


def test_survivor_poor_input_falls_short_of_post():
    c, r = _full_keeps('poor:2048:2000')
    common = len(np.intersect1d(r['keep_left'][0], r['keep_right'][0]))
    print("poor: %d common survivors" % common)
    assert 0 < common < c.post


def test_rich_and_poor_images_of_one_batch_stop_at_different_points():
    c, r = _full_keeps('richpoor')
    common = [np.intersect1d(r['keep_left'][b], r['keep_right'][b]) for b in range(2)]
    assert len(common[0]) > c.post > len(common[1]) > 0
    assert not np.array_equal(c.im_info[0], c.im_info[1])


def test_batches_mix_image_sizes_and_clip_edges():
    """The three im_info rows differ, the small image turns whole boxes into points, +100 gives an infinite float32 width and
    -100 a zero one."""
    c = ref.case('batch:mixed')
    assert len({tuple(r) for r in c.im_info[:, :2].tolist()}) == 3
    anc = ref.anchors(c.shapes)
    r = ref.layer(c.scores, c.deltas, c.im_info, c.shapes, c.pre, c.post)
    d = r['dets_left'][1]
    assert ((d[:, 0] == d[:, 2]) & (d[:, 1] == d[:, 3])).sum() > 100
    assert (anc[:, 3] - anc[:, 1]).max() > c.im_info[1, 0]                   # the image is smaller than a level-0 anchor
    e = c.deltas[2][r['order'][2]]
    with np.errstate(over='ignore'):
        assert np.isinf(np.exp(e[:, [2, 3, 5]].astype(np.float32))).sum() > 50 and (e[:, [2, 3, 5]] == -100).sum() > 50
    z = ref.case('batch:zeros')
    rz = ref.layer(z.scores, z.deltas, z.im_info, z.shapes, z.pre, z.post)
    big = rz['dets_left'][0][:, :4]
    inside = (big > 0).all(1) & (big[:, 2] < 1986) & (big[:, 3] < 599)
    want = anc[rz['order'][0]].astype(np.float64) + np.array([0.0, 0.0, 1.0, 1.0])      # widths carry the + 1 (bbox_transform.py:81-104)
    assert inside.sum() > 100
    assert np.abs(big[inside] - want[inside]).max() < 1e-3


def test_tiny_level_lists_and_their_sizes():
    assert [ref.num_anchors(s) for s in ref.TINY_LEVELS.values()] == [3, 18, 141, 87, 693]
    assert sorted(len(s) for s in ref.TINY_LEVELS.values()) == [1, 1, 2, 4, 5]
    for shapes in ref.TINY_LEVELS.values():
        A = ref.num_anchors(shapes)
        pres = ref.tiny_pre_values(A)
        assert [ref.n_selected(p, A) for p in pres[:3]] == [A, A, A] and all(0 < p < A for p in pres[3:])
    assert ref.num_anchors(ref.UNDER) == 8190 and ref.num_anchors(ref.LIMIT) == 14250 and ref.TK_MAXK == 8192
