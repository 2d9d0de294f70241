"""srcnn_proposal_layer stage by stage against tests/proposal_ref.py, on the small constructed inputs of that file (whose
properties tests/test_proposal_ref_cpu.py asserts): the selection ORDER exactly, the decoded boxes within the derived bound of
tests/proposal_tolerances.py and the score column bit for bit, both keep lists as exact prefixes of the full greedy lists with the
joint stop rule, and the RoIs, the padding and the count bit for bit.  The intermediates come out of the call's workspace
(srcnn_proposal_workspace_layout).

Each stage is fed the device's own output of the stage before, so a deviation belongs to the stage it is found in."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import proposal_ref as ref
import tolerances

pytestmark = pytest.mark.gpu

CANARY = 12345.0                    # no coordinate and no batch index
NUM_CANARY = -77
GUARD_ROWS = 8
_keeps = {}


def _full_keeps(dl, dr, thresh):
    """The reference's full keep lists of a pair of device dets; the same dets (one input at several `post`) are scanned once."""
    k = (hashlib.sha1(dl.tobytes() + dr.tobytes()).hexdigest(), thresh)
    if k not in _keeps:
        _keeps[k] = ref.nms_pair(dl, dr, thresh)
    return _keeps[k]


def _buffers(dev, B, post):
    bufs = [torch.full((B * post + GUARD_ROWS, 5), CANARY, dtype=torch.float32, device=dev) for _ in range(2)]
    nbuf = torch.full((B + GUARD_ROWS,), NUM_CANARY, dtype=torch.int32, device=dev)
    return bufs, nbuf


def _device_inputs(dev, c):
    sc = torch.from_numpy(np.array(c.scores))
    probs = torch.stack((1 - sc, sc), 2).contiguous().to(dev)
    return probs, torch.from_numpy(np.array(c.deltas)).to(dev), torch.from_numpy(np.array(c.im_info)).to(dev)


def _run(dev, c, pre, post, fill=True):
    """One call of the layer on outputs with canary rows behind them and (fill) a workspace prefilled with 0xA5 bytes, as a
    freshly allocated one may be; everything it left behind, on the host."""
    from stereo_rcnn_amd import _lib
    from stereo_rcnn_amd.model.rpn.proposal_layer import _ProposalLayer
    B, A = c.scores.shape
    probs, deltas, info = _device_inputs(dev, c)
    (bl, br), nbuf = _buffers(dev, B, post)
    if fill:
        _lib.workspace(_lib.lib().srcnn_proposal_workspace_bytes(B, A, pre, post), dev, 'proposal').fill_(0xA5)
    layer = _ProposalLayer(16, [0.5, 1, 2])
    out = (bl[:B * post].view(B, post, 5), br[:B * post].view(B, post, 5), nbuf[:B])
    rl, rr = layer.run(probs, deltas, info, c.shapes, pre, post, c.thresh, out=out)
    torch.cuda.synchronize()
    assert rl.data_ptr() == bl.data_ptr() and layer.last_num_valid.data_ptr() == nbuf.data_ptr()
    order, dets, keep, num = ref.read_workspace(B, A, pre, post, dev)
    return {'order': order, 'dets': dets, 'keep': keep, 'num': num, 'rois': (bl.cpu().numpy(), br.cpu().numpy()),
            'num_valid': nbuf.cpu().numpy()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(c, out, pre, post):
    """All four stages of one call; returns what the keep lists looked like, per image."""
    B, A = c.scores.shape
    n = ref.n_selected(pre, A)
    tag = "%s pre %d post %d" % (c.name, pre, post)
    want_order = ref.select(c.scores, n)
    anc = ref.anchors(c.shapes)
    seen = []
    assert out['order'].shape == (B, n)
    for b in range(B):
        # ---- 1. selection: the order itself
        order = out['order'][b]
        bad = np.nonzero(order != want_order[b])[0]
        assert bad.size == 0, "%s image %d: selection differs from row %d on (%d rows): device %s, reference %s" % (
            tag, b, bad[0], bad.size, order[bad[:4]], want_order[b][bad[:4]])
        # ---- 2. decode + clip of the device's order
        dec = ref.decode(anc, c.deltas[b], c.im_info[b], order, c.scores[b])
        for e, (d64, bound, raw) in enumerate(((dec.left, dec.bound_left, dec.raw_left), (dec.right, dec.bound_right, dec.raw_right))):
            got = out['dets'][b, e]
            assert np.array_equal(_bits(got[:, 4]), _bits(c.scores[b][order])), "%s image %d eye %d: score column" % (tag, b, e)
            assert np.isfinite(got).all(), "%s image %d eye %d: a non-finite coordinate" % (tag, b, e)
            err = np.abs(got[:, :4].astype(np.float64) - d64[:, :4])
            sure = ref.surely_clipped(raw, bound, c.im_info[b])
            assert np.array_equal(got[:, :4][sure].astype(np.float64), d64[:, :4][sure]), "%s image %d eye %d: a clipped coordinate" % (tag, b, e)
            tolerances.observe('proposal_stage_decode_px', err.max())
            ratio = float((err[bound > 0] / bound[bound > 0]).max())
            tolerances.observe('proposal_stage_decode_over_bound', ratio)
            assert (err <= bound).all(), "%s image %d eye %d: decode error %.3g of the bound" % (tag, b, e, ratio)
        # ---- 3. both scans: exact prefixes of the full greedy lists, stopped together by the rule
        dl, dr = out['dets'][b, 0], out['dets'][b, 1]
        full = _full_keeps(dl, dr, c.thresh)
        got = []
        for e in range(2):
            m = int(out['num'][b, e])
            assert 1 <= m <= len(full[e]), "%s image %d eye %d: %d kept, the full list has %d" % (tag, b, e, m, len(full[e]))
            k = out['keep'][b, e, :m].astype(np.int64)
            assert np.array_equal(k, full[e][:m]), "%s image %d eye %d: keep list is no prefix of the reference's" % (tag, b, e)
            got.append(k)
        complete = len(got[0]) == len(full[0]) and len(got[1]) == len(full[1])
        common = np.intersect1d(got[0], got[1])
        assert complete or len(common) >= post, "%s image %d: stopped with %d common boxes" % (tag, b, len(common))
        if not complete:       # ... and no later than the 64-row block in which the common count reached post
            first_row_of_last_block = max(got[0][-1], got[1][-1]) // 64 * 64
            assert (common < first_row_of_last_block).sum() < post, "%s image %d: scanned past the stop" % (tag, b)
        # ---- 4. intersection, first post, padding, count
        rl, rr, cnt = ref.intersect_pad(full[0], full[1], dl, dr, b, post)
        for e, want in enumerate((rl, rr)):
            rows = out['rois'][e][b * post:(b + 1) * post]
            assert np.array_equal(_bits(rows), _bits(want)), "%s image %d eye %d: RoI rows" % (tag, b, e)
            assert np.array_equal(rows[cnt:], np.tile(np.array([b, 0, 0, 0, 0], np.float32), (post - cnt, 1)))
        assert int(out['num_valid'][b]) == cnt, (tag, b, int(out['num_valid'][b]), cnt)
        seen.append({'complete': complete, 'kept': (len(got[0]), len(got[1])), 'full': (len(full[0]), len(full[1])), 'count': cnt})
    for e in range(2):
        assert (out['rois'][e][B * post:] == CANARY).all(), "%s: rows behind the RoIs were written" % tag
    assert (out['num_valid'][B:] == NUM_CANARY).all(), "%s: words behind num_valid were written" % tag
    return seen


def _run_and_check(dev, name, pre=None, post=None, fill=True):
    c = ref.case(name)
    pre = c.pre if pre is None else pre
    post = c.post if post is None else post
    return _check(c, _run(dev, c, pre, post, fill), pre, post)


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("name", ref.TINY_CASES)
def test_tiny_levels_every_small_n(dev, name):
    """One to five levels, A from 3 (less than a wave) to 693 (far less than the selection's 65536-thread grid), n == A through
    pre_nms 0 / A / A + 5 and every n around the rank sort's 16- and 64-wide steps; B = 3 mixes three score generators and three
    image sizes."""
    c = ref.case(name)
    A = c.scores.shape[1]
    for pre in ref.tiny_pre_values(A):
        _run_and_check(dev, name, pre, min(ref.n_selected(pre, A), c.post))


@pytest.mark.parametrize("name", ref.RANK_CASES)
def test_n_at_the_rank_sort_edges(dev, name):
    """n = 1000, 1023, 1024, 1025 of A = 3591, each with a score generator that leaves the decision to another part of the radix
    select: a tie group across an index digit, saturated scores cut inside the 1.0 and the 0.0 group, the low and the middle
    key bits alone, 120 exponents."""
    _run_and_check(dev, name)


@pytest.mark.parametrize("name", ref.LIMIT_CASES)
def test_n_at_the_selection_limit(dev, name):
    """pre_nms = 8192 of 14250, and all of 8190 anchors."""
    _run_and_check(dev, name)


def _raw_call(dev, c, pre, post, short_by=0):
    from stereo_rcnn_amd import _lib
    L = _lib.lib()
    B, A = c.scores.shape
    probs, deltas, info = _device_inputs(dev, c)
    (bl, br), nbuf = _buffers(dev, B, post)
    hw = (ctypes.c_int * (2 * len(c.shapes)))(*[int(v) for s in c.shapes for v in s])
    need = L.srcnn_proposal_workspace_bytes(B, A, pre, post)
    ws = _lib.workspace(need, dev, 'proposal')
    rc = L.srcnn_proposal_layer(probs.data_ptr(), deltas.data_ptr(), B, A, hw, len(c.shapes), info.data_ptr(), pre, post, c.thresh,
                                bl.data_ptr(), br.data_ptr(), nbuf.data_ptr(), ws.data_ptr(), need - short_by, _lib.stream())
    torch.cuda.synchronize()
    untouched = bool((bl == CANARY).all()) and bool((br == CANARY).all()) and bool((nbuf == NUM_CANARY).all())
    return rc, untouched


def test_refusals_leave_the_outputs_alone(dev):
    c = ref.case('limit:8192')
    rc, untouched = _raw_call(dev, c, ref.TK_MAXK + 1, 300)
    assert rc != 0 and untouched
    rc, untouched = _raw_call(dev, c, 0, 300)                   # n == A == 14250
    assert rc != 0 and untouched
    rc, untouched = _raw_call(dev, c, ref.TK_MAXK, 300, short_by=1)
    assert rc == -3 and untouched                               # SRCNN_ERR_WORKSPACE
    rc, untouched = _raw_call(dev, c, ref.TK_MAXK, 300)
    assert rc == 0 and not untouched


# ------------------------------------------------------------------ batches, image sizes, clip edges
@pytest.mark.parametrize("name", ref.BATCH_CASES)
def test_batch_of_three_generators_and_three_image_sizes_twice_on_one_workspace(dev, name):
    """Image 0 log-uniform scores / N(0, 0.3) deltas on 600 x 1987, image 1 saturated scores / N(0, 3) on 37 x 53 (whole boxes
    clip to a point), image 2 low-bit scores / +-100 widths on 375 x 1242; all-zero deltas (the anchors come out); five
    levels.  The second run finds the workspace as the first left it: histograms and arrival counters are back at zero."""
    first = _run_and_check(dev, name)
    second = _run_and_check(dev, name, fill=False)
    assert first == second


@pytest.mark.parametrize("name", ref.RIGHT_CASES)
def test_left_and_right_keep_lists_that_differ(dev, name):
    seen = _run_and_check(dev, name)[0]
    if name == 'right:300':
        assert seen['complete'] and seen['count'] < 0.5 * min(seen['full'])
    else:
        assert not seen['complete'] and seen['count'] == 32 and min(seen['kept']) > 32


# ------------------------------------------------------------------ joint stop, training-sized post_nms
@pytest.mark.parametrize("name", ref.STOP_CASES)
def test_joint_stop_and_rows_beyond_1024(dev, name):
    """Survivor-rich: more than 2000 common survivors, so every post in {1, 64, 1024, 1025, 2000} fills all its rows and the scan
    stops early (except where post nearly exhausts pre = 2048).  Survivor-poor: the intersection falls short of post, both scans
    run to the end, the padding starts at the count.  richpoor: both in one launch, two stop points."""
    seen = _run_and_check(dev, name)
    c = ref.case(name)
    if name.startswith('rich:'):
        assert seen[0]['count'] == c.post
        if c.pre == 8192:
            assert not seen[0]['complete'] and max(seen[0]['kept']) < c.post + 256
    elif name.startswith('poor:'):
        assert seen[0]['complete'] and 0 < seen[0]['count'] < c.post
    else:
        assert seen[0]['count'] == c.post and seen[1]['complete'] and 0 < seen[1]['count'] < c.post
