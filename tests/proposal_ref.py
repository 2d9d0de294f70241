"""The proposal layer (csrc/rpn_proposal.hip + the paired scan of csrc/nms.hip) stage by stage on the CPU, the reader of the
device's own intermediates, and the constructed inputs the stage tests run on (TEST INFRASTRUCTURE ONLY).

Every stage function takes the stage before it as ARGUMENTS, so tests/test_proposal_stages_gpu.py can feed it what the device
actually produced and a deviation belongs to the stage it is found in:

    select          stable descending sort, first n            (proposal_layer.py:96,111-115)   exact
    anchors         oracle.proposal.anchors_all_levels         (generate_anchors.py:112-173)    float32, as the kernel casts them
    decode          float64 decode + clip of float32 inputs    (bbox_transform.py:81-104,177-185) with its bound, see
                    tests/proposal_tolerances.py
    decode_f32      the same in float32, operation for operation the oracle's; with planted mistakes on request
    nms_pair        oracle.ops.nms per eye, FULL keep lists    (test_nms_bit_exact holds the kernel bit-equal to it)
    intersect_pad   sorted intersection, first `post`, zero padding (proposal_layer.py:127-143)  exact

tests/test_proposal_ref_cpu.py pins all of it against oracle.proposal.proposal_layer and asserts of every input generator the
property it exists for.
"""
import collections
import zlib

import numpy as np
import torch

from oracle import ops as oops
from oracle import proposal as oprop
import proposal_tolerances as ptol

SCALES = (32.0, 64.0, 128.0, 256.0, 512.0)
STRIDES = (4.0, 8.0, 16.0, 32.0, 64.0)
RATIOS = (0.5, 1.0, 2.0)
TK_MAXK = 8192                      # csrc/rpn_proposal.hip: the most candidates the selection keeps


def num_anchors(shapes):
    return sum(3 * int(h) * int(w) for h, w in shapes)


def n_selected(pre, A):
    """proposal_layer.py:111: everything is kept for pre <= 0 or pre >= A."""
    return pre if 0 < pre < A else A


# ------------------------------------------------------------------ stages
def select(scores, n):
    """(B, A) float32 scores -> (B, n) int64: torch.sort(descending, stable)[:n] per image."""
    s = torch.from_numpy(np.array(scores, np.float32))
    return torch.sort(s, dim=1, descending=True, stable=True)[1][:, :n].numpy().astype(np.int64)


def anchors(feat_shapes):
    return oprop.anchors_all_levels([list(map(int, s)) for s in feat_shapes]).astype(np.float32)


Decoded = collections.namedtuple('Decoded', 'left right bound_left bound_right raw_left raw_right')


def decode(anchors_f32, deltas_f32, im_info, order, scores):
    """One image.  anchors (A, 4) float32, deltas (A, 6) float32, im_info (3,), order (n,) anchor indices, scores (A,) float32
    -> Decoded: left / right (n, 5) float64 dets computed in float64 from the float32 inputs, clipped, the gathered score in
    column 4; bound_* (n, 4) the error bound of a float32 evaluation per coordinate (tests/proposal_tolerances.py); raw_* (n, 4)
    the coordinates before the clip.  Left uses (d0, d1, d2, d3), right (d4, d1, d5, d3)."""
    assert anchors_f32.dtype == np.float32 and deltas_f32.dtype == np.float32
    order = np.asarray(order, np.int64)
    a = anchors_f32[order].astype(np.float64)
    d = deltas_f32[order].astype(np.float64)
    wmax, hmax = ptol.clip_limit(im_info[1]), ptol.clip_limit(im_info[0])
    sc = np.asarray(scores, np.float32)[order].astype(np.float64)
    out = []
    for cols in ((0, 1, 2, 3), (4, 1, 5, 3)):
        x1, x2, ex1, ex2 = ptol.axis(a[:, 0], a[:, 2], d[:, cols[0]], d[:, cols[2]])
        y1, y2, ey1, ey2 = ptol.axis(a[:, 1], a[:, 3], d[:, cols[1]], d[:, cols[3]])
        raw = np.stack([x1, y1, x2, y2], 1)
        lim = np.array([wmax, hmax, wmax, hmax])
        dets = np.concatenate([np.minimum(np.maximum(raw, 0.0), lim), sc[:, None]], 1)
        out.append((dets, np.stack([ex1, ey1, ex2, ey2], 1), raw))
    return Decoded(out[0][0], out[1][0], out[0][1], out[1][1], out[0][2], out[1][2])


def surely_clipped(raw, bound, im_info):
    """(n, 4) bool: coordinates whose float64 value lies beyond a clip limit by more than the bound (an infinite width
    included) -- a float32 evaluation must return the limit itself there."""
    lim = np.array([im_info[1], im_info[0], im_info[1], im_info[0]], np.float64) - 1.0
    return (raw < -bound) | (raw > lim + bound)


MISTAKES = ('right_eye_uses_dx', 'no_plus_one', 'ratio_shifted', 'neighbour_stride', 'other_image_info')


def anchors_f32_restated(feat_shapes, mistake=None):
    """The kernel's analytic anchors (gather_decode_kernel) restated: float64 centre and half size per (level, ratio), cast to
    float32.  mistake 'ratio_shifted': ratio index a + 1; 'neighbour_stride': the stride of the next level (of the one before
    for the last)."""
    rows = []
    for l, (h, w) in enumerate(feat_shapes):
        stride = STRIDES[l]
        if mistake == 'neighbour_stride':
            stride = STRIDES[l + 1 if l + 1 < len(STRIDES) else l - 1]
        ys, xs, aa = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing='ij')
        if mistake == 'ratio_shifted':
            aa = (aa + 1) % 3
        r = np.asarray(RATIOS)[aa]
        aw, ah = SCALES[l] * np.sqrt(r), SCALES[l] / np.sqrt(r)
        cx, cy = xs * stride, ys * stride
        rows.append(np.stack([cx - 0.5 * aw, cy - 0.5 * ah, cx + 0.5 * aw, cy + 0.5 * ah], -1).reshape(-1, 4))
    return np.concatenate(rows, 0).astype(np.float32)


def decode_f32(anchors_f32, deltas_f32, im_info, order, scores, mistake=None, other_info=None):
    """decode in float32, operation for operation oracle.proposal.decode_boxes + clip_boxes (torch float32 on the CPU), so
    that without a mistake it equals the oracle bit for bit.  Returns left, right (n, 5) float32."""
    order = np.asarray(order, np.int64)
    a = torch.from_numpy(anchors_f32[order])
    d = torch.from_numpy(deltas_f32[order])
    info = other_info if mistake == 'other_image_info' else im_info
    wmax, hmax = float(info[1]) - 1, float(info[0]) - 1
    one = 0.0 if mistake == 'no_plus_one' else 1.0
    sc = torch.from_numpy(np.asarray(scores, np.float32)[order])
    out = []
    for eye, cols in enumerate(((0, 1, 2, 3), (4, 1, 5, 3))):
        if eye == 1 and mistake == 'right_eye_uses_dx':
            cols = (0, 1, 5, 3)
        widths = a[:, 2] - a[:, 0] + one
        heights = a[:, 3] - a[:, 1] + one
        ctr_x = a[:, 0] + 0.5 * widths
        ctr_y = a[:, 1] + 0.5 * heights
        pcx = d[:, cols[0]] * widths + ctr_x
        pcy = d[:, cols[1]] * heights + ctr_y
        pw = torch.exp(d[:, cols[2]]) * widths
        ph = torch.exp(d[:, cols[3]]) * heights
        box = torch.stack([(pcx - 0.5 * pw).clamp(0, wmax), (pcy - 0.5 * ph).clamp(0, hmax),
                           (pcx + 0.5 * pw).clamp(0, wmax), (pcy + 0.5 * ph).clamp(0, hmax), sc], 1)
        out.append(box.numpy())
    return out[0], out[1]


def nms_pair(dets_l, dets_r, thresh):
    """FULL greedy keep lists (ascending rows, int64) of the two eyes, from oracle.ops.nms on float32 dets -- the device's own
    dets when a GPU test calls it."""
    assert dets_l.dtype == np.float32 and dets_r.dtype == np.float32
    return oops.nms(dets_l, thresh).astype(np.int64), oops.nms(dets_r, thresh).astype(np.int64)


def intersect_pad(keep_l, keep_r, dets_l, dets_r, b, post):
    """-> rois_left, rois_right (post, 5) float32 [b, x1, y1, x2, y2] with zero padding rows [b, 0, 0, 0, 0], and the count."""
    keep = np.intersect1d(keep_l, keep_r)[:post]
    out = []
    for dets in (dets_l, dets_r):
        r = np.zeros((post, 5), np.float32)
        r[:, 0] = b
        r[:len(keep), 1:] = np.asarray(dets, np.float32)[keep, :4]
        out.append(r)
    return out[0], out[1], len(keep)


def layer(scores, deltas, im_info, shapes, pre, post, thresh=0.7):
    """The five stages chained on the CPU with the float32 decode: a dict of per-image lists like oracle.proposal_layer's
    `extra`, plus the RoIs.  (What test_proposal_ref_cpu.py holds equal to the oracle.)"""
    B, A = scores.shape
    order = select(scores, n_selected(pre, A))
    anc = anchors(shapes)
    res = {'order': order, 'dets_left': [], 'dets_right': [], 'keep_left': [], 'keep_right': [], 'count': [],
           'rois_left': np.zeros((B, post, 5), np.float32), 'rois_right': np.zeros((B, post, 5), np.float32)}
    for b in range(B):
        dl, dr = decode_f32(anc, deltas[b], im_info[b], order[b], scores[b])
        kl, kr = nms_pair(dl, dr, thresh)
        res['rois_left'][b], res['rois_right'][b], c = intersect_pad(kl, kr, dl, dr, b, post)
        for k, v in (('dets_left', dl), ('dets_right', dr), ('keep_left', kl), ('keep_right', kr), ('count', c)):
            res[k].append(v)
    return res


# ------------------------------------------------------------------ the device's intermediates
def read_workspace(B, A, pre, post, device):
    """order (B, n) int64, dets (B, 2, n, 5) float32, keep (B, 2, n) int32, num (B, 2) int32 of the last srcnn_proposal_layer
    call with these sizes on the current stream, read out of the 'proposal' workspace (include/srcnn_hip.h:
    srcnn_proposal_workspace_layout).  Synchronise before calling."""
    import ctypes
    from stereo_rcnn_amd import _lib
    L = _lib.lib()
    n = n_selected(pre, A)
    off = (ctypes.c_size_t * 5)()
    _lib.check(L.srcnn_proposal_workspace_layout(B, A, pre, off, 5), 'srcnn_proposal_workspace_layout')
    ws = _lib.workspace(L.srcnn_proposal_workspace_bytes(B, A, pre, post), device, 'proposal')
    lo, hi = int(off[0]), int(off[3]) + B * 2 * 4
    raw = ws[lo:hi].cpu().numpy()               # the scratch of the NMS mask behind `num` stays on the device
    o = [int(v) - lo for v in off]
    order = raw[o[0]:o[0] + B * n * 4].view(np.int32).reshape(B, n).astype(np.int64)
    dets = raw[o[1]:o[1] + B * 2 * n * 5 * 4].view(np.float32).reshape(B, 2, n, 5).copy()
    keep = raw[o[2]:o[2] + B * 2 * n * 4].view(np.int32).reshape(B, 2, n).copy()
    num = raw[o[3]:o[3] + B * 2 * 4].view(np.int32).reshape(B, 2).copy()
    return order, dets, keep, num


# ------------------------------------------------------------------ scores: all in [0, 1]
def score_key(s):
    """The selection's order-preserving key of a non-negative float32 (csrc/rpn_proposal.hip: score_key)."""
    return np.asarray(s, np.float32).view(np.uint32) | np.uint32(0x80000000)


def first_digit(s):
    return score_key(s) >> np.uint32(21)


def log_uniform(rng, A):
    """2 ** -U(0, 120): a hundred and twenty exponents, as a trained RPN's scores span -- many bins of the first radix pass,
    over most lanes of the picking wave."""
    return (2.0 ** -rng.uniform(0.0, 120.0, A)).astype(np.float32)


def saturated(rng, A):
    """40 % exactly 1.0f, 40 % exactly 0.0f (a saturated softmax), the rest log-uniform with a few subnormals."""
    s = log_uniform(rng, A)
    k = A - 2 * int(0.4 * A)
    s[:min(3, k)] = np.array([2.0 ** -130, 2.0 ** -140, 2.0 ** -149], np.float32)[:min(3, k)]
    s[k:k + int(0.4 * A)] = 1.0
    s[k + int(0.4 * A):] = 0.0
    return s[rng.permutation(A)]


def low_bits(rng, A, which='low'):
    """One exponent (0.5 <= s < 1) and equal high mantissa bits.  'low': only the low 10 bits differ, the third radix pass
    decides alone; 'mid': only bits 10..20 differ, the second pass decides."""
    base = np.uint32(0x3F000000) | np.uint32(0x2 << 21)
    if which == 'low':
        u = base | np.uint32(0x5A5 << 10) | rng.integers(0, 1024, A).astype(np.uint32)
    else:
        u = base | (rng.integers(0, 2048, A).astype(np.uint32) << np.uint32(10)) | np.uint32(0x155)
    return u.view(np.float32)


def tie_across_index_digits(rng, A, n, lo=1500, hi=2600, taken=800):
    """n - taken distinct scores above one tie group at the indices [lo, hi), which straddle 2048; everything else below.  The cut
    takes `taken` of the ties: the largest tie index selected is lo + taken - 1 >= 2048, so both index passes pick a digit."""
    assert A > hi and n > taken and hi - lo > taken and n - taken <= A - (hi - lo)
    s = (0.2 * rng.random(A)).astype(np.float32)
    outside = np.concatenate([np.arange(lo), np.arange(hi, A)])
    top = rng.choice(outside, n - taken, replace=False)
    s[top] = (0.5 + 0.5 * rng.permutation(n - taken) / (n - taken)).astype(np.float32)
    s[lo:hi] = 0.25
    return s


def uniform(rng, A):
    return rng.random(A).astype(np.float32)


# ------------------------------------------------------------------ deltas
def normal_deltas(rng, A, sigma):
    return (rng.standard_normal((A, 6)) * sigma).astype(np.float32)


def edge_deltas(rng, A):
    """N(0, 0.3) with every fifth row's widths at +100 (expf overflows to inf; the clip brings it back) and every seventh row's
    at -100 (zero size), left and right eye and the height in turn."""
    d = normal_deltas(rng, A, 0.3)
    for k, cols in enumerate(([2], [3], [5], [2, 3, 5])):
        d[k * 5::20, cols] = 100.0
        d[k * 7 + 1::28, cols] = -100.0
    return d


def independent_right(rng, A, sigma=0.03):
    """d4 / d5 independent of d0 / d2 and ten times as wide: the right boxes of a neighbourhood sit elsewhere than the left ones
    and suppress each other differently."""
    d = normal_deltas(rng, A, sigma)
    d[:, 4:] = normal_deltas(rng, A, 10 * sigma)[:, 4:]
    return d


def survivor_rich(rng, A):
    """dw = dh = -3 and centres moved by at most 5 % of the anchor: boxes narrower than the level-0 stride, hardly any pair
    overlaps by 0.7, nearly every candidate survives both scans."""
    d = np.full((A, 6), -3.0, np.float32)
    d[:, [0, 1, 4]] = rng.uniform(-0.05, 0.05, (A, 3)).astype(np.float32)
    return d


# ------------------------------------------------------------------ cases
INFO = {'kitti': (600.0, 1987.0, 1.6), 'tiny': (37.0, 53.0, 0.1), 'raw': (375.0, 1242.0, 1.0)}
INFO3 = np.array([INFO['kitti'], INFO['tiny'], INFO['raw']], np.float32)

TINY_LEVELS = {'a3': [[1, 1]], 'a18': [[2, 3]], 'two': [[5, 7], [3, 4]], 'four': [[4, 5], [2, 3], [1, 2], [1, 1]],
               'five': [[10, 16], [6, 8], [3, 5], [2, 3], [1, 2]]}
RANK = [[19, 63]]                   # A = 3591
LIMIT = [[38, 125]]                 # A = 14250
UNDER = [[21, 130]]                 # A = 8190: n == A just under TK_MAXK


def tiny_pre_values(A):
    return [0, A, A + 5] + [p for p in (1, 2, 15, 16, 17, 63, 64, 65) if p < A]


Case = collections.namedtuple('Case', 'name shapes scores deltas im_info pre post thresh')
_cases = {}


def _seed(name):
    return zlib.crc32(name.encode())


def _mixed3(rng, A):
    return np.stack([log_uniform(rng, A), saturated(rng, A), low_bits(rng, A, 'low' if A > 100 else 'mid')])


def _build(name):
    rng = np.random.default_rng(_seed(name))
    kind, _, arg = name.partition(':')
    one = np.array([INFO['kitti']], np.float32)
    if kind == 'tiny':                                      # tiny:<levels>:<B>  (pre / post are set per call by the test)
        lv, B = arg.split(':')
        shapes, B = TINY_LEVELS[lv], int(B)
        A = num_anchors(shapes)
        sc = _mixed3(rng, A)[:B] if B == 3 else log_uniform(rng, A)[None]
        de = np.stack([normal_deltas(rng, A, 0.3) for _ in range(B)])
        return Case(name, shapes, sc, de, INFO3[:B] if B == 3 else one, 0, max(1, min(A, 40)), 0.7)
    if kind == 'rank':                                      # rank:<n>:<generator>
        n, gen = arg.split(':')
        n, A = int(n), num_anchors(RANK)
        sc = {'log_uniform': lambda: log_uniform(rng, A), 'saturated': lambda: saturated(rng, A),
              'low': lambda: low_bits(rng, A, 'low'), 'mid': lambda: low_bits(rng, A, 'mid'),
              'tie': lambda: tie_across_index_digits(rng, A, n)}[gen]()
        return Case(name, RANK, sc[None], normal_deltas(rng, A, 0.3)[None], one, n, 300, 0.7)
    if kind == 'limit':                                     # limit:8192 | limit:under
        shapes, pre = (LIMIT, TK_MAXK) if arg == '8192' else (UNDER, 0)
        A = num_anchors(shapes)
        return Case(name, shapes, log_uniform(rng, A)[None], normal_deltas(rng, A, 0.3)[None], one, pre, 300, 0.7)
    if kind == 'batch':                                     # batch:<deltas>: B = 3, three score generators, three image sizes
        shapes, pre = (TINY_LEVELS['five'], 0) if arg == 'five' else (RANK, 1000)     # five levels (A = 693): everything kept
        A = num_anchors(shapes)
        sc = _mixed3(rng, A)
        if arg == 'zeros':                                  # the anchors themselves come out
            de = np.zeros((3, A, 6), np.float32)
        else:
            de = np.stack([normal_deltas(rng, A, 0.3), normal_deltas(rng, A, 3.0), edge_deltas(rng, A)])
        return Case(name, shapes, sc, de, INFO3, pre, 300, 0.7)
    if kind == 'right':                                     # right:<post>: left and right keep lists that differ strongly (every
        A = num_anchors(RANK)                               # anchor of a dense level, threshold 0.4: both eyes keep a small part)
        rng = np.random.default_rng(_seed(kind))
        return Case(name, RANK, log_uniform(rng, A)[None], independent_right(rng, A)[None], one, 0, int(arg), 0.4)
    if kind in ('rich', 'poor'):                            # rich:<pre>:<post> | poor:<pre>:<post>
        pre, post = [int(v) for v in arg.split(':')]
        A = num_anchors(LIMIT)
        rng = np.random.default_rng(_seed(kind))            # one input per kind, whatever pre / post
        sc = log_uniform(rng, A)[None]
        de = (survivor_rich(rng, A) if kind == 'rich' else normal_deltas(rng, A, 0.3))[None]
        return Case(name, LIMIT, sc, de, one, pre, post, 0.7)
    if kind == 'richpoor':                                  # B = 2: image 0 survivor-rich, image 1 survivor-poor
        r, p = case('rich:2048:1800'), case('poor:2048:1800')
        return Case(name, LIMIT, np.concatenate([r.scores, p.scores]), np.concatenate([r.deltas, p.deltas]),
                    np.array([INFO['kitti'], INFO['raw']], np.float32), 2048, 1800, 0.7)
    raise KeyError(name)


def case(name):
    """A named input set, built once and read-only."""
    if name not in _cases:
        c = _build(name)
        for a in (c.scores, c.deltas, c.im_info):
            assert a.dtype == np.float32
            a.setflags(write=False)
        assert c.scores.min() >= 0.0 and c.scores.max() <= 1.0 and np.isfinite(c.deltas).all()
        _cases[name] = c
    return _cases[name]


RANK_CASES = ['rank:1000:tie', 'rank:1000:saturated', 'rank:1023:log_uniform', 'rank:1024:low', 'rank:1025:mid',
              'rank:2500:saturated']
LIMIT_CASES = ['limit:8192', 'limit:under']
BATCH_CASES = ['batch:mixed', 'batch:zeros', 'batch:five']
RICH_CASES = ['rich:%d:%d' % (pre, post) for pre in (2048, 8192) for post in (1, 64, 1024, 1025, 2000)]
STOP_CASES = RICH_CASES + ['poor:2048:2000', 'richpoor']
TINY_CASES = ['tiny:%s:%d' % (lv, B) for lv in TINY_LEVELS for B in (1, 3)]
RIGHT_CASES = ['right:300', 'right:32']
FIXED_CASES = RANK_CASES + LIMIT_CASES + BATCH_CASES + RIGHT_CASES + STOP_CASES
