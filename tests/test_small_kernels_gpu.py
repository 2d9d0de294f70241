"""The small kernels around the conv engines, each called directly through the C ABI and compared with a plain reference of the same
operation (tests/small_kernels_ref.py, pinned on the CPU by tests/test_small_kernels_ref_cpu.py): head tails, detection decode,
per-class / batched NMS, max-pool, upsample-add, subsample, layout transposes, SPLIT16 conversion and the RPN score.

Copies, index outputs, max-pool, subsample, transposes and the SPLIT16 split are held bit for bit.  Softmax-type outputs and
upsample-add are held to bounds DERIVED from the float32 evaluation model (small_kernels_ref.softmax_bound / upsample_add_bound);
the observed maxima are reported as a fraction of those bounds through tolerances.observe (1.0 = at the bound)."""
import ctypes

import numpy as np
import pytest
import torch

import small_kernels_ref as R
import tolerances as tol_
from oracle import ops as oops
from test_ops_gpu import _rand_dets

pytestmark = pytest.mark.gpu

CANARY = -7.0
ERR_WORKSPACE = -3          # SRCNN_ERR_WORKSPACE (include/srcnn_hip.h)
TAG_MAXPOOL = 9003          # range-guard flag of srcnn_maxpool3x3s2_ceil (include/srcnn_hip.h)
TAG_CONVERT = 9002


def _L():
    from stereo_rcnn_amd import _lib
    return _lib, _lib.lib()


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _canary(shape, dev, dtype=torch.float32, value=CANARY):
    return torch.full(shape, value, dtype=dtype, device=dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _within(name, got, ref, bound):
    """|got - ref| <= bound elementwise; reports max(|got - ref| / bound) under `name` before asserting."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    frac = tol_.observe(name, float((err / bound).max()))
    assert np.isfinite(np.asarray(got)).all() and frac <= 1.0, (name, frac, float(err.max()))


# ================================================================================================ 1. softmax tails
def _logits(rng, rows, cols):
    """Ordinary logits; from the LAST row backwards (the rows next to a block edge), where rows allow: a row shifted by +1e4
    and its unshifted twin (multiples of 1/64, so the shift is exact in float32), one dominating logit, logits spread over
    +-80, equal logits."""
    x = rng.normal(0, 3, (rows, cols)).astype(np.float32)
    twin = None
    if rows >= 2:
        x[rows - 2] = np.round(x[rows - 2] * 64) / 64
        x[rows - 1] = x[rows - 2] + np.float32(1e4)
        assert np.array_equal(x[rows - 1].astype(np.float64) - 1e4, x[rows - 2].astype(np.float64))
        twin = (rows - 1, rows - 2)
    if rows >= 3:
        x[rows - 3] = -200.0
        x[rows - 3, cols // 2] = 30.0
    if rows >= 4:
        x[rows - 4] = np.linspace(-80, 80, cols) if cols > 1 else 80.0
    if rows >= 5:
        x[rows - 5] = 1.25
    return x, twin


def _check_softmax(name, got, logits, twin):
    ref, bound = R.softmax_rows(logits), R.softmax_bound(logits)
    _within(name, got, ref, bound)
    assert (np.abs(got.astype(np.float64).sum(1) - 1.0) <= bound.sum(1)).all()
    if twin is not None:       # the shifted row: the same probabilities as the unshifted one, within the bound
        assert (np.abs(got[twin[0]].astype(np.float64) - ref[twin[1]]) <= bound[twin[1]]).all()


@pytest.mark.parametrize("rows", [1, 127, 128, 129, 257])
def test_softmax_rows_vs_float64(dev, rows):
    """srcnn_softmax_rows (256 threads per block: 257 rows take two) over cols in {1, 2, 4, 7}, row stride > cols with a canary
    in the gap that would dominate any softmax it entered."""
    _lib, L = _L()
    for cols in (1, 2, 4, 7):
        rng = np.random.default_rng(rows * 10 + cols)
        x, twin = _logits(rng, rows, cols)
        xs = cols + 3
        buf = np.full((rows, xs), 777.0, np.float32)
        buf[:, :cols] = x
        xd = _d(buf, dev)
        y = _canary((rows + 2, cols), dev)
        _lib.check(L.srcnn_softmax_rows(xd.data_ptr(), rows, cols, xs, y.data_ptr(), _lib.stream()))
        got = y.cpu().numpy()
        assert (got[rows:] == CANARY).all() and np.array_equal(xd.cpu().numpy(), buf)
        _check_softmax('small.softmax_rows / bound', got[:rows], x, twin)


@pytest.mark.parametrize("rows", [1, 127, 128, 129, 257])
def test_box_head_tail_vs_float64(dev, rows):
    """srcnn_box_head_tail (128 threads per block) on rows [bbox 6 n_cls | dim_orien 5 n_cls | logits n_cls | gap]: the two
    regressions are bit-equal copies, the class probabilities the float64 softmax of the float32 logits."""
    _lib, L = _L()
    for n_cls in (1, 2, 4, 7):
        rng = np.random.default_rng(rows * 10 + n_cls + 5)
        nb, nd = 6 * n_cls, 5 * n_cls
        x, twin = _logits(rng, rows, n_cls)
        xs = nb + nd + n_cls + 5
        buf = np.full((rows, xs), 777.0, np.float32)
        buf[:, :nb + nd] = rng.normal(0, 1, (rows, nb + nd))
        buf[:, nb + nd:nb + nd + n_cls] = x
        fc = _d(buf, dev)
        bb, dm, cl = _canary((rows + 2, nb), dev), _canary((rows + 2, nd), dev), _canary((rows + 2, n_cls), dev)
        _lib.check(L.srcnn_box_head_tail(fc.data_ptr(), rows, nb, nd, n_cls, xs, bb.data_ptr(), dm.data_ptr(), cl.data_ptr(), _lib.stream()))
        bb, dm, cl = bb.cpu().numpy(), dm.cpu().numpy(), cl.cpu().numpy()
        assert np.array_equal(_bits(bb[:rows]), _bits(buf[:, :nb])) and np.array_equal(_bits(dm[:rows]), _bits(buf[:, nb:nb + nd]))
        assert (bb[rows:] == CANARY).all() and (dm[rows:] == CANARY).all() and (cl[rows:] == CANARY).all()
        assert np.array_equal(fc.cpu().numpy(), buf)
        _check_softmax('small.box_head_tail cls / bound', cl[:rows], x, twin)


# ================================================================================================ 2. keypoint tail
@pytest.mark.parametrize("G", [1, 2, 7, 28, 32])
def test_kpts_tail_vs_float64(dev, G):
    """srcnn_kpts_tail: sum over h, then softmaxes over the 4 G bins of channels 0-3 (output order (channel, w)), the G bins of
    channel 4 and those of channel 5.  The column sums of channel c sit 10 c apart, so a group that takes in a wrong channel, or
    normalises with another group's maximum, moves probabilities by orders of magnitude.  Logits are multiples of 2^-10 below
    64: their float32 sums over h <= 32 rows are exact in any order, so the bound is the pure softmax bound of the summed
    columns.  roi_limit: rows at or past it keep their canary."""
    _lib, L = _L()
    for n in (1, 3):
        rng = np.random.default_rng(G * 10 + n)
        lg = rng.integers(-2048, 2049, (n, G, G, 6)) / 1024.0 + np.round(10.0 * np.arange(6) / G * 1024) / 1024
        lg = lg.astype(np.float32)
        k_ref, l_ref, r_ref, col = R.kpts_tail(lg)
        assert np.array_equal(col, col.astype(np.float32).astype(np.float64))
        x = _d(lg, dev)
        for limit in (None, 0, 1, n, n + 5):
            kp, lp, rp = _canary((n + 1, 4 * G), dev), _canary((n + 1, G), dev), _canary((n + 1, G), dev)
            lim = None if limit is None else torch.tensor([limit], dtype=torch.int32, device=dev)
            _lib.check(L.srcnn_kpts_tail(x.data_ptr(), n, G, kp.data_ptr(), lp.data_ptr(), rp.data_ptr(),
                                         None if lim is None else lim.data_ptr(), _lib.stream()))
            kp, lp, rp = kp.cpu().numpy(), lp.cpu().numpy(), rp.cpu().numpy()
            live = n if limit is None else min(limit, n)
            assert (kp[live:] == CANARY).all() and (lp[live:] == CANARY).all() and (rp[live:] == CANARY).all()
            if live == 0:
                continue
            groups = ((kp, k_ref, col[:, :4].reshape(n, 4 * G), 'kpts'), (lp, l_ref, col[:, 4], 'left'), (rp, r_ref, col[:, 5], 'right'))
            for got, ref, c, nm in groups:
                bound = R.softmax_bound(c[:live])
                _within('small.kpts_tail %s / bound' % nm, got[:live], ref[:live], bound)
                assert (np.abs(got[:live].astype(np.float64).sum(1) - 1.0) <= bound.sum(1)).all()
        assert np.array_equal(x.cpu().numpy(), lg)


# ================================================================================================ 3. decode
def _decode_case(rng, n, n_cls, G, scale):
    H, W = 192.0, 640.0
    x1 = rng.uniform(0, W - 60, n); y1 = rng.uniform(0, H - 40, n)
    rl = np.stack([np.zeros(n), x1, y1, x1 + rng.uniform(0, 200, n), y1 + rng.uniform(0, 80, n)], 1).astype(np.float32)
    bp = rng.normal(0, 1, (n, 6 * n_cls)).astype(np.float32)
    dp = rng.normal(0, 1, (n, 5 * n_cls)).astype(np.float32)
    kp = rng.uniform(0, 0.5, (n, 4 * G)).astype(np.float32)
    lp = rng.uniform(0, 0.5, (n, G)).astype(np.float32)
    rp = rng.uniform(0, 0.5, (n, G)).astype(np.float32)
    if n >= 16:
        rl[0, 1:] = [-90, 10, -20, 60]                       # wholly left of the image
        rl[1, 1:] = [30, -70, 90, -5]                        # wholly above
        bp[2, 0::6], bp[3, 0::6] = -60.0, 60.0               # dx: past the left / right border
        bp[4, 1::6], bp[5, 1::6] = -60.0, 60.0               # dy: past the top / bottom border
        bp[6, 4::6], bp[7, 4::6] = -60.0, 60.0               # the right eye's dx
        bp[8, 2::6], bp[8, 5::6] = 500.0, 500.0              # dw = 100: expf overflows, the clipped box is [0, wmax]
        bp[9, 3::6] = 500.0                                  # dh likewise
        rl[10, 3] = rl[10, 1]                                # zero-width roi (x2 == x1)
        kp[11, [G + 2, 3 * G + 1]] = 0.75; lp[11, [2, G - 1]] = 0.75; rp[11, [1, G - 2]] = 0.75            # two equal maxima
        kp[12, [3, 2 * G, 4 * G - 1]] = 0.875; lp[12, [0, 3, 4]] = 0.875; rp[12, [4, 5, 6]] = 0.875        # three
        kp[13], lp[13], rp[13] = 0, 0, 0                     # the lazy-keypoint path's all-zero row
    rr = rl.copy()
    rr[:, [1, 3]] -= rng.uniform(0, 30, (n, 1)).astype(np.float32)
    return rl, rr, bp, dp, kp, lp, rp, np.array([H, W, scale], np.float32)


def _decode_gpu(dev, case, n, n_cls, G):
    _lib, L = _L()
    t = [_d(a, dev) for a in case]
    bl, br, dm, kk = (_canary((n + 1, 4 * n_cls), dev), _canary((n + 1, 4 * n_cls), dev), _canary((n + 1, 5 * n_cls), dev),
                      _canary((n + 1, 5), dev))
    _lib.check(L.srcnn_decode_detections(*[v.data_ptr() for v in t], n, n_cls, G, bl.data_ptr(), br.data_ptr(), dm.data_ptr(),
                                         kk.data_ptr(), _lib.stream()))
    out = {'boxes_left': bl.cpu().numpy(), 'boxes_right': br.cpu().numpy(), 'dim_orien': dm.cpu().numpy(), 'kpts': kk.cpu().numpy()}
    for v in out.values():
        assert (v[n:] == CANARY).all()
    return {k: v[:n] for k, v in out.items()}, t


@pytest.mark.parametrize("n", [1, 128, 129])
@pytest.mark.parametrize("G", [7, 28])
def test_decode_detections_vs_oracle(dev, n, G):
    """srcnn_decode_detections against oracle.postprocess.decode_detections: boxes and dimensions at tolerances.DECODED_PX; the
    keypoint row is exact -- column 1 (type = index / G), column 2 (the maximum, a copy) and the columns decoded from the argmax
    indices (the same four float32 operations as the oracle's, so a wrong index is the only way to differ).  Clipping edges,
    expf overflow and argmax ties included (_decode_case)."""
    for n_cls in (1, 2, 4):
        for scale in (1.0, 1.6):
            case = _decode_case(np.random.default_rng(n + G + n_cls), n, n_cls, G, scale)
            ref = R.decode_detections(*case, n_cls=n_cls, G=G)
            got, _ = _decode_gpu(dev, case, n, n_cls, G)
            for k in ('boxes_left', 'boxes_right', 'dim_orien'):
                assert np.isfinite(got[k]).all()
                assert tol_.observe('small.decode %s' % k, np.abs(got[k].astype(np.float64) - ref[k]).max()) < tol_.DECODED_PX, k
            assert np.array_equal(_bits(got['kpts']), _bits(ref['kpts']))
            if n >= 16:
                wmax = np.float32(639.0) / np.float32(scale)
                assert (got['boxes_left'][8, 0::4] == 0).all() and (got['boxes_left'][8, 2::4] == wmax).all()
                assert (got['boxes_right'][8, 0::4] == 0).all() and (got['boxes_right'][8, 2::4] == wmax).all()
                assert (got['boxes_left'][0, 0::4] == 0).all() and (got['boxes_left'][1, 1::4] == 0).all()
                kd = np.round(got['kpts'][11:14, 1].astype(np.float64) * G).astype(int)
                assert kd.tolist() == [G + 2, 3, 0] and got['kpts'][11:14, 2].tolist() == [0.75, 0.875, 0.0]


@pytest.mark.parametrize("n,G", [(1, 7), (129, 28), (128, 7)])
def test_decode_kept_kpts_and_gather_rows(dev, n, G):
    """srcnn_decode_kept_kpts: probabilities in KEPT order, results in the roi's own row, bit-equal to the full decode's row (and so
    to the oracle's); rows not kept, -1 entries and entries at or past num leave `kpts` alone.  srcnn_gather_rows: -1 reads row 0."""
    _lib, L = _L()
    rng = np.random.default_rng(n)
    case = _decode_case(rng, n, 2, G, 1.6)
    full, t = _decode_gpu(dev, case, n, 2, G)
    ref = R.decode_detections(*case, n_cls=2, G=G)['kpts']
    for num in sorted({0, 1, n}):
        keep = np.full(n, -1, np.int32)
        keep[:num] = rng.permutation(n)[:num]                 # out of order
        if num > 8:
            keep[[3, 7]] = -1                                 # holes inside the list
        kd = _d(keep, dev)
        numd = torch.tensor([num], dtype=torch.int32, device=dev)
        g = [torch.empty_like(t[4]), torch.empty_like(t[5]), torch.empty_like(t[6])]
        for src, dst in zip(t[4:7], g):
            cols = int(src.shape[1])
            _lib.check(L.srcnn_gather_rows(src.data_ptr(), kd.data_ptr(), n, cols, dst.data_ptr(), _lib.stream()))
            assert torch.equal(dst.cpu(), src.cpu()[torch.from_numpy(np.maximum(keep, 0)).long()])
        out = _canary((n, 5), dev)
        _lib.check(L.srcnn_decode_kept_kpts(t[0].data_ptr(), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), kd.data_ptr(),
                                            numd.data_ptr(), t[7].data_ptr(), n, G, out.data_ptr(), _lib.stream()))
        out = out.cpu().numpy()
        kept = keep[:num][keep[:num] >= 0]
        rest = np.setdiff1d(np.arange(n), kept)
        assert np.array_equal(_bits(out[kept]), _bits(full['kpts'][kept])) and np.array_equal(_bits(out[kept]), _bits(ref[kept]))
        assert (out[rest] == CANARY).all()


def test_gather_rows_across_a_block(dev):
    """n_idx * cols = 37 * 7 = 259 elements: the second 256-thread block holds three."""
    _lib, L = _L()
    rng = np.random.default_rng(3)
    src = rng.normal(0, 1, (50, 7)).astype(np.float32)
    idx = rng.integers(0, 50, 37).astype(np.int32)
    idx[[0, 20, 36]] = -1
    dst = _canary((38, 7), dev)
    srcd, idxd = _d(src, dev), _d(idx, dev)                   # both alive across the call: a freed temporary's block may be handed out again
    _lib.check(L.srcnn_gather_rows(srcd.data_ptr(), idxd.data_ptr(), 37, 7, dst.data_ptr(), _lib.stream()))
    dst = dst.cpu().numpy()
    assert np.array_equal(_bits(dst[:37]), _bits(src[np.maximum(idx, 0)])) and (dst[37] == CANARY).all()


@pytest.mark.parametrize("n,n_cls", [(1, 2), (129, 2), (129, 4)])
def test_pack_detections_record(dev, n, n_cls):
    """srcnn_pack_detections: row 0 = [count, range flag, 0 ...], one row per kept roi with the roi index in column 19, zero rows
    past the count, nothing past row n; the library's range-flag word travels in rec[0, 1] and reads back as 0 afterwards."""
    _lib, L = _L()
    rng = np.random.default_rng(n + n_cls)
    sc = rng.uniform(0, 1, (n, n_cls)).astype(np.float32)
    bl, br = rng.uniform(0, 600, (n, 4 * n_cls)).astype(np.float32), rng.uniform(0, 600, (n, 4 * n_cls)).astype(np.float32)
    do, kp = rng.normal(0, 1, (n, 5 * n_cls)).astype(np.float32), rng.normal(0, 1, (n, 5)).astype(np.float32)
    dv = [_d(a, dev) for a in (sc, bl, br, do, kp)]
    hot = _d(np.full((1, 8), 7e4, np.float32), dev)
    sink = torch.empty_like(hot)
    for num in sorted({0, 1, n}):
        keep = np.full(n, -1, np.int32)
        keep[:num] = rng.permutation(n)[:num]
        kd, numd = _d(keep, dev), torch.tensor([num], dtype=torch.int32, device=dev)
        for j in sorted({1, n_cls - 1}):
            for cols in (20, 24):
                for flagged in (False, True):
                    L.srcnn_range_flag_read(1)
                    if flagged:       # an out-of-range conversion leaves its tag in the flag word
                        _lib.check(L.srcnn_act_convert(hot.data_ptr(), 0, sink.data_ptr(), 1, 1, 8, _lib.stream()))
                        assert L.srcnn_range_flag_read(0) == TAG_CONVERT
                    rec = _canary((n + 2, cols), dev)
                    _lib.check(L.srcnn_pack_detections(*[v.data_ptr() for v in dv], kd.data_ptr(), numd.data_ptr(), n, n_cls, j, cols,
                                                       rec.data_ptr(), _lib.stream()))
                    assert L.srcnn_range_flag_read(0) == 0
                    rec = rec.cpu().numpy()
                    want = R.pack_detections(sc, bl, br, do, kp, keep, num, j, cols, flag=float(TAG_CONVERT) if flagged else 0.0)
                    assert np.array_equal(_bits(rec[:n + 1]), _bits(want)) and (rec[n + 1] == CANARY).all()


# ================================================================================================ 4. class NMS, batched NMS
THRESH = 0.05


def _score_patterns(rng, n):
    one = np.full(n, 0.01, np.float32); one[n // 3] = 0.6
    at = rng.uniform(0, 1, n).astype(np.float32); at[::3] = np.float32(THRESH)
    return {'below': np.full(n, 0.01, np.float32), 'above': rng.uniform(0.1, 1, n).astype(np.float32), 'one': one, 'at_threshold': at,
            'quantised': np.round(rng.uniform(0, 1, n), 2).astype(np.float32), 'equal': np.full(n, 0.5, np.float32)}


@pytest.mark.parametrize("n", [1, 2, 300, 1023, 1024, 1025, 2048])
def test_class_nms_vs_oracle(dev, n):
    """srcnn_class_nms against: score > thresh (strict), stable descending sort (ties by ascending roi index), oracle.ops.nms on
    the class's left boxes, mapped back.  keep_idx, its -1 tail and num are exact.  n crosses the one / two candidates per thread
    edge of the bitonic select (1024) up to the documented maximum (2048); the other classes hold high scores and huge boxes."""
    _lib, L = _L()
    need = L.srcnn_class_nms_workspace_bytes(n)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    for n_cls, j in ((2, 1), (4, 1), (4, 3)):
        rng = np.random.default_rng(n * 10 + n_cls + j)
        boxes = rng.uniform(0, 1, (n, 4 * n_cls)).astype(np.float32) * np.float32(1500.0)
        boxes[:, 0::4], boxes[:, 1::4] = 0.0, 0.0                                  # huge boxes over everything
        boxes[:, 4 * j:4 * j + 4] = _rand_dets(rng, n)[:, :4]
        bd = _d(boxes, dev)
        for name, s in _score_patterns(rng, n).items():
            scores = rng.uniform(0.5, 1, (n, n_cls)).astype(np.float32)
            scores[:, j] = s
            keep, num = _canary((n + 1,), dev, torch.int32, -5), _canary((2,), dev, torch.int32, -5)
            _lib.check(L.srcnn_class_nms(_d(scores, dev).data_ptr(), n, n_cls, j, bd.data_ptr(), THRESH, 0.3, keep.data_ptr(),
                                         num.data_ptr(), ws.data_ptr(), need, _lib.stream()))
            want_keep, want_num = R.class_nms(scores, boxes, j, THRESH, 0.3)
            keep, num = keep.cpu().numpy(), num.cpu().numpy()
            assert num.tolist() == [want_num, -5], (name, n_cls, j)
            assert np.array_equal(keep[:n], want_keep) and keep[n] == -5, (name, n_cls, j)
            if name == 'below':
                assert want_num == 0
            if name == 'one':
                assert want_num == 1 and keep[0] == n // 3
            if name == 'at_threshold':
                assert not (np.isin(np.arange(0, n, 3), keep[:want_num])).any()


def test_class_nms_refusals(dev):
    """More than 2048 rois: an error, nothing launched.  A workspace one byte short: SRCNN_ERR_WORKSPACE."""
    _lib, L = _L()
    n = 2049
    sc, bx = torch.rand(n, 2, device=dev), torch.rand(n, 8, device=dev)
    keep, num = _canary((n,), dev, torch.int32, -5), _canary((1,), dev, torch.int32, -5)
    need = L.srcnn_class_nms_workspace_bytes(n)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    assert L.srcnn_class_nms(sc.data_ptr(), n, 2, 1, bx.data_ptr(), THRESH, 0.3, keep.data_ptr(), num.data_ptr(), ws.data_ptr(), need,
                             _lib.stream()) < 0
    torch.cuda.synchronize()
    assert bool((keep == -5).all()) and int(num[0]) == -5 and int(ws.max()) == 0
    n = 300
    need = L.srcnn_class_nms_workspace_bytes(n)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    assert L.srcnn_class_nms(sc.data_ptr(), n, 2, 1, bx.data_ptr(), THRESH, 0.3, keep.data_ptr(), num.data_ptr(), ws.data_ptr(), need - 1,
                             _lib.stream()) == ERR_WORKSPACE
    assert L.srcnn_class_nms(sc.data_ptr(), n, 2, 1, bx.data_ptr(), THRESH, 0.3, keep.data_ptr(), num.data_ptr(), None, need,
                             _lib.stream()) == ERR_WORKSPACE


@pytest.mark.parametrize("n_valid", [[0, 1, 200], [200, 37, 64]])
def test_nms_batched_with_differing_valid_counts(dev, n_valid):
    """srcnn_nms_batched, three problems of 200 boxes: each keep list and count equal oracle.ops.nms on the problem's valid
    prefix; the entries past n_valid are image-sized boxes with the highest scores, which would suppress everything if read."""
    _lib, L = _L()
    nb, n = 3, 200
    rng = np.random.default_rng(sum(n_valid))
    dets = np.stack([_rand_dets(rng, n) for _ in range(nb)])
    for b, nv in enumerate(n_valid):
        dets[b, nv:] = [0.0, 0.0, 1986.0, 599.0, 2.0]
    keep, num = _canary((nb, n), dev, torch.int32, -5), _canary((nb + 1,), dev, torch.int32, -5)
    need = L.srcnn_nms_batched_workspace_bytes(nb, n)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    detsd, nvd = _d(dets, dev), _d(np.array(n_valid, np.int32), dev)      # both alive across the call (see test_gather_rows_across_a_block)
    _lib.check(L.srcnn_nms_batched(keep.data_ptr(), detsd.data_ptr(), num.data_ptr(), nvd.data_ptr(),
                                   nb, n, 5, 0.7, ws.data_ptr(), need, _lib.stream()))
    keep, num = keep.cpu().numpy(), num.cpu().numpy()
    assert num[nb] == -5
    for b, nv in enumerate(n_valid):
        want = oops.nms(dets[b, :nv], 0.7)
        assert num[b] == len(want) and np.array_equal(keep[b, :len(want)], want), b
    assert L.srcnn_nms_batched(_canary((nb, n), dev, torch.int32).data_ptr(), _d(dets, dev).data_ptr(), _canary((nb,), dev, torch.int32).data_ptr(),
                               None, nb, n, 5, 0.7, ws.data_ptr(), need - 256, _lib.stream()) == ERR_WORKSPACE


# ================================================================================================ 5. max-pool
def _pool_inputs(rng, B, H, W, C):
    yield 'negative', (-np.abs(rng.normal(0, 1, (B, H, W, C))) - 0.5).astype(np.float32)      # a 0-initialised maximum shows
    yield 'mixed', rng.normal(0, 100, (B, H, W, C)).astype(np.float32)
    OH, OW = R.ceil_pool_out(H), R.ceil_pool_out(W)
    for pos in range(9):                     # the maximum of every window at each of its nine positions in turn
        x = (-np.abs(rng.normal(0, 1, (B, H, W, C))) - 1.0).astype(np.float32)
        dh, dw = divmod(pos, 3)
        for oh in range(OH):
            for ow in range(OW):
                h, w = min(2 * oh + dh, H - 1), min(2 * ow + dw, W - 1)
                x[:, h, w, :] = 3.0 + oh * OW + ow + 0.125 * pos
        yield 'peak%d' % pos, x


@pytest.mark.parametrize("H,W", [(3, 3), (4, 4), (5, 5), (4, 7), (7, 4), (6, 9)])
def test_maxpool_bit_exact_both_formats(dev, H, W):
    """srcnn_maxpool3x3s2_ceil: F32 output bit-equal to F.max_pool2d(3, 2, 0, ceil_mode=True), SPLIT16 output bit-equal to the
    split of it; no partial window, 1- and 2-wide partial windows in H, in W and in both."""
    import torch.nn.functional as F
    _lib, L = _L()
    OH, OW = R.ceil_pool_out(H), R.ceil_pool_out(W)
    for B in (1, 2):
        for C in (8, 24):
            rng = np.random.default_rng(H * 100 + W * 10 + B + C)
            for name, x in _pool_inputs(rng, B, H, W, C):
                want = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 3, 2, 0, ceil_mode=True).permute(0, 2, 3, 1).contiguous().numpy()
                assert want.shape == (B, OH, OW, C) and np.array_equal(want, R.maxpool3x3s2_ceil(x))
                xd = _d(x, dev)
                for fmt in (0, 1):
                    y = _canary((B * OH * OW + 1, C), dev)
                    _lib.check(L.srcnn_maxpool3x3s2_ceil(xd.data_ptr(), B, H, W, C, y.data_ptr(), OH, OW, fmt, _lib.stream()))
                    y = y.cpu().numpy()
                    expect = want.reshape(-1, C) if fmt == 0 else R.split16_pack(want.reshape(-1, C))
                    assert np.array_equal(_bits(y[:-1]), _bits(expect)), (name, B, C, fmt)
                    assert (y[-1] == CANARY).all()


def test_maxpool_refusals(dev):
    _lib, L = _L()
    x, y = torch.zeros(1, 4, 7, 24, device=dev), _canary((64, 24), dev)
    assert L.srcnn_maxpool3x3s2_ceil(x.data_ptr(), 1, 4, 7, 24, y.data_ptr(), 3, 3, 0, _lib.stream()) < 0      # OH: row 4 of 4
    assert L.srcnn_maxpool3x3s2_ceil(x.data_ptr(), 1, 4, 7, 24, y.data_ptr(), 2, 5, 0, _lib.stream()) < 0      # OW: column 8 of 7
    assert L.srcnn_maxpool3x3s2_ceil(x.data_ptr(), 1, 4, 7, 12, y.data_ptr(), 2, 3, 0, _lib.stream()) < 0      # C = 12
    torch.cuda.synchronize()
    assert bool((y == CANARY).all())


def test_maxpool_split16_output_raises_the_range_flag(dev):
    """A pooled value beyond +-65504 cannot be held by SPLIT16 (hi = inf, lo = -inf, read back as NaN): the max-pool must raise
    the library's range flag like every other kernel that writes the format, under its own tag."""
    _lib, L = _L()
    rng = np.random.default_rng(1)
    x = rng.normal(0, 1, (1, 5, 5, 24)).astype(np.float32)
    x[0, 2, 2, 8:16] = 65504.0
    y = torch.empty(4, 24, device=dev)
    L.srcnn_range_flag_read(1)
    _lib.check(L.srcnn_maxpool3x3s2_ceil(_d(x, dev).data_ptr(), 1, 5, 5, 24, y.data_ptr(), 2, 2, 1, _lib.stream()))
    assert L.srcnn_range_flag_read(1) == 0                     # the largest value the format holds: no flag
    x[0, 2, 2, 11] = 7e4
    _lib.check(L.srcnn_maxpool3x3s2_ceil(_d(x, dev).data_ptr(), 1, 5, 5, 24, y.data_ptr(), 2, 2, 0, _lib.stream()))
    assert L.srcnn_range_flag_read(1) == 0                     # F32 output is not subject to the format's range
    _lib.check(L.srcnn_maxpool3x3s2_ceil(_d(x, dev).data_ptr(), 1, 5, 5, 24, y.data_ptr(), 2, 2, 1, _lib.stream()))
    flag = L.srcnn_range_flag_read(0)
    assert flag != 0, "7e4 stored as SPLIT16 (reads back as NaN) without raising the range flag"
    assert flag == TAG_MAXPOOL
    from stereo_rcnn_amd import engine
    assert 'maxpool' in engine.range_flag(reset=True)[1] and L.srcnn_range_flag_read(0) == 0


# ================================================================================================ 6. upsample-add
@pytest.mark.parametrize("TH,TW,H,W", [(1, 1, 3, 5), (1, 4, 2, 7), (3, 1, 5, 1), (3, 4, 3, 4), (3, 4, 5, 7), (7, 5, 19, 11), (2, 2, 1, 1)])
def test_upsample_add_vs_float64(dev, TH, TW, H, W):
    """srcnn_upsample_add against the float64 bilinear (float32 source index and fraction, as ATen and the kernel compute them) plus
    the lateral, within upsample_add_bound; a SPLIT16 top is read as hi + lo, a SPLIT16 result is allowed one step of the split on
    top.  Same size in and out: bit-equal to top + lateral (and to its split)."""
    _lib, L = _L()
    for B in (1, 3):
        for C in (8, 24):
            rng = np.random.default_rng(TH * 1000 + H * 10 + B + C)
            top = (rng.normal(0, 30, (B, TH, TW, C))).astype(np.float32)
            lat = (rng.normal(0, 30, (B, H, W, C))).astype(np.float32)
            top_raw = R.split16_pack(top)
            top_q = R.split16_unpack(top_raw)
            ld = _d(lat, dev)
            for tf, yf in ((0, 0), (1, 1), (0, 1), (1, 0)):
                src = top_q if tf else top
                ref, mag = R.upsample_add(src, lat)
                y = _canary((B * H * W + 1, C), dev)
                L.srcnn_range_flag_read(1)
                _lib.check(L.srcnn_upsample_add(_d(top_raw if tf else top, dev).data_ptr(), TH, TW, ld.data_ptr(), B, H, W, C, y.data_ptr(),
                                                tf, yf, _lib.stream()))
                assert L.srcnn_range_flag_read(1) == 0
                y = y.cpu().numpy()
                assert (y[-1] == CANARY).all()
                got = (R.split16_unpack(y[:-1]) if yf else y[:-1]).reshape(B, H, W, C)
                bound = R.upsample_add_bound(mag) + (R.split16_step(ref) if yf else 0.0)
                _within('small.upsample_add%s / bound' % ('.split16' if yf else ''), got, ref, bound)
                if (TH, TW) == (H, W):
                    exact = (src + lat).reshape(-1, C)
                    assert np.array_equal(_bits(y[:-1]), _bits(R.split16_pack(exact) if yf else exact))


@pytest.mark.parametrize("TH,TW,H,W", [(1, 1, 3, 5), (1, 4, 2, 7), (3, 1, 5, 1), (3, 4, 3, 4), (3, 4, 5, 7), (7, 5, 19, 11), (2, 2, 1, 1)])
def test_upsample_add_equals_the_float32_restatement(dev, TH, TW, H, W):
    """Bit for bit (the library is built with -ffp-contract=off) against small_kernels_ref.upsample_add_f32, the restatement of
    csrc/bilinear_tap.h, in all four format pairs: a SPLIT16 top enters as float32(hi) + float32(lo), a SPLIT16 result is the
    split of the restated float32.  The shapes reach every branch of the tap: a one-pixel source (r = 0), a one-pixel output, the
    clamped last row and column (i1p = 0), the identity size."""
    _lib, L = _L()
    for B in (1, 3):
        for C in (8, 24):
            rng = np.random.default_rng(TH * 1000 + H * 10 + B + C)
            top = (rng.normal(0, 30, (B, TH, TW, C))).astype(np.float32)
            lat = (rng.normal(0, 30, (B, H, W, C))).astype(np.float32)
            top_raw = R.split16_pack(top)
            top_q = R.split16_unpack(top_raw)
            ld = _d(lat, dev)
            for tf, yf in ((0, 0), (1, 1), (0, 1), (1, 0)):
                want = R.upsample_add_f32(top_q if tf else top, lat).reshape(-1, C)
                y = _canary((B * H * W + 1, C), dev)
                _lib.check(L.srcnn_upsample_add(_d(top_raw if tf else top, dev).data_ptr(), TH, TW, ld.data_ptr(), B, H, W, C, y.data_ptr(),
                                                tf, yf, _lib.stream()))
                y = y.cpu().numpy()
                assert (y[-1] == CANARY).all()
                expect = R.split16_pack(want) if yf else want
                differ = int((_bits(y[:-1]) != _bits(expect)).sum())
                print("upsample_add %s B=%d C=%d fmt %d->%d: %d of %d words differ from the float32 restatement"
                      % ((TH, TW, H, W), B, C, tf, yf, differ, expect.size))
                assert differ == 0, (B, C, tf, yf)


# ================================================================================================ 7. subsample, transposes
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 5), (4, 6)])
def test_subsample2_bit_exact(dev, H, W):
    _lib, L = _L()
    for C in (4, 12):
        x = np.random.default_rng(H + C).normal(0, 1, (2, H, W, C)).astype(np.float32)
        want = R.subsample2(x)
        OH, OW = want.shape[1:3]
        assert (OH, OW) == ((H + 1) // 2, (W + 1) // 2)
        y = _canary((2 * OH * OW + 1, C), dev)
        _lib.check(L.srcnn_subsample2(_d(x, dev).data_ptr(), 2, H, W, C, y.data_ptr(), OH, OW, _lib.stream()))
        y = y.cpu().numpy()
        assert np.array_equal(_bits(y[:-1]), _bits(want.reshape(-1, C))) and (y[-1] == CANARY).all()


@pytest.mark.parametrize("C", [1, 31, 32, 33, 65])
def test_layout_transposes_bit_exact(dev, C):
    """srcnn_nchw_to_nhwc / srcnn_nhwc_to_nchw on (C, H W) with each side below, at, and above one and two 32 x 32 tiles."""
    _lib, L = _L()
    B = 3
    for hw in (1, 31, 32, 33, 65):
        x = np.random.default_rng(C * 100 + hw).normal(0, 1, (B, C, hw, 1)).astype(np.float32)
        y = _canary((B * C * hw + 7,), dev)
        _lib.check(L.srcnn_nchw_to_nhwc(_d(x, dev).data_ptr(), B, C, hw, 1, y.data_ptr(), _lib.stream()))
        y = y.cpu().numpy()
        want = R.nchw_to_nhwc(x)
        assert np.array_equal(_bits(y[:-7]), _bits(want.reshape(-1))) and (y[-7:] == CANARY).all()
        z = _canary((B * C * hw + 7,), dev)
        _lib.check(L.srcnn_nhwc_to_nchw(_d(want, dev).data_ptr(), B, hw, 1, C, z.data_ptr(), _lib.stream()))
        z = z.cpu().numpy()
        assert np.array_equal(_bits(z[:-7]), _bits(x.reshape(-1))) and (z[-7:] == CANARY).all()
        assert np.array_equal(R.nhwc_to_nchw(want), x)


# ================================================================================================ 8. SPLIT16 conversion
def _convert_values(rng, pixels, C):
    x = (rng.normal(0, 1, (pixels, C)) * 10.0 ** rng.integers(-7, 4, (pixels, C))).astype(np.float32)
    mid = np.float32(1.0 + 2.0 ** -11)                      # midpoint between the float16 neighbours 1 and 1 + 2^-10
    special = [0.0, -0.0, 6e-8, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 6.1e-5, 6.09e-5, -5.5e-6, 1e-8, -1e-8,
               mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(2)), 1.0 + 3 * 2.0 ** -11,
               2049.0, 2051.0, 65504.0, -65504.0, np.nextafter(np.float32(65520.0), np.float32(0)), 65503.99, 1000.123]
    flat = x.reshape(-1)
    flat[:len(special)] = special
    flat[-len(special):] = special
    return x


@pytest.mark.parametrize("C", [8, 24])
def test_act_convert_is_the_numpy_float16_split(dev, C):
    """srcnn_act_convert F32 -> SPLIT16: hi = float16(x), lo = float16(x - float32(hi)), round-to-nearest-even, laid out per
    8-channel group as 8 hi then 8 lo at the byte offset the 8 floats had -- bit for bit against numpy; and back:
    float32(hi) + float32(lo).  300 pixels: more than one 256-thread block of groups."""
    _lib, L = _L()
    pixels = 300
    x = _convert_values(np.random.default_rng(C), pixels, C)
    want = R.split16_pack(x)
    y = _canary((pixels + 1, C), dev)
    _lib.check(L.srcnn_act_convert(_d(x, dev).data_ptr(), 0, y.data_ptr(), 1, pixels, C, _lib.stream()))
    L.srcnn_range_flag_read(1)          # (the largest float32 that still rounds to 65504 is beyond the guard's 65504: conservative)
    yh = y.cpu().numpy()
    assert np.array_equal(_bits(yh[:-1]), _bits(want)) and (yh[-1] == CANARY).all()
    z = _canary((pixels + 1, C), dev)
    _lib.check(L.srcnn_act_convert(y.data_ptr(), 1, z.data_ptr(), 0, pixels, C, _lib.stream()))
    z = z.cpu().numpy()
    assert np.array_equal(_bits(z[:-1]), _bits(R.split16_unpack(want))) and (z[-1] == CANARY).all()
    assert (np.abs(z[:-1].astype(np.float64) - x) <= R.split16_step(x)).all()


def test_act_convert_range_flag(dev):
    """65504 converts silently; 65520 (rounds to inf) and a NaN raise the flag of the input conversion."""
    _lib, L = _L()
    sink = torch.empty(2, 8, device=dev)
    for value, raised in ((65504.0, False), (-65504.0, False), (65520.0, True), (-65520.0, True), (float('nan'), True)):
        x = np.ones((2, 8), np.float32)
        x[1, 5] = value
        L.srcnn_range_flag_read(1)
        _lib.check(L.srcnn_act_convert(_d(x, dev).data_ptr(), 0, sink.data_ptr(), 1, 2, 8, _lib.stream()))
        assert L.srcnn_range_flag_read(1) == (TAG_CONVERT if raised else 0), value
    assert L.srcnn_range_flag_read(0) == 0


# ================================================================================================ 9. RPN score
LEVEL_HW = [1, 2 * 3, 5 * 7]


def _rpn_check(name, probs, deltas, head, b_rows):
    """probs / deltas rows `b_rows` of one level against the float64 pair softmax and the copied deltas of `head` (B, hw, 24)."""
    p_ref, d_ref, bound = R.rpn_score(head)
    _within(name, probs[:, b_rows], p_ref, bound)
    assert np.array_equal(_bits(deltas[:, b_rows]), _bits(d_ref))


@pytest.mark.parametrize("B", [1, 2])
def test_rpn_score_per_level_vs_float64(dev, B):
    """srcnn_rpn_score per level into a shared (B, a_total) output at level offsets with canary anchors between and behind the
    levels: the pair softmax (background c with foreground c + 3, flattened in consecutive pairs) against float64, the deltas
    copied bit for bit."""
    _lib, L = _L()
    rng = np.random.default_rng(B)
    heads = [(rng.normal(0, 4, (B, hw, 24))).astype(np.float32) for hw in LEVEL_HW]
    offs, a = [], 0
    for hw in LEVEL_HW:
        offs.append(a)
        a += 3 * hw + 2                                            # two canary anchors behind every level
    pr, dl = _canary((B, a, 2), dev), _canary((B, a, 6), dev)
    for hd, hw, off in zip(heads, LEVEL_HW, offs):
        _lib.check(L.srcnn_rpn_score(_d(hd, dev).data_ptr(), B, hw, 24, pr.data_ptr(), dl.data_ptr(), off, a, _lib.stream()))
    pr, dl = pr.cpu().numpy(), dl.cpu().numpy()
    for hd, hw, off in zip(heads, LEVEL_HW, offs):
        _rpn_check('small.rpn_score / bound', pr, dl, hd, slice(off, off + 3 * hw))
        assert (pr[:, off + 3 * hw:off + 3 * hw + 2] == CANARY).all() and (dl[:, off + 3 * hw:off + 3 * hw + 2] == CANARY).all()


@pytest.mark.parametrize("B", [1, 2])
def test_rpn_score_levels_and_parts_vs_float64(dev, B):
    """The two fused forms against the same float64 reference: srcnn_rpn_score_levels (all levels in one launch) and
    srcnn_rpn_score_parts (per level 1, 2 and 3 partial planes with padding between them, added in plane order, then the bias --
    restated in float32 on the CPU, operation for operation, to obtain the logits the softmax sees)."""
    _lib, L = _L()
    rng = np.random.default_rng(B + 10)
    nl = len(LEVEL_HW)
    A = 3 * sum(LEVEL_HW)
    heads = [(rng.normal(0, 4, (B, hw, 24))).astype(np.float32) for hw in LEVEL_HW]
    hd = [_d(h, dev) for h in heads]
    pr, dl = _canary((B + 1, A, 2), dev), _canary((B + 1, A, 6), dev)
    ptrs = (ctypes.c_void_p * nl)(*[t.data_ptr() for t in hd])
    hws = (ctypes.c_int * nl)(*LEVEL_HW)
    _lib.check(L.srcnn_rpn_score_levels(ptrs, hws, nl, B, 24, pr.data_ptr(), dl.data_ptr(), A, _lib.stream()))
    pr, dl = pr.cpu().numpy(), dl.cpu().numpy()
    assert (pr[B] == CANARY).all() and (dl[B] == CANARY).all()
    off = 0
    for h, hw in zip(heads, LEVEL_HW):
        _rpn_check('small.rpn_score_levels / bound', pr[:B], dl[:B], h, slice(off, off + 3 * hw))
        off += 3 * hw
    # partial planes
    bias = rng.normal(0, 1, 24).astype(np.float32)
    nparts = [1, 2, 3]
    planes, sums = [], []
    for hw, k in zip(LEVEL_HW, nparts):
        plane = B * hw * 24 + 8                                    # padding behind every plane: the plane stride is what counts
        buf = np.full((k, plane), 1e6, np.float32)
        part = (rng.normal(0, 3, (k, B * hw * 24))).astype(np.float32)
        buf[:, :B * hw * 24] = part
        s = part[0].copy()
        for q in range(1, k):
            s = s + part[q]
        sums.append((s.reshape(B, hw, 24) + bias).astype(np.float32))
        planes.append((_d(buf, dev), plane))
    pr, dl = _canary((B + 1, A, 2), dev), _canary((B + 1, A, 6), dev)
    pp = (ctypes.c_void_p * nl)(*[t.data_ptr() for t, _ in planes])
    npp = (ctypes.c_int * nl)(*nparts)
    pl = (ctypes.c_longlong * nl)(*[p for _, p in planes])
    _lib.check(L.srcnn_rpn_score_parts(pp, npp, pl, hws, nl, B, _d(bias, dev).data_ptr(), pr.data_ptr(), dl.data_ptr(), A, _lib.stream()))
    pr, dl = pr.cpu().numpy(), dl.cpu().numpy()
    assert (pr[B] == CANARY).all() and (dl[B] == CANARY).all()
    off = 0
    for h, hw in zip(sums, LEVEL_HW):
        _rpn_check('small.rpn_score_parts / bound', pr[:B], dl[:B], h, slice(off, off + 3 * hw))
        off += 3 * hw


def test_rpn_score_forms_write_identical_bits(dev):
    """The three RPN score entry points run one body (csrc/rpn_score.h): srcnn_rpn_score per level, srcnn_rpn_score_levels, and
    srcnn_rpn_score_parts with one plane per level and an all-zero bias write the same bits to probs and deltas; so does _parts
    with a second, all-zero plane behind padding.  (x + 0.0f == x bit for bit unless x is -0.0, which normal deviates are not.)
    Levels of 6, 2 and 1 locations: the last is a single location at the end of the level search."""
    _lib, L = _L()
    B, level_hw = 2, [6, 2, 1]
    nl, A = len(level_hw), 3 * sum(level_hw)
    assert A == 27
    rng = np.random.default_rng(77)
    heads = [rng.normal(0, 4, (B, hw, 24)).astype(np.float32) for hw in level_hw]
    assert not any(np.signbit(h[h == 0]).any() for h in heads)
    hd = [_d(h, dev) for h in heads]
    hws = (ctypes.c_int * nl)(*level_hw)
    new = lambda: (_canary((B + 1, A, 2), dev), _canary((B + 1, A, 6), dev))
    got = {}
    pr, dl = new()
    off = 0
    for t, hw in zip(hd, level_hw):
        _lib.check(L.srcnn_rpn_score(t.data_ptr(), B, hw, 24, pr.data_ptr(), dl.data_ptr(), off, A, _lib.stream()))
        off += 3 * hw
    got['per level'] = (pr.cpu().numpy(), dl.cpu().numpy())
    pr, dl = new()
    ptrs = (ctypes.c_void_p * nl)(*[t.data_ptr() for t in hd])
    _lib.check(L.srcnn_rpn_score_levels(ptrs, hws, nl, B, 24, pr.data_ptr(), dl.data_ptr(), A, _lib.stream()))
    got['levels'] = (pr.cpu().numpy(), dl.cpu().numpy())
    bias = torch.zeros(24, dtype=torch.float32, device=dev)
    for planes in (1, 2):
        bufs, sizes = [], []
        for h, hw in zip(heads, level_hw):
            plane = B * hw * 24 + (8 if planes == 2 else 0)              # padding between the planes
            buf = np.full((planes, plane), 1e6, np.float32)
            buf[0, :B * hw * 24] = h.ravel()
            if planes == 2:
                buf[1, :B * hw * 24] = 0.0
            bufs.append(_d(buf, dev))
            sizes.append(plane)
        pr, dl = new()
        pp = (ctypes.c_void_p * nl)(*[t.data_ptr() for t in bufs])
        npp = (ctypes.c_int * nl)(*([planes] * nl))
        pl = (ctypes.c_longlong * nl)(*sizes)
        _lib.check(L.srcnn_rpn_score_parts(pp, npp, pl, hws, nl, B, bias.data_ptr(), pr.data_ptr(), dl.data_ptr(), A, _lib.stream()))
        got['parts, %d plane(s)' % planes] = (pr.cpu().numpy(), dl.cpu().numpy())
    p0, d0 = got['per level']
    assert (p0[B] == CANARY).all() and (d0[B] == CANARY).all() and (p0[:B] != CANARY).all() and (d0[:B] != CANARY).all()
    for name, (p, d) in got.items():
        assert np.array_equal(_bits(p), _bits(p0)) and np.array_equal(_bits(d), _bits(d0)), name
