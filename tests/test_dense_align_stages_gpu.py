"""csrc/dense_align.hip stage by stage against the references of tests/dense_align_ref.py, on the small constructed scenes of
tests/dense_align_scenes.py (validated on the CPU by tests/test_dense_align_ref_cpu.py): the upsample bit for bit, the lattice
and its compaction ORDER exactly, the overflow path, the taps, every cost of both searches, both argmins, and batches of more
than 64 objects.  The intermediates come out of the call's workspace (srcnn_dense_align_workspace_layout with 11 offsets).

Each stage is fed the device's own output of the stage before, so a deviation belongs to the stage it is found in."""
import numpy as np
import pytest
import torch

import dense_align_ref as ref
import dense_align_scenes as sc
import tolerances

pytestmark = pytest.mark.gpu

CANARY = 0xA5                       # every byte of the workspace before a call; 0xA5A5A5A5 is no coordinate and no count
UPSAMPLE_SIZES = [(2, 2), (3, 5), (5, 257), (13, 256), (96, 320)]
_cache = {}


def _images():
    if 'img' not in _cache:
        from stereo_rcnn_amd import fixture
        l, r, info = fixture.make_inputs(sc.SEED, 60, 200, target_short=96)
        assert tuple(l.shape) == (1, 3, sc.H, sc.W) and abs(float(info[0, 2]) - sc.SCALE) < 1e-6
        _cache['img'] = (l, r)
    return _cache['img']


def _call(dev, im_l, im_r, names, valid=None, max_pixels=None):
    """One native call on a workspace prefilled with the canary; everything it left behind, on the host."""
    from stereo_rcnn_amd import _lib
    from stereo_rcnn_amd.model.dense_align import dense_align as da
    mp = da.MAX_PIXELS if max_pixels is None else max_pixels
    poses, boxes, kp = [torch.from_numpy(a).to(dev) for a in sc.arrays(names)]
    Hh, Ww = im_l.shape[2], im_l.shape[3]
    ws = _lib.workspace(_lib.lib().srcnn_dense_align_workspace_bytes(Hh, Ww, len(names), mp), dev, "dense_align")
    ws.fill_(CANARY)
    v = None if valid is None else torch.tensor(valid, dtype=torch.float32, device=dev)
    st, dis, s = da.align_parallel(sc.calib(), sc.SCALE, im_l.to(dev), im_r.to(dev), boxes, kp, poses, valid=v,
                                   return_search='stages', max_pixels=mp)
    torch.cuda.synchronize()
    out = {k: t.cpu().numpy() for k, t in s.items()}
    out.update(status=st.cpu().numpy(), best_dis=dis.cpu().numpy(), names=list(names), max_pixels=mp)
    return out


def _scene(dev, key, max_pixels=None):
    """A scene's call, made once and shared (read-only) by the tests that look at different stages of it."""
    k = (key, max_pixels)
    if k not in _cache:
        names = sc.many(int(key[4:])) if key.startswith('many') else [key[4:]] if key.startswith('one:') else sc.SCENES[key]
        valid = None
        if key in sc.MASKED:
            valid = [0.0 if i in sc.MASKED[key] else 1.0 for i in range(len(names))]
        l, r = _images()
        out = _call(dev, l, r, names, valid, max_pixels)
        out['live'] = [valid is None or valid[i] > 0 for i in range(len(names))]
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[k] = out
    return _cache[k]


def _expected(out, i):
    """(count, u, v, dz) of object i from the float64 reference; a row the valid mask switched off has no sample."""
    L = sc.lattice(out['names'][i])
    m = L['mask'] if out['live'][i] else np.zeros(len(L['mask']), bool)
    return int(m.sum()), L['u'][m], L['v'][m], L['dz'][m]


def _canary(a):
    return np.ascontiguousarray(a).view(np.uint8) == CANARY


# ------------------------------------------------------------------ upsample2x_kernel
@pytest.mark.parametrize("Hh,Ww", UPSAMPLE_SIZES)
def test_upsample_equals_the_float32_restatement(dev, Hh, Ww):
    """Bit for bit (the library is built with -ffp-contract=off), and within the derived bound of float64.  Ragged last row
    block at 2H = 10 and 26, a second x-workgroup from W = 257, the last column pair; every plane of either eye has its own
    value range, so a swapped z = image * 3 + plane shows."""
    rng = np.random.default_rng(Hh * 1000 + Ww)
    base = np.array([[10.0, 80.0, 150.0], [220.0, 290.0, 360.0]])
    imgs = [(rng.random((3, Hh, Ww)) * 50 + base[e][:, None, None]).astype(np.float32) for e in range(2)]
    out = _call(dev, torch.from_numpy(imgs[0])[None], torch.from_numpy(imgs[1])[None], ['nr0'])
    for e, key in enumerate(('up_left', 'up_right')):
        want32, want64 = ref.upsample2x_f32(imgs[e]), ref.upsample2x_f64(imgs[e])
        got = out[key]
        assert got.shape == want32.shape
        d = tolerances.observe('dense_align_upsample_vs_f64_over_bound',
                               np.abs(got.astype(np.float64) - want64).max() / ref.upsample_bound(Hh, Ww, np.abs(imgs[e]).max()))
        print("upsample %dx%d %s: %d of %d values differ from the float32 restatement; |device - f64| = %.3f of the bound"
              % (Hh, Ww, key, int((got != want32).sum()), got.size, d))
        assert np.array_equal(got, want32)
        assert d <= 1.0


# ------------------------------------------------------------------ sample_kernel
@pytest.mark.parametrize("scene", ['totals', 'edges', 'allmiss'])
def test_sample_stage_lattice_order_and_canary(dev, scene):
    out = _scene(dev, scene)
    assert not out['overflow'].any()
    total = 0
    for i, n in enumerate(out['names']):
        c, u, v, dz = _expected(out, i)
        total += c
        assert int(out['count'][i]) == c, (n, int(out['count'][i]), c)
        uvz = out['uvz'][i]
        assert np.array_equal(uvz[:c, 0], u.astype(np.float32)) and np.array_equal(uvz[:c, 1], v.astype(np.float32)), n
        if c:
            d = tolerances.observe('dense_align_dz', np.abs(uvz[:c, 2].astype(np.float64) - dz).max())
            assert d <= tolerances.DENSE_ALIGN_DZ, (n, d)
        assert _canary(uvz[c:]).all(), "%s: rows beyond count were written" % n
        assert _canary(out['left_val'][i][c:]).all(), "%s: taps beyond count were written" % n
    want = [1.0 if total and _expected(out, i)[0] else 0.0 for i in range(len(out['names']))]
    assert out['status'].tolist() == want


def test_overflow_is_reported_and_spills_nowhere(dev):
    from stereo_rcnn_amd.model.dense_align import dense_align as da
    full = _scene(dev, 'overflow')
    C = _expected(full, 1)[0]
    assert C == 257 and int(full['count'][1]) == C and full['status'].tolist() == [1.0, 1.0, 1.0]
    fit = _scene(dev, 'overflow', C)                                  # exactly fits
    assert fit['status'].tolist() == [1.0, 1.0, 1.0] and not fit['overflow'].any()
    for k in ('count', 'best_dis', 'coarse_cost', 'fine_cost', 'coarse_depth', 'fine_depth'):
        assert np.array_equal(fit[k], full[k]), k
    assert np.array_equal(fit['uvz'], full['uvz'][:, :C]) and np.array_equal(fit['left_val'], full['left_val'][:, :C])
    for mp in (C - 1, 1):
        cut = _scene(dev, 'overflow', mp)
        want_st = [1.0 if _expected(full, i)[0] <= mp else -1.0 for i in range(3)]
        assert want_st[1] == -1.0 and cut['status'].tolist() == want_st
        for i in range(3):
            c = _expected(full, i)[0]
            assert int(cut['overflow'][i]) == (c if c > mp else 0) and int(cut['count'][i]) == min(c, mp)
            assert np.array_equal(cut['uvz'][i, :min(c, mp)], full['uvz'][i, :min(c, mp)])     # the FIRST lattice points, in order
            assert _canary(cut['uvz'][i, min(c, mp):]).all()
            if want_st[i] == 1.0:                                     # the neighbours of the overflowing row are untouched
                assert np.array_equal(cut['best_dis'][i], full['best_dis'][i])
                assert np.array_equal(cut['coarse_cost'][:, i], full['coarse_cost'][:, i])
                assert np.array_equal(cut['left_val'][i, :c], full['left_val'][i, :c])
        with pytest.raises(RuntimeError):
            da.check_status(cut['status'])
    assert _scene(dev, 'overflow', C - 1)['status'].tolist() == [1.0, -1.0, 1.0]
    da.check_status(full['status'])


# ------------------------------------------------------------------ left_sample_kernel / cost_kernel / argmin / finish
def _enum_f32(z, best=None):
    """make_enum_kernel's hypotheses, operation by operation in float32 (dense_align.py:265,283-285,291-294)."""
    f = np.float32
    scale2 = sc.SCALE * 2
    c = sc.calib()
    ff = c.p2[0, 0] * scale2
    bl = (c.p2[0, 3] - c.p3[0, 3]) * scale2 / ff
    if best is None:
        dis_init = (f(1) / f(z)) * f(ff * bl)
        d = np.array([(((f(1) / dis_init) * f(ff)) * f(bl) - f(12.5)) + f(0.5 * i) for i in range(50)], f)
        return np.maximum(d, f(1.5))
    return np.array([(f(best) - f(0.5)) + f(0.05 * i) for i in range(20)], f)


def _check_search(out, i):
    """Object i's taps, costs, argmins and disparity against float64 on the device's own images, lattice and hypotheses."""
    n = out['names'][i]
    c = int(out['count'][i])
    uvz, lv = out['uvz'][i, :c], out['left_val'][i, :c]
    u, v, dz = uvz[:, 0], uvz[:, 1], uvz[:, 2]
    d = tolerances.observe('dense_align_tap', np.abs(lv.astype(np.float64) - ref.taps_f64(out['up_left'], u.astype(np.float64), v.astype(np.float64))).max())
    assert d <= tolerances.DENSE_ALIGN_TAP, (n, d)
    z = np.float32(sc.OBJECTS[n][0][2])
    assert np.array_equal(out['coarse_depth'][:, i], _enum_f32(z)), n
    bound = float(ref.order_bound(c))
    best = None
    for stage, iters in (('coarse', 50), ('fine', 20)):
        depths = out[stage + '_depth'][:iters, i]
        got = out[stage + '_cost'][:iters, i].astype(np.float64)
        want = sc.costs_f64(out['up_right'], lv, u, v, dz, depths, np.float32)
        rel = tolerances.observe('dense_align_cost_over_order_bound', (np.abs(got - want) / np.maximum(want, 1e-30)).max() / bound)
        print("%s %s: %d pixels, max |cost - f64| / cost = %.3f of the summation-order bound %.2e" % (n, stage, c, rel, bound))
        assert rel <= 1.0, (n, stage, rel)
        a = sc.first_argmin(want)
        assert sc.first_argmin(got) == a, (n, stage, sc.first_argmin(got), a)
        same = np.nonzero(depths == depths[a])[0]                     # equal hypotheses (clamped to 1.5 m): bit-identical costs,
        assert (out[stage + '_cost'][same, i] == out[stage + '_cost'][a, i]).all() and a == same[0]      # and the first one wins
        if stage == 'coarse':
            clamped = np.nonzero(depths == np.float32(1.5))[0]
            assert len(set(out['coarse_cost'][clamped, i].tolist())) <= 1, n
            assert np.array_equal(out['fine_depth'][:20, i], _enum_f32(z, depths[a])), n
        assert out[stage + '_best'][i] == depths[a], (n, stage)
        best = float(depths[a])
    want_dis = sc.fb() / (best * sc.SCALE * 2) + 0.5
    d = tolerances.observe('dense_align_stage_best_dis_px', abs(float(out['best_dis'][i]) - want_dis))
    assert d < 2e-5, (n, d)


@pytest.mark.parametrize("scene", ['totals', 'edges'])
def test_taps_costs_and_argmins_against_float64(dev, scene):
    out = _scene(dev, scene)
    live = [i for i in range(len(out['names'])) if out['count'][i] > 0]
    assert len(live) >= 5
    for i in live:
        _check_search(out, i)
    z14 = [i for i in live if sc.OBJECTS[out['names'][i]][0][2] < 14]
    assert z14 and all((out['coarse_depth'][:3, i] == np.float32(1.5)).all() for i in z14)


def test_clamped_right_taps_at_the_left_edge(dev):
    """The close object at column 0: under the hypotheses near its initial depth every right tap clamps at x = 0 (has nothing to
    its west), and the device's costs still meet float64 there -- checked above; here: that those hypotheses exist in the call."""
    out = _scene(dev, 'edges')
    i = out['names'].index('left')
    c = int(out['count'][i])
    u, dz = out['uvz'][i, :c, 0], out['uvz'][i, :c, 2]
    n_clamped = [int((ref.right_u(u, dz, d, sc.fb()) < 0).sum()) for d in out['coarse_depth'][:, i]]
    assert max(n_clamped) == c and any(0 < k < c for k in n_clamped), (min(n_clamped), max(n_clamped), c)


# ------------------------------------------------------------------ more than 64 objects
@pytest.mark.parametrize("R", [65, 130])
def test_many_objects_equal_their_lone_runs(dev, R):
    """The second (and third) block of argmin_kernel / finish_kernel and the `it * R + r` indexing at R not a multiple of 64:
    every live object's result is bit for bit what the same object gives alone (R = 1)."""
    out = _scene(dev, 'many%d' % R)
    assert len(out['names']) == R and not out['overflow'].any()
    for i, n in enumerate(out['names']):
        c = _expected(out, i)[0]
        assert int(out['count'][i]) == c and out['status'][i] == (1.0 if c else 0.0), (i, n)
        if not c:
            continue
        one = _scene(dev, 'one:' + n)
        for k in ('coarse_depth', 'coarse_cost', 'fine_depth', 'fine_cost'):
            assert np.array_equal(out[k][:, i], one[k][:, 0]), (i, n, k)
        for k in ('coarse_best', 'fine_best', 'best_dis', 'status'):
            assert out[k][i] == one[k][0], (i, n, k)
        assert np.array_equal(out['uvz'][i, :c], one['uvz'][0, :c]) and np.array_equal(out['left_val'][i, :c], one['left_val'][0, :c])
    for n in sorted(set(out['names'])):                               # status, count and argmin of the lone runs: the reference's
        one = _scene(dev, 'one:' + n)
        if one['count'][0]:
            _check_search(one, 0)
    for i in (R - 1, R - 2, 64, 63):                                  # and directly in the batch, around the block boundary
        if out['count'][i]:
            _check_search(out, i)


@pytest.mark.parametrize("R", [65, 130])
def test_many_empty_objects_keep_their_initial_disparity(dev, R):
    names = [('miss', 'nr0', 'nc0')[i % 3] for i in range(R)]
    l, r = _images()
    out = _call(dev, l, r, names)
    assert not out['count'].any() and not out['overflow'].any() and not out['status'].any()
    f = np.float32
    want = np.array([(f(1) / f(sc.OBJECTS[n][0][2])) * f(sc.fb()) for n in names], f)          # dis_init (dense_align.py:265)
    assert np.array_equal(out['best_dis'], want)
    assert _canary(out['uvz']).all()
