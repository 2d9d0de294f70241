"""The stage references of tests/dense_align_ref.py and the scenes of tests/dense_align_scenes.py, validated on the CPU before
any device sees them: the float32 restatement of the upsample against float64, the float64 lattice against the oracle, the
scene CONDITIONS (decision margins, tie-free argmins -- conditions the reference alone satisfies, not measurements of a device)
and that every edge scene really reaches its edge.  Also holds the oracle-against-float64 deviations that
tests/tolerances.py turns into DENSE_ALIGN_DZ / DENSE_ALIGN_TAP."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_align_ref as ref
import dense_align_scenes as sc
import tolerances

ORACLE_SCENES = ['totals', 'edges', 'overflow', 'allmiss', 'many65']
UPSAMPLE_SIZES = [(2, 2), (3, 5), (5, 257), (13, 256), (96, 320)]


def _names(scene):
    return sc.many(65) if scene == 'many65' else sc.SCENES[scene]


_cache = {}


def _images():
    if 'img' not in _cache:
        from stereo_rcnn_amd import fixture
        l, r, info = fixture.make_inputs(sc.SEED, 60, 200, target_short=96)
        assert tuple(l.shape) == (1, 3, sc.H, sc.W) and abs(float(info[0, 2]) - sc.SCALE) < 1e-6
        _cache['img'] = (l, r, info)
    return _cache['img']


def _oracle(scene):
    """The oracle's whole alignment of one scene plus, per object, the float64 evaluation on the oracle's own upsampled images."""
    if scene in _cache:
        return _cache[scene]
    from oracle import dense_align as oda
    l, r, info = _images()
    names = _names(scene)
    poses, boxes, kp = [torch.from_numpy(a) for a in sc.arrays(names)]
    st, dis, ex = oda.align_parallel(sc.calib(), sc.SCALE, l, r, boxes, kp, poses, return_extra=True)
    up = lambda t: F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=True)
    up_l, up_r = up(l)[0].numpy(), up(r)[0].numpy()
    objs = []
    for i, n in enumerate(names):
        L = sc.lattice(n)
        m = L['mask']
        o = {'name': n, 'L': L, 'count': int(m.sum())}
        if ex and o['count']:
            u, v, dz = L['u'][m], L['v'][m], L['dz'][m]
            o['left'] = ref.taps_f64(up_l, u.astype(np.float64), v.astype(np.float64))
            o['coarse'] = sc.costs_f64(up_r, o['left'], u, v, dz, ex['depth_enum'][:, i].numpy())
            best = ex['coarse_depth'][i:i + 1]
            fine = torch.stack([best - 20 * 0.05 / 2 + 0.05 * k for k in range(20)])[:, 0].numpy()       # dense_align.py:290-294
            o['fine'] = sc.costs_f64(up_r, o['left'], u, v, dz, fine)
        objs.append(o)
    _cache[scene] = (st, dis, ex, objs, up_l, up_r)
    return _cache[scene]


# ------------------------------------------------------------------ upsample
def _upsample_image(Hh, Ww):
    """Distinct non-negative values per plane (callers give each eye its own offset): neighbouring values differ by less than
    the largest, which is what the derived bound assumes of the source."""
    rng = np.random.default_rng(Hh * 1000 + Ww)
    return (rng.random((3, Hh, Ww)) * 50 + np.array([10.0, 80.0, 150.0])[:, None, None]).astype(np.float32)


@pytest.mark.parametrize("Hh,Ww", UPSAMPLE_SIZES)
def test_upsample_f32_restatement_within_the_derived_bound_of_f64(Hh, Ww):
    img = _upsample_image(Hh, Ww)
    a, b = ref.upsample2x_f32(img), ref.upsample2x_f64(img)
    assert a.shape == (3, 2 * Hh, 2 * Ww)
    d = float(np.abs(a.astype(np.float64) - b).max())
    bound = ref.upsample_bound(Hh, Ww, np.abs(img).max())
    t = F.interpolate(torch.from_numpy(img)[None], scale_factor=2, mode='bilinear', align_corners=True)[0].numpy()
    print("upsample2x_f32 %dx%d: max |f32 - f64| %.3e (bound %.3e); bit-equal to F.interpolate(align_corners=True): %s (max diff %.3e)"
          % (Hh, Ww, d, bound, bool(np.array_equal(a, t)), float(np.abs(a - t).max())))
    assert d <= bound
    # the corners are the source's corners, exactly (align_corners)
    assert a[:, 0, 0].tolist() == img[:, 0, 0].tolist()
    assert np.abs(a[:, -1, -1] - img[:, -1, -1]).max() <= bound


def test_upsample_reference_on_the_network_input():
    l, r, _ = _images()
    for t in (l, r):
        img = t[0].numpy()
        d = float(np.abs(ref.upsample2x_f32(img).astype(np.float64) - ref.upsample2x_f64(img)).max())
        assert d <= ref.upsample_bound(sc.H, sc.W, np.abs(img).max())
        assert np.abs(np.diff(img, axis=1)).max() <= np.abs(img).max() and np.abs(np.diff(img, axis=2)).max() <= np.abs(img).max()


# ------------------------------------------------------------------ lattice against the oracle
@pytest.mark.parametrize("scene", ORACLE_SCENES)
def test_lattice_f64_agrees_with_the_oracle(scene):
    """Count, (u, v) and ORDER exactly; dz within the oracle's own float32 deviation, which this test holds at the value
    tests/tolerances.py records."""
    from oracle import dense_align as oda
    names = _names(scene)
    poses, boxes, kp = [torch.from_numpy(a) for a in sc.arrays(names)]
    s2 = sc.SCALE * 2
    uvz, w = oda.sample(sc.calib(), s2, sc.H2, sc.W2, boxes * s2, poses, (kp * s2)[:, 3:5])
    worst = 0.0
    for i, n in enumerate(names):
        L = sc.lattice(n)
        m = L['mask']
        c = int(m.sum())
        assert int(w[i].sum()) == c, (n, int(w[i].sum()), c)
        assert np.array_equal(uvz[i, :c, 0].numpy(), L['u'][m].astype(np.float32)), n
        assert np.array_equal(uvz[i, :c, 1].numpy(), L['v'][m].astype(np.float32)), n
        if c:
            worst = max(worst, float(np.abs(uvz[i, :c, 2].numpy().astype(np.float64) - L['dz'][m]).max()))
    print("oracle (float32) against lattice_f64, scene %s: max |dz| deviation %.3e m" % (scene, worst))
    assert worst <= tolerances.DENSE_ALIGN_DZ_REFERENCE_MEASURED
    assert tolerances.DENSE_ALIGN_DZ == pytest.approx(4 * tolerances.DENSE_ALIGN_DZ_REFERENCE_MEASURED)


@pytest.mark.parametrize("scene", ORACLE_SCENES)
def test_oracle_left_taps_against_taps_f64(scene):
    """F.grid_sample in float32 (what the oracle's cost reads for the left image) against taps_f64 at the exact lattice point, on
    the same upsampled image: the reference's own deviation behind DENSE_ALIGN_TAP."""
    _, _, _, objs, up_l, _ = _oracle(scene)
    worst = 0.0
    for o in objs:
        if not o['count']:
            continue
        m = o['L']['mask']
        u, v = torch.from_numpy(o['L']['u'][m].astype(np.float32)), torch.from_numpy(o['L']['v'][m].astype(np.float32))
        f_w, f_h = float(sc.W2) - 1, float(sc.H2) - 1
        g = torch.stack(((u - f_w / 2) / (f_w / 2), (v - f_h / 2) / (f_h / 2)), 1).view(1, 1, -1, 2)      # dense_align.py:194-202
        t = F.grid_sample(torch.from_numpy(up_l)[None], g, mode='bilinear', padding_mode='border', align_corners=True)[0, :, 0].t()
        worst = max(worst, float(np.abs(t.numpy().astype(np.float64) - ref.taps_f64(up_l, u.numpy(), v.numpy())).max()))
    print("oracle (float32) left taps against taps_f64, scene %s: max deviation %.3e" % (scene, worst))
    assert worst <= tolerances.DENSE_ALIGN_TAP_REFERENCE_MEASURED
    assert tolerances.DENSE_ALIGN_TAP == pytest.approx(4 * tolerances.DENSE_ALIGN_TAP_REFERENCE_MEASURED)


@pytest.mark.parametrize("scene", ORACLE_SCENES)
def test_oracle_argmins_agree_with_the_float64_costs(scene):
    st, dis, ex, objs, _, _ = _oracle(scene)
    counts = [o['count'] for o in objs]
    if sum(counts) == 0:
        assert ex == {} and st.tolist() == [0.0] * len(objs)
        return
    assert st.tolist() == [1.0 if c else 0.0 for c in counts]
    worst = 0.0
    for i, o in enumerate(objs):
        if not o['count']:
            continue
        for stage, cost in (('coarse', ex['coarse_cost']), ('fine', ex['fine_cost'])):
            assert sc.first_argmin(cost[:, i].numpy()) == sc.first_argmin(o[stage]), (o['name'], stage)
            worst = max(worst, float(np.abs(cost[:, i].numpy() - o[stage]).max() / o[stage].max()))
    print("oracle costs against the all-float64 costs, scene %s: max deviation %.3e of the largest cost" % (scene, worst))


# ------------------------------------------------------------------ scene conditions
def test_every_lattice_pixel_has_a_decision_margin():
    for n in sc.OBJECTS:
        L = sc.lattice(n)
        if len(L['margin']):
            assert float(L['margin'].min()) >= sc.MARGIN, (n, float(L['margin'].min()))
        assert L['nearest_gap'] >= 1e-2, (n, L['nearest_gap'])        # metres: no float32 evaluation picks another nearest vertex


@pytest.mark.parametrize("scene", ORACLE_SCENES)
def test_no_argmin_is_a_near_tie(scene):
    _, _, ex, objs, _, _ = _oracle(scene)
    for o in objs:
        if ex and o['count']:
            for stage in ('coarse', 'fine'):
                why = sc.near_tie(o[stage], o['count'])
                assert why is None, (o['name'], stage, why)


# ------------------------------------------------------------------ the edges are reached
def test_lattice_totals_occur():
    counts = {n: int(sc.lattice(n)['mask'].sum()) for n in sc.SCENES['totals']}
    assert [counts[n] for n in ('n1', 'n63', 'n64', 'n65', 'n255', 'n256', 'n257')] == [1, 63, 64, 65, 255, 256, 257], counts
    big = sc.lattice('big')
    assert counts['big'] > 1024 and big['nr'] * big['nc'] - counts['big'] > 100           # several rounds, and it compacts
    assert set(big['plane'][big['mask']].tolist()) == {0, 1}                              # first plane misses, second hits
    assert len(set((np.nonzero(~big['mask'])[0] // 256).tolist())) >= 3                   # misses inside several 256-pixel rounds
    assert 0 < int((~sc.lattice('n257')['mask']).sum()) and 0 < int((~sc.lattice('n256')['mask']).sum())


def test_edge_scenes_reach_their_edges():
    la = sc.lattice
    L = la('left')
    assert L['c0'] == 0 and L['mask'][L['u'] == 0].any()
    # right taps clamped at x = 0 for part of the hypotheses: under the initial depth every valid pixel's u - gdd is negative,
    # 12 m behind it only the leftmost columns' are
    m, z = L['mask'], float(np.float32(sc.OBJECTS['left'][0][2]))
    ur = ref.right_u(L['u'][m], L['dz'][m], z, sc.fb())
    assert (ur < 0).all()
    assert (ref.right_u(L['u'][m], L['dz'][m], z + 12.0, sc.fb())[L['u'][m] > 40] > 0).all()
    L = la('right')
    assert L['c1'] == sc.W2 and L['mask'][L['u'] == sc.W2 - 1].any()
    L = la('bottom')
    assert L['r1'] == sc.H2 and L['mask'][L['v'] == sc.H2 - 1].any()
    assert la('hstep')['hstep'] > 1 and la('hstep')['mask'].any()
    assert la('n257')['wstep'] > 1 and la('big')['wstep'] > 1
    assert la('nr0')['nr'] == 0 and la('nr0')['nc'] > 0
    assert la('nc0')['nc'] == 0 and la('nc0')['nr'] > 0
    assert la('miss')['nr'] * la('miss')['nc'] > 0 and not la('miss')['mask'].any()
    L = la('n63')                                                                         # borders narrower than the box
    assert L['c1'] - L['c0'] < 0.2 * (sc.OBJECTS['n63'][1][2] - sc.OBJECTS['n63'][1][0]) * sc.SCALE * 2
    e = sc.SCENES['edges']
    k = sc.MASKED['edges'][0]
    assert la(e[k])['mask'].any() and la(e[k - 1])['mask'].any() and la(e[k + 1])['mask'].any()
    assert all(float(sc.OBJECTS[n][0][2]) < 14 for n in ('left', 'bottom', 'hstep', 'big'))
    for n in sc.SMALL:
        assert int(la(n)['mask'].sum()) <= 255
