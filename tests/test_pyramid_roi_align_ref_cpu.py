"""CPU: the references of tests/test_pyramid_roi_align_gpu.py (tests/pyramid_roi_align_ref.py) are pinned before a GPU sees them --
the exact one against the oracle's own pyramid routing, the derived float64 bound against the exact one (a correct implementation
satisfies it), the planted level ties against the derived window, and the case against what the issue asks of it."""
import numpy as np
import pytest
import torch

import pyramid_roi_align_ref as R
import roi_align_backward_ref as RB
import small_kernels_ref as SK

F = np.float32
FMTS = [R.F32, R.SPLIT16]


@pytest.fixture(scope='module')
def case():
    return R.build_case()


@pytest.mark.parametrize('A', [7, 14])
@pytest.mark.parametrize('mfmt', FMTS)
def test_exact_reference_is_the_oracles_pyramid_on_decided_rois(case, A, mfmt):
    """oracle.net.pyramid_roi_feat routes with torch float32 (stereo_rcnn.py:113-119); on every roi whose level is decided it must
    give the bits of exact_reference at the float64 level.  64 channels: the channels are independent."""
    from oracle import net as onet
    d = case['decided']
    vals = [np.ascontiguousarray(m[..., :64]) for m in R.map_values(mfmt)]
    rois = case['rois'][d]
    lv = onet.roi_levels(torch.from_numpy(rois)).numpy().astype(np.int64) - 2
    assert np.array_equal(lv, case['level'][d])
    ref = onet.pyramid_roi_feat([torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2))) for v in vals], torch.from_numpy(rois),
                                torch.tensor([[float(R.IM_H), float(R.IM_W), 1.0]]), kpts=(A == 14)).numpy()
    got = R.expected(mfmt, A)[d][..., :64]
    assert np.array_equal(got.view(np.int32), np.ascontiguousarray(ref.transpose(0, 2, 3, 1)).view(np.int32))
    # and the explicit level array is honoured: the same rois sent one level up or down give another result
    other = np.where(case['level'][d] < 3, case['level'][d] + 1, 2)
    moved = R.exact_reference(vals, rois, A, R.IM_H, other)
    inside = ~np.isin(case['name'][d], ['outside'])
    assert all((moved[i] != got[i]).any() for i in np.nonzero(inside)[0])


@pytest.mark.parametrize('A', [7, 14])
@pytest.mark.parametrize('mfmt', FMTS)
def test_exact_reference_within_the_derived_bound_of_float64(case, A, mfmt):
    """On all CMAX channels, hence on every case of the GPU table (a case reads the first C channels): float32 output and SPLIT16
    output, expected levels and the ties' other level.  Prints how much of the bound a correct implementation uses."""
    for alt in (False, True):
        ref, bound = R.expected64(mfmt, A, alt)
        exact = R.expected(mfmt, A, alt)
        for ofmt in FMTS:
            ok, err, allowed = R.within_bound(R.as_bits(exact, ofmt), ofmt, ref, bound)
            used = float((err / np.maximum(allowed, 1e-300)).max())
            print('A=%d maps=%d out=%d alt=%d: exact reference uses %.3f of the derived bound' % (A, mfmt, ofmt, alt, used))
            assert ok.all(), (used, float(err.max()))
    # the bound is about the magnitudes: nothing where nothing is sampled, and never below the value's own rounding
    ref, bound = R.expected64(mfmt, A)
    out = case['name'] == 'outside'
    assert (ref[out] == 0).all() and (bound[out] == 0).all() and (R.expected(mfmt, A)[out].view(np.int32) == 0).all()
    assert (bound >= float(RB.gamma(R.BOUND_C)) * np.abs(ref) * (1 - 1e-12)).all()


def test_lattice64_agrees_with_roi_align_torch64(case):
    """lattice64 (which supplies the magnitudes S of the bound) samples the same float32 coordinates with the same weights as
    roi_align_torch64: equal to 1e-13 of the magnitude on every roi of the case."""
    vals = [np.ascontiguousarray(m[..., :8]) for m in R.map_values(R.F32)]
    for i, roi in enumerate(case['rois']):
        l = int(case['level'][i])
        scale = R.level_scale(l)
        feat = torch.from_numpy(np.ascontiguousarray(vals[l].transpose(0, 3, 1, 2))).double()
        want = RB.roi_align_torch64(feat, roi[None].copy(), 15, 15, scale).numpy()[0].transpose(1, 2, 0)
        got = R.lattice64(vals[l], roi, 15, scale)
        mag = R.lattice64(vals[l], roi, 15, scale, absolute=True)
        assert (np.abs(got - want) <= 1e-13 * mag).all(), case['name'][i]
        assert (mag >= np.abs(got) * (1 - 1e-12)).all()


def test_case_rois(case):
    rois, kind, name, margin = case['rois'], case['kind'], case['name'], case['margin']
    n = len(rois)
    assert 64 <= n <= 96
    rnd = kind == 'random'
    assert (margin[rnd] >= R.RANDOM_MARGIN).all()
    for b in range(R.BATCH):
        assert set(case['level'][rnd & (rois[:, 0] == b)]) == {0, 1, 2, 3}
    tie = kind == 'tie'
    assert (margin[tie] < R.TIE_WINDOW).all() and R.TIE_WINDOW < 1e-5
    assert tie.sum() <= 0.1 * n
    for k in R.BOUNDARIES:
        t = tie & (case['tie_k'] == k)
        assert t.sum() >= 2
        assert all({int(case['level'][i]), int(case['alt'][i])} == {k - 2, k - 1} for i in np.nonzero(t)[0])
        assert all(R.device_level_set(rois[i]) <= {k - 2, k - 1} for i in np.nonzero(t)[0])
        near = np.array([nm.startswith('near%d' % k) for nm in name])
        assert (margin[near] >= R.NEAR_MARGIN[0]).all() and (margin[near] <= R.NEAR_MARGIN[1]).all()
        assert {int(v) for v in case['level'][near]} == {k - 2, k - 1}              # both sides of the boundary
    # at lv = 4.5 the planted rois are ties of the float32 evaluation itself, whose float64 level lies BELOW the boundary: round
    # half away sends them up, round half to even would not
    t4 = np.nonzero(tie & (case['tie_k'] == 4))[0]
    assert all(R.device_lv_interval(rois[i]) == (F(4.5), F(4.5)) and R.device_level_set(rois[i]) == {3} for i in t4)
    # a decided roi is decided for every admissible float32 evaluation
    for i in np.nonzero(case['decided'])[0]:
        assert R.device_level_set(rois[i]) == {int(case['level'][i])}, name[i]
    assert R.device_level_set(rois[name == 'negative-area'][0]) == {0}
    for nm in ('zero', 'negative-area', 'reversed', 'one-pixel', 'right-bottom', 'negative-start', 'outside', 'last-row-on-height'):
        assert (name == nm).sum() == 1
    assert (rois[name == 'zero'][0][1:] == 0).all()
    r = rois[name == 'negative-area'][0]
    assert r[3] < r[1]
    # the geometry the edge rois are there for, in the kernels' float32 arithmetic
    for A in (7, 14):
        a = A + 1

        def axes(nm):
            i = int(np.nonzero(name == nm)[0][0])
            l = int(case['level'][i])
            H, W = R.MAP_HW[l]
            _, sw, sh, bw, bh, _, _ = RB.roi_geometry(rois[i], R.level_scale(l), a, a)
            return ([RB.lattice_axis(j, bh, sh, 0.0, H) for j in range(a)], [RB.lattice_axis(j, bw, sw, 0.0, W) for j in range(a)], bw, bh, H, W)

        rows, cols, bw, bh, H, W = axes('last-row-on-height')
        assert float(rows[-1][3]) == H and not rows[-1][0] and rows[-2][0] and all(c[0] for c in cols)
        rows, cols, bw, bh, H, W = axes('negative-area')
        assert bw == 0 and bh > 0
        rows, cols, bw, bh, H, W = axes('reversed')
        assert bw == 0 and bh == 0
        rows, cols, bw, bh, H, W = axes('outside')
        assert not any(c[0] for c in cols) and not any(r_[0] for r_ in rows)
        for nm, first in (('right-bottom', True), ('negative-start', False)):
            rows, cols, bw, bh, H, W = axes(nm)
            for ax in (rows, cols):
                ok = [p[0] for p in ax]
                assert ok[0 if first else -1] and not ok[-1 if first else 0]             # partly inside, partly outside


@pytest.mark.parametrize('k', R.BOUNDARIES)
def test_planted_ties_are_found_anywhere(k):
    """the search is deterministic and does not depend on the spots the case uses"""
    a = R.plant_ties(k, 1, 33.125, 17.75, 25.0 * 2 ** (k - 1), count=3)
    assert np.array_equal(a, R.plant_ties(k, 1, 33.125, 17.75, 25.0 * 2 ** (k - 1), count=3))
    lv, m = RB.pyramid_levels(a)
    assert (m < R.TIE_WINDOW).all() and set(lv) <= {k - 2, k - 1} and len({tuple(r) for r in a}) == 3
    assert (a[:, 1:] != np.round(a[:, 1:])).any(axis=1).all()                           # fractional coordinates


def test_split16_maps_round_trip():
    for raw, val in zip(R.map_bytes(R.SPLIT16), R.map_values(R.SPLIT16)):
        assert np.array_equal(SK.split16_pack(SK.split16_unpack(raw)).view(np.int32), raw.view(np.int32))
        assert np.array_equal(R.split16_unpack64(raw), val.astype(np.float64))           # hi + lo is exact in float32 here
    # the format is lossy on these maps: the SPLIT16 cases do not see the float32 values
    assert (R.map_values(R.SPLIT16)[0] != R.map_values(R.F32)[0]).any()


def test_table_covers_every_form():
    """five instantiated forms x A in {7, 14}: the roi form, the row-pair form with one block row (C > 256) and with 64 / G rows
    per block (C <= 256, the child process), the per-channel kernel, and the roi form's shipped configurations."""
    cases = R.TABLE + R.FORM0 + [dict(R.BOX_HEAD, coffset=0)]
    for form in ('roi', 'rowpair', 'perchannel'):
        assert {c['A'] for c in cases if c['form'] == form} == {7, 14}
    for c in cases:
        aligned = c['cstride'] % 8 == 0 and c['coffset'] % 8 == 0
        want = 'perchannel' if not aligned else 'roi' if c['C'] <= 256 and c not in R.FORM0 else 'rowpair'
        assert c['form'] == want and c['C'] % 64 == 0 and c['coffset'] + c['C'] <= c['cstride']
    assert len({c['id'] for c in R.TABLE}) == len(R.TABLE)
    # the partial last block of the row-pair form: 64 / (C / 8) rows per block does not divide A
    assert any(c['A'] % (64 // (c['C'] // 8)) for c in R.FORM0 if c['A'] == 14)
