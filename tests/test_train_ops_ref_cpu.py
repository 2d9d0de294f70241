"""CPU: the float64 restatement of the three training adjoints (tests/train_ops_ref.py) against torch.autograd of
F.interpolate(mode='bilinear', align_corners=True), strided slicing and F.conv_transpose2d, and against the inner-product
identity <U x, g> = <x, U^T g>."""
import pytest
import torch
import torch.nn.functional as F

import train_ops_ref as T

UP_SHAPES = [((4, 11), (7, 21)), ((7, 21), (13, 41)), ((13, 41), (26, 82)), ((1, 1), (3, 5)), ((5, 5), (5, 5)), ((2, 3), (2, 7)),
             ((3, 2), (1 + 2 * 37, 2))]


@pytest.mark.parametrize('top_hw,out_hw', UP_SHAPES)
def test_upsample_backward_against_interpolate(top_hw, out_hw):
    (TH, TW), (H, W) = top_hw, out_hw
    gen = torch.Generator().manual_seed(7)
    top = torch.randn(2, TH, TW, 8, generator=gen)
    dy = torch.randn(2, H, W, 8, generator=gen)
    t = top.double().permute(0, 3, 1, 2).requires_grad_(True)
    up = F.interpolate(t, size=(H, W), mode='bilinear', align_corners=True)
    up.backward(dy.double().permute(0, 3, 1, 2))
    # the restatement's float32 tap weights against float64 ones: one float32 rounding of rh * h per axis, coefficients <= 1
    tol = 8 * max(H, W) * T.U
    fwd = T.upsample(top, H, W)
    assert float((fwd - up.detach().permute(0, 2, 3, 1)).abs().max()) <= tol * float(top.abs().max())
    g, S = T.upsample_add_backward(dy, TH, TW)
    assert g.shape == (2, TH, TW, 8)
    assert bool(((g - t.grad.permute(0, 2, 3, 1)).abs() <= tol * S + 1e-300).all())
    # each output pixel's coefficients sum to 1 (to float32 rounding), so the adjoint keeps the total
    assert abs(float(g.sum() - dy.double().sum())) <= tol * float(dy.abs().sum())
    # inner-product identity, exact up to float64 rounding
    lhs, rhs = float((fwd * dy.double()).sum()), float((top.double() * g).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((fwd.abs() * dy.double().abs()).sum())


def _round_f32(fr):
    """Correctly rounded (nearest, ties to even) float32 of an exact Fraction of normal magnitude."""
    from fractions import Fraction
    if fr == 0:
        return 0.0
    sign, fr = (-1 if fr < 0 else 1), abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    q = fr / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return sign * float(n) * 2.0 ** (e - 23)


def test_fmaf32_rounds_once():
    """train_ops_ref.fmaf32 against exact rational arithmetic: random operands, and sums that land exactly between two float32
    values once the product's low bits are dropped (where rounding the float64 sum a second time goes wrong)."""
    import numpy as np
    from fractions import Fraction
    rng = np.random.default_rng(5)
    k = rng.random(2000).astype(np.float32)
    v = rng.normal(0, 1, 2000).astype(np.float32)
    acc = (rng.normal(0, 1, 2000) * 10.0 ** rng.integers(-3, 4, 2000)).astype(np.float32)
    # k v = 2^-14 (1 - 2^-46): 2^-60 short of half a float32 ulp of acc = 2^10 (1 + 2^-23), whose last bit is odd.  The float64
    # sum drops the 2^-60 and lands on the tie, which a second rounding would resolve upwards (to even); once rounded, acc stays.
    # Mirrored in sign, and the true tie (k v = 2^-14) for contrast.
    e = np.float32(1.0 + 2.0 ** -23)
    k = np.concatenate([k, np.float32([2.0 ** -14, 2.0 ** -14, 2.0 ** -14]) * np.float32([e, -e, 1.0])])
    v = np.concatenate([v, np.float32([1.0 - 2.0 ** -23, 1.0 - 2.0 ** -23, 1.0])])
    acc = np.concatenate([acc, np.float32([2.0 ** 10, -2.0 ** 10, 2.0 ** 10]) * e])
    got = T.fmaf32(k, v, acc)
    assert float(got[-3]) == float(acc[-3]) and float(got[-2]) == float(acc[-2]) and float(got[-1]) > float(acc[-1])
    assert got.dtype == np.float32
    for i in range(len(k)):
        want = _round_f32(Fraction(float(k[i])) * Fraction(float(v[i])) + Fraction(float(acc[i])))
        assert float(got[i]) == want, (i, float(k[i]), float(v[i]), float(acc[i]), float(got[i]), want)


@pytest.mark.parametrize('top_hw,out_hw', [((1, 1), (3, 5)), ((3, 4), (5, 7)), ((2, 2), (2, 2))])
def test_upsample_backward_f32_restatement_lies_within_the_bound_of_float64(top_hw, out_hw):
    """The float32 restatement the GPU test compares bits with, against the float64 one: (n + 2) u S as in the GPU test."""
    (TH, TW), (H, W) = top_hw, out_hw
    dy = torch.randn(2, H, W, 8, generator=torch.Generator().manual_seed(11))
    g32 = torch.from_numpy(T.upsample_add_backward_f32(dy.numpy(), TH, TW))
    g, S = T.upsample_add_backward(dy, TH, TW)
    n = 4 * H * W
    assert bool(((g32.double() - g).abs() <= (n + 2) * T.U * S + 1e-300).all())


def test_upsample_taps_are_in_range():
    for n_top, n_out in ((4, 7), (7, 13), (13, 26), (1, 3), (5, 5), (38, 75), (2, 1000)):
        i1, i2, l0, l1 = T.up_taps(n_out, n_top)
        assert i1.min() >= 0 and i2.max() <= n_top - 1
        assert (abs(l0.astype('float64') + l1 - 1) <= 2 * T.U).all() and (l1 >= 0).all() and (l1 < 1).all()


def test_gather_candidates_lose_no_term_for_any_size():
    """The kernel's candidate range (restated in train_ops_ref.up_candidates) against the taps of every output index: gathering
    over the candidates alone rebuilds the interpolation matrix exactly, for every n_top <= n_out up to 70, sizes around the
    pyramid's (.. -> 150, 497), extreme ratios and n_out = 1."""
    pairs = [(t, o) for o in range(1, 71) for t in range(1, o + 1)]
    pairs += [(75, 150), (249, 497), (38, 75), (125, 249), (19, 38), (63, 125), (2, 1000), (3, 4099), (999, 1000), (1000, 1000),
              (511, 1023), (333, 1000), (7, 2048)]
    for n_top, n_out in pairs:
        full, gathered = T.up_matrix(n_out, n_top), T.up_gather_matrix(n_out, n_top)
        assert torch.equal(full, gathered), (n_top, n_out)
        lo_hi = [T.up_candidates(n_out, n_top, t) for t in range(n_top)]
        assert all(0 <= lo <= hi <= n_out - 1 for lo, hi in lo_hi), (n_top, n_out)
        if n_top > 1 and n_out > 1:           # the range stays local: no more than the 2 / r indices it needs plus the slack
            assert max(hi - lo for lo, hi in lo_hi) <= 2.0 * (n_out - 1) / (n_top - 1) + 5, (n_top, n_out)


@pytest.mark.parametrize('H,W', [(7, 21), (4, 11), (2, 6), (1, 1), (5, 4)])
def test_subsample_backward_against_slicing(H, W):
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(2, H, W, 8, generator=gen, dtype=torch.float64).requires_grad_(True)
    y = x[:, ::2, ::2, :]
    assert y.shape[1:3] == ((H + 1) // 2, (W + 1) // 2) and torch.equal(T.subsample2(x.detach()), y.detach())
    dy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(dy)
    dx = T.subsample2_backward(dy, H, W)
    assert torch.equal(dx, x.grad)
    assert float((T.subsample2(x.detach()) * dy).sum()) == pytest.approx(float((x.detach() * dx).sum()), rel=1e-13)


def test_pixel_shuffle_round_trip_and_order():
    x = torch.arange(3 * 2 * 5 * 32, dtype=torch.float64).reshape(3, 2, 5, 32)
    y = T.pixel_shuffle2(x, 8)
    assert y.shape == (3, 4, 10, 8)
    for (m, a, b, i, j, co) in ((0, 0, 0, 0, 1, 3), (2, 1, 4, 1, 0, 7), (1, 1, 2, 1, 1, 0)):
        assert y[m, 2 * a + i, 2 * b + j, co] == x[m, a, b, (2 * i + j) * 8 + co]
    assert torch.equal(T.pixel_unshuffle2(y), x)


@pytest.mark.parametrize('cin,cout', [(32, 8), (64, 40)])
def test_conv_transpose_against_torch(cin, cout):
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(3, 5, 4, cin, generator=gen)
    w = torch.randn(cin, cout, 2, 2, generator=gen) / cin ** 0.5
    b = torch.randn(cout, generator=gen)
    g = torch.randn(3, 10, 8, cout, generator=gen)
    leaves = [t.double().requires_grad_(True) for t in (x.permute(0, 3, 1, 2), w, b)]
    y = F.conv_transpose2d(leaves[0], leaves[1], leaves[2], stride=2)
    y.backward(g.double().permute(0, 3, 1, 2))
    mine = T.conv_transpose2x2(x, w, b)
    assert float((mine - y.detach().permute(0, 2, 3, 1)).abs().max()) <= 1e-12
    r = T.conv_transpose2x2_backward(x, w, g)
    assert float((r['dx'] - leaves[0].grad.permute(0, 2, 3, 1)).abs().max()) <= 1e-12
    assert float((r['dw'] - leaves[1].grad).abs().max()) <= 1e-11
    assert float((r['db'] - leaves[2].grad).abs().max()) <= 1e-11
    # <U x, g> = <x, U^T g> for the linear part
    lin = mine - b.double()
    assert float((lin * g.double()).sum()) == pytest.approx(float((x.double() * r['dx']).sum()), rel=1e-10)
