"""CPU: the numpy restatement of the 3 x f16 backward (tests/conv_backward_f16x3_ref.py) against float64 torch autograd
(tests/conv_backward_ref.py) on the GPU tests' cases, and the derived bound on it -- the bound the GPU tests assert first."""
import numpy as np
import pytest
import torch

import conv_backward_f16x3_ref as R3
import conv_backward_ref as R


def _grads(c, dy_scale=1.0):
    cin, cout = c['cin'], c['cout']
    x = c['x'][..., :cin].contiguous()
    dy = (c['dy_full'][..., c['yco']:c['yco'] + cout] * dy_scale).contiguous()
    ref = R.conv_backward(x, c['w'], dy, c['stride'], c['pad'], y32=c['y32'], relu=c['relu'])
    g = ref['g'].float().numpy()                        # the masked gradient is exact in float32
    dx, dw = R3.conv_backward3(x.numpy(), c['w'].numpy(), g, c['stride'], c['pad'])
    return ref, g, x.numpy(), dx, dw


@pytest.mark.parametrize('name', sorted(R3.CASES))
def test_restatement_meets_the_bound(name):
    c = R3.make_case(name)
    ref, g, x, dx, dw = _grads(c)
    M = c['B'] * c['OH'] * c['OW']
    gmax, wmax, xmax = np.abs(g).max(), c['w'].abs().max(), np.abs(x).max()
    for n, got, k_terms, bmax in (('dx', dx, c['k'] ** 2 * c['cout'], wmax), ('dw', dw, M, xmax)):
        err = (torch.from_numpy(got).double() - ref[n]).abs()
        lim = R3.bound(k_terms, 0, ref['S_' + n], gmax, bmax)
        worst = float((err / lim).max())
        print('%s %s: max err / bound %.4f, normalised %.3e' % (name, n, worst, float(err.max() / ref[n].abs().max())))
        assert worst <= 1.0, (name, n, worst)
        assert float(err.max() / ref[n].abs().max()) < 1e-5     # fp32-class, nowhere near float16's 1e-3


def test_scale_follows_the_tensor():
    """dy times a power of two gives the same gradients times that power, bit for bit: the scale is taken from the tensor."""
    c = R3.make_case('ragged_3x3')
    _, _, _, dx, dw = _grads(c)
    for p in (-40, 30):
        _, _, _, dx2, dw2 = _grads(c, 2.0 ** p)
        assert np.array_equal(dx2, dx * np.float32(2.0 ** p)) and np.array_equal(dw2, dw * np.float32(2.0 ** p))


def test_scale_of():
    assert R3.scale_of(np.zeros(4, np.float32)) == np.float32(2.0 ** 126)
    assert R3.scale_of(np.array([1.0, -1.5], np.float32)) == np.float32(2.0 ** 14)
    assert R3.scale_of(np.array([3e-7], np.float32)) == np.float32(2.0 ** 36)          # 3e-7 = 1.26 * 2^-22
    hi, lo = R3.split(np.array([3e-7, 1e-9], np.float32), R3.scale_of(np.array([3e-7], np.float32)))
    assert float(hi[0]) >= 2.0 ** 14 and np.isfinite(hi).all() and float(lo[1]) != 0.0


def test_zero_gradient_gives_zeros():
    c = R3.make_case('single_k_tile')
    g = np.zeros((c['B'], c['OH'], c['OW'], c['cout']), np.float32)
    dx, dw = R3.conv_backward3(c['x'].numpy(), c['w'].numpy(), g, c['stride'], c['pad'])
    assert not dx.any() and not dw.any() and np.isfinite(dx).all() and np.isfinite(dw).all()
