"""CPU: the numpy restatement of the 3 x f16 training forward (tests/conv_forward_f16x3_ref.py) against float64 torch on the GPU
tests' cases, the derived bound on it -- the bound the GPU tests assert first -- and the two exact properties the header states."""
import numpy as np
import pytest
import torch

import conv_forward_f16x3_ref as RF


def _run(c, x_scale=1.0, w_scale=1.0, bias=True, res=True, zero_x=False):
    x = c['x'][..., :c['cin']].contiguous().numpy() * np.float32(x_scale)
    if zero_x:
        x = np.zeros_like(x)
    b = c['bias'].numpy() if (bias and c['bias'] is not None) else None
    r = c['res'].numpy() if (res and c['res'] is not None) else None
    return RF.conv_forward3(x, c['w'].numpy() * np.float32(w_scale), b, r, c['stride'], c['pad'], c['relu'])


@pytest.mark.parametrize('name', sorted(RF.CASES))
def test_restatement_meets_the_bound(name):
    c = RF.make_case(name)
    got = _run(c)
    ref, S, E = RF.case_reference(c)
    err = (torch.from_numpy(got).double() - ref).abs()
    lim = RF.bound(c['k'] ** 2 * c['cin'], S, E, c['x'][..., :c['cin']].abs().max(), c['w'].abs().max())
    worst = float((err / lim).max())
    print('%s: max err / bound %.4f, normalised %.3e' % (name, worst, float(err.max() / ref.abs().max())))
    assert worst <= 1.0, (name, worst)
    assert float(err.max() / ref.abs().max()) < 1e-5     # fp32-class, nowhere near float16's 1e-3


def test_power_of_two_scaling_is_exact():
    """x * 2^-40 and w * 2^20 with no bias and no residual: y * 2^-20, bit for bit -- each scale follows its tensor."""
    for name in ('ragged_3x3', 'residual_relu'):
        c = RF.make_case(name)
        y = _run(c, bias=False, res=False)
        y2 = _run(c, x_scale=2.0 ** -40, w_scale=2.0 ** 20, bias=False, res=False)
        assert np.array_equal(y2, y * np.float32(2.0 ** -20)) and np.abs(y).max() > 0


def test_zero_input_gives_the_epilogue_alone():
    for name in ('ragged_3x3', 'residual_relu', 'single_k_tile'):
        c = RF.make_case(name)
        y = _run(c, zero_x=True)
        want = np.zeros_like(y)
        if c['bias'] is not None:
            want = want + c['bias'].numpy()
        if c['res'] is not None:
            want = want + c['res'].numpy()
        if c['relu']:
            want = np.maximum(want, np.float32(0))
        assert np.array_equal(y, want) and np.isfinite(y).all()


def test_an_element_beyond_the_float16_range():
    c = RF.make_case('ragged_3x3')
    c['x'][1, 3, 4, 5] = 1e5
    got = _run(c)
    ref, S, E = RF.case_reference(c)
    assert np.isfinite(got).all()
    lim = RF.bound(c['k'] ** 2 * c['cin'], S, E, 1e5, c['w'].abs().max())
    assert float(((torch.from_numpy(got).double() - ref).abs() / lim).max()) <= 1.0
