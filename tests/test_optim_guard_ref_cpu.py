"""CPU: the restatement of the guarded optimiser pair (tests/optim_guard_ref.py) against the restatement of the plain one
(tests/optim_ref.py) and against its own definition: with grad_scale 1 and finite gradients it IS the plain step, bit for bit;
a skipped step changes nothing; a skipped first step leaves zero buffers after which a normal step is the first step."""
import numpy as np
import pytest

import optim_guard_ref as G
import optim_ref as R

F32 = np.float32
SIZES = (1, 3, 4, 255, 4095, 4096, 4097, 2 * 4096 + 5)


def _u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _data(seed, n):
    rng = np.random.RandomState(seed)
    return tuple(rng.randn(n).astype(F32) for _ in range(3))


@pytest.mark.parametrize('momentum,first', [(0.9, True), (0.9, False), (0.0, False)])
@pytest.mark.parametrize('wd', [0.0, 1e-3])
@pytest.mark.parametrize('coef', [None, 0.37])
def test_scale_one_is_the_plain_step(momentum, first, wd, coef):
    for n in SIZES:
        p, g, m = _data(n, n)
        want_p, want_m = R.sgd_step_f32(p, g, m, 0.01, wd, momentum, first, coef)
        got_p, got_m = G.sgd_step_guarded_f32(p, g, m, 0.01, wd, momentum, first, 1.0, F32(1.0), coef)
        assert np.array_equal(_u32(got_p), _u32(want_p))
        assert (got_m is None and want_m is None) or np.array_equal(_u32(got_m), _u32(want_m))


def test_the_scale_is_one_rounding_applied_first():
    p, g, m = _data(5, 1000)
    s = F32(1.0 / 3.0)
    want_p, want_m = R.sgd_step_f32(p, (g * s).astype(F32), m, 0.01, 1e-3, 0.9, False, 0.37)
    got_p, got_m = G.sgd_step_guarded_f32(p, g, m, 0.01, 1e-3, 0.9, False, 1.0 / 3.0, F32(1.0), 0.37)
    assert np.array_equal(_u32(got_p), _u32(want_p)) and np.array_equal(_u32(got_m), _u32(want_m))
    # not the same as scaling the coefficient: two roundings in another order
    other_p, _ = R.sgd_step_f32(p, g, m, 0.01, 1e-3, 0.9, False, F32(0.37) * s)
    assert not np.array_equal(_u32(got_p), _u32(other_p))


def test_a_skipped_step_changes_nothing():
    p, g, m = _data(6, 300)
    g[17] = np.inf
    got_p, got_m = G.sgd_step_guarded_f32(p, g, m, 0.01, 1e-3, 0.9, False, 0.5, F32(0.0), 0.37)
    assert np.array_equal(_u32(got_p), _u32(p)) and np.array_equal(_u32(got_m), _u32(m))
    got_p, got_m = G.sgd_step_guarded_f32(p, g, None, 0.01, 1e-3, 0.0, False, 0.5, F32(0.0), 0.37)
    assert np.array_equal(_u32(got_p), _u32(p)) and got_m is None


def test_a_skipped_first_step_then_a_normal_step_is_a_first_step():
    p, g, garbage = _data(7, 4097)
    bad = g.copy()
    bad[0] = np.nan
    p1, m1 = G.sgd_step_guarded_f32(p, bad, garbage, 0.01, 1e-3, 0.9, True, 1.0, F32(0.0), 0.37)
    assert np.array_equal(_u32(p1), _u32(p)) and np.array_equal(_u32(m1), np.zeros(p.size, np.uint32))
    p2, m2 = G.sgd_step_guarded_f32(p1, g, m1, 0.01, 1e-3, 0.9, False, 1.0, F32(1.0), 0.37)
    want_p, want_m = R.sgd_step_f32(p, g, None, 0.01, 1e-3, 0.9, True, 0.37)
    assert np.array_equal(_u32(p2), _u32(want_p))
    # momentum * (+0) + d: d's bits, but for d = -0, which becomes +0 (equal as numbers; p - lr * m has the same bits either way)
    assert np.array_equal(m2, want_m) and np.array_equal(_u32(m2)[want_m != 0], _u32(want_m)[want_m != 0])


def test_norm_against_float64_and_its_three_words():
    rng = np.random.RandomState(11)
    grads = [rng.randn(n).astype(F32) for n in SIZES + (0,)]
    for scale in (1.0, 0.5, 0.25, 1.0 / 3.0):
        norm, coef, ok = G.grad_norm_guarded_f32(grads, 10.0, scale)
        want = R.norm_f64([(g * F32(scale)).astype(F32) for g in grads])
        assert abs(float(norm) - want) / want <= R.norm_bound()
        assert ok == 1 and coef == F32(10.0) / max(norm, F32(10.0)) and coef < 1
        assert all(v.dtype == F32 for v in (norm, coef, ok))
    one, _, _ = G.grad_norm_guarded_f32(grads, 10.0, 1.0)
    half, _, _ = G.grad_norm_guarded_f32(grads, 10.0, 0.5)
    assert half == one * F32(0.5)                       # a power of two scales every term exactly (no subnormals here)
    norm, coef, ok = G.grad_norm_guarded_f32(grads, float('inf'), 1.0)
    assert norm == one and coef == 1 and ok == 1
    norm, coef, ok = G.grad_norm_guarded_f32([np.zeros(0, F32)], 10.0, 1.0)
    assert norm == 0 and coef == 1 and ok == 1


@pytest.mark.parametrize('value,where', [(np.inf, -1), (-np.inf, 5000), (np.nan, 0)])
def test_norm_of_a_non_finite_gradient(value, where):
    rng = np.random.RandomState(12)
    grads = [rng.randn(n).astype(F32) for n in (7, 2 * 4096 + 5, 100)]
    grads[1][where] = value
    norm, coef, ok = G.grad_norm_guarded_f32(grads, 10.0, 0.5)
    assert ok == 0 and not np.isfinite(norm)
    assert (coef == 0) if np.isinf(value) else (coef == 1)     # clip / inf, and max(NaN, clip) = clip as the kernel's `>` picks it


def test_norm_of_finite_gradients_whose_squares_overflow():
    g = np.zeros(4097, F32)
    g[3] = g[4096] = 3e19
    norm, coef, ok = G.grad_norm_guarded_f32([g], 10.0, 1.0)
    assert np.isinf(norm) and coef == 0 and ok == 0
    norm, coef, ok = G.grad_norm_guarded_f32([g], 10.0, 0.25)          # (0.75e19)^2 = 5.6e37 fits
    assert ok == 1 and abs(float(norm) - 0.75e19 * 2 ** 0.5) / float(norm) < 1e-6
