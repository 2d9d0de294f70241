"""CPU: the numpy restatements of tests/optim_ref.py against torch.optim.SGD and the reference's clip_gradient formula.

Three steps (the first creates the momentum buffers) over the reference's kinds of parameter group (trainval_net.py:158-168): a
weight (lr, weight decay), a bias (its own lr, weight decay 0) and an `uncert`-like tensor that is not clipped; the clip
coefficient is the reference's (net_utils.py:37-49), on both branches -- norm below clip_norm (coefficient 1) and above it."""
import numpy as np
import pytest
import torch

import optim_ref as R

LR, WD, MOMENTUM = 0.001, 0.0001, 0.9
GROUPS = [          # (shape, lr, weight decay, clipped)
    ((37, 5), LR, WD, True),
    ((37,), 2 * LR, 0.0, True),
    ((6,), LR, 0.0, False),
]
# float32 restatement against torch.optim.SGD in float32 on the CPU, max |difference| / max |torch| over three steps: measured
# 1.93e-8 (gradients below the clip) and 4.46e-8 (above it) -- torch's vectorised CPU kernels form a + alpha * b as one fused
# multiply-add, the restatement rounds the product first; the limit is twice the larger value
F32_VS_TORCH_LIMIT = 2 * 4.461e-08


def _data(seed, grad_scale):
    rng = np.random.RandomState(seed)
    ps = [rng.randn(*s).astype(np.float32) for s, _, _, _ in GROUPS]
    gs = [[(rng.randn(*s) * grad_scale).astype(np.float32) for s, _, _, _ in GROUPS] for _ in range(3)]
    return ps, gs


def _reference_clip_torch(grads, clip_norm):
    """net_utils.py:37-49 on float64 CPU tensors: the coefficient and the scaled gradients."""
    totalnorm = 0
    for g in grads:
        totalnorm += g.norm() ** 2
    totalnorm = float(np.sqrt(float(totalnorm)))
    norm = clip_norm / max(totalnorm, clip_norm)
    return totalnorm, norm, [g * norm for g in grads]


def _run(dtype, step_fn, grad_scale, clip_norm=10.0):
    """Three steps of torch.optim.SGD on clip_gradient's gradients, and of `step_fn` with the coefficient folded in."""
    ps, gs = _data(3, grad_scale)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    tp = [torch.tensor(p, dtype=tdt, requires_grad=True) for p in ps]
    opt = torch.optim.SGD([{'params': [t], 'lr': lr, 'weight_decay': wd} for t, (_, lr, wd, _) in zip(tp, GROUPS)], lr=LR, momentum=MOMENTUM)
    mine_p = [p.astype(dtype) for p in ps]
    mine_m = [None] * len(ps)
    coefs = []
    for it in range(3):
        g64 = [torch.tensor(g, dtype=torch.float64) for g in gs[it]]
        clipped = [g for g, grp in zip(g64, GROUPS) if grp[3]]
        total, coef, _ = _reference_clip_torch(clipped, clip_norm)
        t2, c2, _ = R.clip_gradient_f64([g.numpy() for g in clipped], clip_norm)
        assert abs(t2 - total) <= 1e-12 * total and abs(c2 - coef) <= 1e-15
        coefs.append(coef)
        use = np.float32(coef) if dtype == np.float32 else coef
        for t, g, grp in zip(tp, gs[it], GROUPS):
            gt = torch.tensor(g, dtype=tdt)
            t.grad = gt * torch.tensor(use, dtype=tdt) if grp[3] else gt        # clip_gradient's in-place scaling
        opt.step()
        for i, (g, (_, lr, wd, clip)) in enumerate(zip(gs[it], GROUPS)):
            mine_p[i], mine_m[i] = step_fn(mine_p[i], g.astype(dtype), mine_m[i], lr, wd, MOMENTUM, it == 0, use if clip else None)
    return tp, opt, mine_p, mine_m, coefs


@pytest.mark.parametrize('grad_scale, clips', [(0.01, False), (5.0, True)])
def test_float64_restatement_is_torch_sgd_after_clip_gradient(grad_scale, clips):
    tp, opt, mine_p, mine_m, coefs = _run(np.float64, R.sgd_step_f64, grad_scale)
    assert all((c < 1.0) == clips for c in coefs), coefs
    if not clips:
        assert all(c == 1.0 for c in coefs)
    for t, p, m in zip(tp, mine_p, mine_m):
        np.testing.assert_allclose(p, t.detach().numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(m, opt.state[t]['momentum_buffer'].numpy(), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize('grad_scale', [0.01, 5.0])
def test_float32_restatement_against_torch_sgd_float32(grad_scale):
    tp, opt, mine_p, mine_m, _ = _run(np.float32, R.sgd_step_f32, grad_scale)
    worst = 0.0
    for t, p, m in zip(tp, mine_p, mine_m):
        assert p.dtype == np.float32 and m.dtype == np.float32
        for got, ref in ((p, t.detach().numpy()), (m, opt.state[t]['momentum_buffer'].numpy())):
            worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max()))
    print('float32 restatement against torch.optim.SGD float32 (CPU): %.3e' % worst)
    assert worst <= F32_VS_TORCH_LIMIT


def test_momentum_zero_and_unclipped_paths():
    rng = np.random.RandomState(0)
    p, g = rng.randn(11).astype(np.float32), rng.randn(11).astype(np.float32)
    t = torch.tensor(p.astype(np.float64), requires_grad=True)
    opt = torch.optim.SGD([t], lr=0.05, momentum=0.0, weight_decay=0.01)
    t.grad = torch.tensor(g.astype(np.float64))
    opt.step()
    p64, m64 = R.sgd_step_f64(p, g, None, 0.05, 0.01, 0.0, True)
    assert m64 is None
    np.testing.assert_allclose(p64, t.detach().numpy(), rtol=1e-14)
    p32, m32 = R.sgd_step_f32(p, g, None, 0.05, 0.01, 0.0, True)
    assert m32 is None and p32.dtype == np.float32
    np.testing.assert_allclose(p32, p64, rtol=4 * 2.0 ** -24, atol=1e-7)


def test_clip_formula_and_norm_bound():
    rng = np.random.RandomState(1)
    grads = [rng.randn(5, 3), rng.randn(7)]
    total, coef, scaled = R.clip_gradient_f64(grads, 1.0)
    assert abs(total - R.norm_f64(grads)) <= 1e-14 * total
    assert total > 1.0 and abs(coef - 1.0 / total) <= 1e-15
    assert abs(R.norm_f64(scaled) - 1.0) <= 1e-12
    total, coef, scaled = R.clip_gradient_f64(grads, 100.0)
    assert coef == 1.0 and all(np.array_equal(a, b) for a, b in zip(scaled, grads))
    assert R.norm_bound() == 27 * 2.0 ** -24
