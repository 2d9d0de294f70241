"""CPU: pins tests/losses_ref.py, the float64 restatement the loss kernels are compared with (tests/test_losses_gpu.py), against
torch.nn.functional.cross_entropy, closed-form smooth-L1 values at hand-picked points and torch.autograd.gradcheck."""
import math

import torch
import torch.nn.functional as F

import losses_ref as R


def _logits(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, generator=g, dtype=torch.float64) * 3.0


def test_cross_entropy_mean_over_kept_rows_is_torch_cross_entropy():
    for rows, cols in ((7, 2), (40, 28), (9, 112)):
        x = _logits(rows, cols, rows)
        y = torch.randint(0, cols, (rows,), generator=torch.Generator().manual_seed(1))
        assert abs(float(R.cross_entropy_rows(x, y)) - float(F.cross_entropy(x, y))) < 1e-12
        # ignored labels: -1, cols and a large negative value drop their rows, exactly as selecting the others first
        y2 = y.clone()
        y2[0], y2[rows // 2], y2[rows - 1] = -1, cols, -2000000000
        keep = torch.tensor([i for i in range(rows) if i not in (0, rows // 2, rows - 1)])
        assert abs(float(R.cross_entropy_rows(x, y2)) - float(F.cross_entropy(x[keep], y[keep]))) < 1e-12


def test_cross_entropy_weighted_rule_and_empty_selection():
    x = _logits(12, 5, 3)
    y = torch.randint(0, 5, (12,), generator=torch.Generator().manual_seed(2))
    per_row = F.cross_entropy(x, y, reduction='none')
    for total in (0.0, 0.5, 1.0, 37.25):
        w = torch.zeros(12, dtype=torch.float64)
        if total:
            w[1], w[4], w[9] = total / 4, total / 4, total / 2
        s = float((per_row * w).sum())
        want = s if total < 1 else s / total           # exactly 1.0 divides
        assert abs(float(R.cross_entropy_rows(x, y, w)) - want) < 1e-12
    none = torch.full((12,), -1, dtype=torch.long)
    assert float(R.cross_entropy_rows(x, none)) == 0.0 and float(R.cross_entropy_rows(x, none, torch.ones(12))) == 0.0


def test_cross_entropy_is_stable_for_large_logits():
    x = _logits(6, 4, 5) * 1e4
    y = torch.tensor([0, 1, 2, 3, 0, 1])
    v = float(R.cross_entropy_rows(x, y))
    assert math.isfinite(v) and abs(v - float(F.cross_entropy(x, y))) <= 1e-9 * abs(v)


def _one(d, sigma):
    """smooth L1 of a single difference d."""
    return float(R.smooth_l1(torch.tensor([[d]], dtype=torch.float64), torch.zeros(1, 1, dtype=torch.float64), sigma=sigma, divisor=1))


def test_smooth_l1_closed_form_points():
    for sigma in (1.0, 3.0):
        s2 = sigma * sigma
        t = 1.0 / s2
        assert _one(0.0, sigma) == 0.0
        # exactly at the threshold: `<` is strict, so the LINEAR branch, |d| - 0.5 / sigma^2 (= the quadratic value there)
        assert _one(t, sigma) == t - 0.5 / s2 and _one(-t, sigma) == t - 0.5 / s2
        inside = t * (1.0 - 2.0 ** -20)
        assert _one(inside, sigma) == 0.5 * s2 * inside * inside         # just inside: quadratic
        assert abs(_one(inside, sigma) - _one(t, sigma)) < 1e-5 * t      # continuous across the threshold
        assert _one(5.0, sigma) == 5.0 - 0.5 / s2
    # weights: d = w_in (p - t), value times w_out; the divisor divides the sum
    p, tg = torch.tensor([[2.0, 0.25]], dtype=torch.float64), torch.tensor([[0.0, 0.0]], dtype=torch.float64)
    w_in, w_out = torch.tensor([[0.5, 2.0]], dtype=torch.float64), torch.tensor([[3.0, 0.25]], dtype=torch.float64)
    want = (3.0 * (1.0 - 0.5) + 0.25 * 0.5 * 0.25) / 4.0
    assert abs(float(R.smooth_l1(p, tg, w_in, w_out, sigma=1.0, divisor=4.0)) - want) < 1e-15


def test_smooth_l1_selector_is_gather_and_drops_out_of_range_rows():
    g = torch.Generator().manual_seed(7)
    pred = torch.randn(6, 3 * 5, generator=g, dtype=torch.float64)
    tg = torch.randn(6, 5, generator=g, dtype=torch.float64)
    sel = torch.tensor([0, 2, 1, 3, -1, 2])
    rows = [0, 1, 2, 5]
    picked = torch.stack([pred[r].view(3, 5)[int(sel[r])] for r in rows])
    want = float(R.smooth_l1(picked, tg[rows], divisor=6))
    assert abs(float(R.smooth_l1(pred, tg, selector=sel, n_sel=3)) - want) < 1e-15


def test_divisor_quirk_of_the_rpn_box_loss():
    """(B, A, 6) summed over dim=[1] leaves (B, 6) for .mean(): the sum is divided by B * 6, not by B * A."""
    B, A = 2, 11
    g = torch.Generator().manual_seed(9)
    pred = torch.randn(B, A, 6, generator=g, dtype=torch.float64)
    tg = torch.randn(B, A, 6, generator=g, dtype=torch.float64)
    total = float(R.smooth_l1(pred.view(-1, 6), tg.view(-1, 6), sigma=3, divisor=1))
    assert abs(float(R.smooth_l1_loss(pred, tg, sigma=3, dim=(1,))) - total / (B * 6)) < 1e-14
    tl, tr = tg[:, :, :4], torch.stack((tg[:, :, 4], tg[:, :, 0], tg[:, :, 5], tg[:, :, 1]), 2)
    ones = torch.ones(B, A, dtype=torch.float64)
    label = torch.randint(-1, 2, (B, A), generator=g)
    cls = torch.randn(B, A, 2, generator=g, dtype=torch.float64)
    loss_cls, loss_box = R.rpn_losses(cls, pred, label, tl, tr, ones, ones)
    assert abs(float(loss_box) - total / (B * 6)) < 1e-14
    keep = label.view(-1) >= 0
    assert abs(float(loss_cls) - float(F.cross_entropy(cls.view(-1, 2)[keep], label.view(-1)[keep]))) < 1e-12
    # (n, 6) with dim=[1]: the plain per-roi mean
    assert abs(float(R.smooth_l1_loss(pred[0], tg[0])) - float(R.smooth_l1(pred[0], tg[0], divisor=A))) < 1e-14


def test_gradcheck_of_the_restatement():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(9, 6, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.tensor([0, 5, -1, 3, 6, 2, 2, -7, 1])
    w = torch.rand(9, generator=g, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda t: R.cross_entropy_rows(t, y), (x,))
    assert torch.autograd.gradcheck(lambda t: R.cross_entropy_rows(t, y, w), (x,))
    assert torch.autograd.gradcheck(lambda t: R.cross_entropy_rows(t, y, w * 0.01), (x,))
    # smooth L1 away from the kink of the second derivative (the value and the gradient are continuous, gradcheck only needs
    # the finite difference to stay on one branch)
    tg = torch.randn(7, 5, generator=g, dtype=torch.float64)
    d = torch.tensor([0.05, -0.3, 0.6, -0.9, 1.4, -2.5, 3.0], dtype=torch.float64)
    pred = torch.zeros(7, 2, 5, dtype=torch.float64)
    pred[:, 0], pred[:, 1] = tg + d.view(-1, 1), tg - 2.0 * d.view(-1, 1)
    pred = pred.view(7, 10).clone().requires_grad_(True)
    sel = torch.tensor([0, 1, 1, 0, 2, 0, 1])
    w_in = torch.rand(7, 5, generator=g, dtype=torch.float64) * 0.2 + 0.9
    w_out = torch.rand(7, 1, generator=g, dtype=torch.float64)
    for sigma in (1.0, 3.0):
        assert torch.autograd.gradcheck(lambda t: R.smooth_l1(t, tg, w_in, w_out, sigma=sigma, selector=sel, n_sel=2), (pred,))


def test_multi_task_loss():
    losses = [torch.tensor(float(i + 1), dtype=torch.float64) for i in range(6)]
    u = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 0.25], dtype=torch.float64)
    want = sum((i + 1) * math.exp(-float(u[i])) + float(u[i]) for i in range(6))
    assert abs(float(R.multi_task_loss(losses, u)) - want) < 1e-12
