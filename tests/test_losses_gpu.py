"""GPU: the fused loss kernels (srcnn_cross_entropy, srcnn_smooth_l1, their backwards) and the Python entry points over them
(stereo_rcnn_amd.model.stereo_rcnn.losses, model.utils.net_utils) against the float64 restatement tests/losses_ref.py on the same
float32 inputs.

Loss values are compared by relative error, gradients by the largest absolute error over the largest reference gradient
magnitude of the case; both against tests/loss_tolerances.py (twice the MI355X maxima) and, for values, its derived ceiling.
Op-level cases go through the C ABI with the gradient buffer pre-filled with NaN (every element must be written) and an upstream
gradient other than 1 on the device; every forward and backward runs twice and must repeat bit for bit.
"""
import math

import numpy as np
import pytest
import torch

import loss_tolerances as LT
import losses_ref as R
import tolerances

pytestmark = pytest.mark.gpu

CANARY = -12345.5
UPSTREAM = 1.7


@pytest.fixture(scope='module')
def m(dev):
    from stereo_rcnn_amd import _lib
    _lib.lib()
    return _lib


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_value(name, got, ref, elements, table):
    """relative error of a loss value against the table entry and the derived ceiling; a reference of exactly 0 must be met."""
    got, ref = float(got), float(ref)
    assert math.isfinite(got), got
    if ref == 0.0:
        assert got == 0.0
        return
    rel = tolerances.observe(name, abs(got - ref) / abs(ref))
    print('%s: %.3e (ceiling %.3e, %d elements)' % (name, rel, LT.value_ceiling(elements), elements))
    assert rel <= LT.value_ceiling(elements), (rel, LT.value_ceiling(elements))
    assert rel <= table, (rel, table)


def _check_grad(name, got, ref, table):
    got, ref = got.double(), ref.double()
    assert bool(torch.isfinite(got).all()), 'an element of the gradient was not written (NaN pre-fill) or is not finite'
    top = float(ref.abs().max()) if ref.numel() else 0.0
    if top == 0.0:
        assert float(got.abs().max()) == 0.0 if got.numel() else True
        return
    err = tolerances.observe(name, float((got - ref).abs().max()) / top)
    print('%s: %.3e' % (name, err))
    assert err <= table, (err, table)
    assert bool((got[ref == 0] == 0).all()), 'an element whose gradient is exactly 0 was written as non-zero'


# ------------------------------------------------------------------------------------------------------------ cross-entropy
def run_ce(m, dev, x, labels, weights=None, stride=None, gstride=None):
    """srcnn_cross_entropy + _backward on float32 x (rows, cols) laid out with the given row strides; twice, bit-equal.
    Returns (loss, norm, grad (rows, cols)) on the CPU."""
    L = m.lib()
    rows, cols = int(x.shape[0]), int(x.shape[1])
    stride, gstride = stride or cols, gstride or cols
    mode = m.CE_MEAN_KEPT if weights is None else m.CE_WEIGHTED
    buf = torch.full((max(rows, 1), stride), CANARY, dtype=torch.float32, device=dev)
    buf[:rows, :cols] = x.to(dev)
    lab = labels.to(torch.int32).to(dev)
    w = None if weights is None else weights.float().to(dev)
    up = torch.tensor([UPSTREAM], dtype=torch.float32, device=dev)
    ws_bytes = L.srcnn_loss_workspace_bytes(rows)
    outs = []
    for _ in range(2):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        loss = torch.full((1,), float('nan'), device=dev)
        norm = torch.full((1,), float('nan'), device=dev)
        grad = torch.full((max(rows, 1), gstride), float('nan'), device=dev)
        m.check(L.srcnn_cross_entropy(buf.data_ptr(), rows, cols, stride, m.ptr(lab), m.ptr(w), mode, loss.data_ptr(), norm.data_ptr(),
                                      ws.data_ptr(), ws_bytes, m.stream()))
        m.check(L.srcnn_cross_entropy_backward(buf.data_ptr(), rows, cols, stride, m.ptr(lab), m.ptr(w), mode, norm.data_ptr(),
                                               up.data_ptr(), grad.data_ptr(), gstride, m.stream()))
        outs.append((loss.cpu(), norm.cpu(), grad.cpu()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(_bits(a), _bits(b)), 'not repeatable bit for bit'
    host = buf.cpu()
    assert bool((host[:rows, cols:] == CANARY).all()) and torch.equal(host[:rows, :cols], x), 'the logits buffer was written'
    grad = outs[0][2][:rows]
    assert bool(torch.isnan(grad[:, cols:]).all()), 'the gap behind a gradient row was written'
    return float(outs[0][0]), float(outs[0][1]), grad[:, :cols].contiguous()


def ref_ce(x, labels, weights=None):
    x64 = x.double().clone().requires_grad_(True)
    loss = R.cross_entropy_rows(x64, labels, None if weights is None else weights.double())
    (loss * UPSTREAM).backward()
    return float(loss.detach()), x64.grad


def _ce_inputs(rows, cols, seed, ignore=True):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, cols, generator=g) * 2.0).float()
    y = torch.randint(0, cols, (rows,), generator=g)
    if ignore and rows >= 8:          # -1, cols and a large negative value: ignored, never an index
        y[1], y[rows // 2], y[rows - 2] = -1, cols, -2000000000
    return x, y


def _ce_case(m, dev, x, y, w=None, **strides):
    got, norm, grad = run_ce(m, dev, x, y, w, **strides)
    ref, rgrad = ref_ce(x, y, w)
    _check_value('loss_ce_value_rel', got, ref, x.numel(), LT.CE_VALUE_REL)
    _check_grad('loss_ce_grad', grad, rgrad, LT.CE_GRAD)
    return got, norm, grad


@pytest.mark.parametrize('rows,cols', [(1, 2), (63, 2), (65, 2), (257, 2), (300, 28), (300, 64), (300, 65), (128, 112)])
def test_cross_entropy_shapes(m, dev, rows, cols):
    x, y = _ce_inputs(rows, cols, 100 * rows + cols)
    _, norm, _ = _ce_case(m, dev, x, y)
    assert norm == float(((y >= 0) & (y < cols)).sum())            # the normaliser left on the device is the kept count


@pytest.mark.parametrize('cols', [2, 28])
def test_cross_entropy_more_than_two_workgroups(m, dev, cols):
    x, y = _ce_inputs(2 * m.LOSS_ROWS_PER_WG + 1, cols, 5 + cols)
    _ce_case(m, dev, x, y)


def test_cross_entropy_rpn_like_many_partials(m, dev):
    """200000 anchors x 2, about 0.5 % kept: nearly every row is a don't-care, 196 partials."""
    rows = 200000
    g = torch.Generator().manual_seed(77)
    x = torch.randn(rows, 2, generator=g).float()
    y = torch.full((rows,), -1, dtype=torch.long)
    kept = torch.randperm(rows, generator=g)[:1000]
    y[kept] = torch.randint(0, 2, (1000,), generator=g)
    _, norm, grad = _ce_case(m, dev, x, y)
    assert norm == 1000.0
    assert int((grad.abs().sum(1) != 0).sum()) <= 1000


@pytest.mark.parametrize('rows,cols,stride,gstride', [(65, 2, 3, 5), (65, 2, 4, 2), (300, 28, 37, 28), (130, 112, 168, 120)])
def test_cross_entropy_row_strides_leave_the_gaps_alone(m, dev, rows, cols, stride, gstride):
    x, y = _ce_inputs(rows, cols, rows + stride)
    _ce_case(m, dev, x, y, stride=stride, gstride=gstride)          # run_ce checks the canaries


@pytest.mark.parametrize('cols', [2, 28])
def test_cross_entropy_all_rows_ignored_is_exactly_zero(m, dev, cols):
    x, _ = _ce_inputs(300, cols, 9)
    y = torch.tensor([-1, cols, -2000000000] * 100)
    for w in (None, torch.ones(300)):
        got, norm, grad = run_ce(m, dev, x, y, w)
        assert got == 0.0 and norm == 0.0 and float(grad.abs().max()) == 0.0
    got, norm, _ = run_ce(m, dev, x[:0], y[:0])                     # rows == 0 succeeds and writes loss 0
    assert got == 0.0 and norm == 0.0


@pytest.mark.parametrize('rows,cols', [(257, 2), (300, 28), (128, 112)])
def test_cross_entropy_large_logits_stay_finite(m, dev, rows, cols):
    x, y = _ce_inputs(rows, cols, 31 + cols)
    x = (x * 5000.0).clamp(-1e4, 1e4)
    x[0, 0], x[0, cols - 1] = 1e4, -1e4
    got, _, grad = _ce_case(m, dev, x, y)
    assert math.isfinite(got) and bool(torch.isfinite(grad).all())


@pytest.mark.parametrize('cols', [2, 28, 112])
@pytest.mark.parametrize('total', [0.0, 0.5, 1.0, 37.25])
def test_cross_entropy_weighted_rule_on_the_device(m, dev, cols, total):
    """S if W < 1 else S / W, decided on the device: W = 0, 0.5, exactly 1.0 (divides) and 37.25 (all sums exact in float32)."""
    rows = 300
    x, y = _ce_inputs(rows, cols, 55 + cols)
    w = torch.zeros(rows)
    if total == 37.25:
        w[10:47], w[200] = 1.0, 0.25
    elif total:
        w[torch.arange(int(total / 0.25)) * 61 + 3] = 0.25
    assert float(w.double().sum()) == total
    got, norm, grad = _ce_case(m, dev, x, y, w)
    assert norm == total
    if total == 0.0:
        assert got == 0.0 and float(grad.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- smooth L1
def run_smooth_l1(m, dev, pred, target, w_in, w_out, sigma, divisor, selector, n_sel):
    """srcnn_smooth_l1 + _backward; weights (rows, D), per row (rows) or None; twice, bit-equal.  Returns (loss, grad) on the CPU."""
    L = m.lib()
    rows, D = int(target.shape[0]), int(target.shape[1])
    p, t = pred.float().contiguous().to(dev), target.float().contiguous().to(dev)
    wi = None if w_in is None else w_in.float().contiguous().to(dev)
    wo = None if w_out is None else w_out.float().contiguous().to(dev)
    sel = None if selector is None else selector.to(torch.int32).to(dev)
    up = torch.tensor([UPSTREAM], dtype=torch.float32, device=dev)
    ws_bytes = L.srcnn_loss_workspace_bytes(rows)
    outs = []
    for _ in range(2):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        loss = torch.full((1,), float('nan'), device=dev)
        norm = torch.full((1,), float('nan'), device=dev)
        grad = torch.full((rows, n_sel * D), float('nan'), device=dev)
        args = (p.data_ptr(), m.ptr(sel), n_sel, t.data_ptr(), m.ptr(wi), int(wi is not None and wi.dim() == 1), m.ptr(wo),
                int(wo is not None and wo.dim() == 1), rows, D, sigma)
        m.check(L.srcnn_smooth_l1(*args, divisor, loss.data_ptr(), norm.data_ptr(), ws.data_ptr(), ws_bytes, m.stream()))
        m.check(L.srcnn_smooth_l1_backward(*args, norm.data_ptr(), up.data_ptr(), grad.data_ptr(), m.stream()))
        outs.append((loss.cpu(), norm.cpu(), grad.cpu()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(_bits(a), _bits(b)), 'not repeatable bit for bit'
    assert float(outs[0][1]) == float(np.float32(divisor))
    return float(outs[0][0]), outs[0][2]


def ref_smooth_l1(pred, target, w_in, w_out, sigma, divisor, selector, n_sel):
    p64 = pred.double().clone().requires_grad_(True)
    loss = R.smooth_l1(p64, target, w_in, w_out, sigma=sigma, divisor=divisor, selector=selector, n_sel=n_sel)
    (loss * UPSTREAM).backward()
    return float(loss.detach()), p64.grad


@pytest.mark.parametrize('sigma', [1.0, 3.0])
@pytest.mark.parametrize('rows', [1, 65, 513])
@pytest.mark.parametrize('D', [5, 6])
def test_smooth_l1_value_and_gradient(m, dev, D, rows, sigma):
    thr = np.float32(1.0 / (sigma * sigma))
    planted = [float(thr), float(np.nextafter(thr, np.float32(0))), float(np.nextafter(thr, np.float32(2)))]   # at, below, above
    for weights in ('none', 'full', 'per_row'):
        for n_sel in (1, 2, 4):
            g = torch.Generator().manual_seed(1000 * D + rows + 7 * n_sel + len(weights))
            target = torch.randn(rows, D, generator=g).float()
            pred = (target.repeat(1, n_sel) + torch.randn(rows, n_sel * D, generator=g) * (1.5 / (sigma * sigma))).float()
            selector = None if (n_sel == 1 and weights == 'none') else torch.randint(0, n_sel, (rows,), generator=g)
            if selector is not None and rows >= 8:
                selector[3], selector[rows - 1] = -1, n_sel                   # out of range: the row contributes nothing
            if weights == 'none':
                w_in = w_out = None
            elif weights == 'full':
                w_in = (torch.rand(rows, D, generator=g) > 0.3).float() * (0.5 + torch.rand(rows, D, generator=g))
                w_out = torch.rand(rows, D, generator=g).float()
            else:
                w_in = (torch.rand(rows, generator=g) > 0.3).float()
                w_out = torch.rand(rows, generator=g).float()
            # row 0: differences exactly at, just below and just above the threshold, as float32 values (inside weight 1)
            s0 = 0 if selector is None else int(selector[0])
            target[0, :3] = 0.0
            pred[0, s0 * D:s0 * D + 3] = torch.tensor(planted)
            pred[0, s0 * D + 1] = -pred[0, s0 * D + 1]
            if w_in is not None:
                if w_in.dim() == 2:
                    w_in[0, :3] = 1.0
                else:
                    w_in[0] = 1.0
            divisor = float(rows) if D == 5 else 6.0 * max(rows // 32, 1)      # the host's divisor, of either kind
            got, grad = run_smooth_l1(m, dev, pred, target, w_in, w_out, sigma, divisor, selector, n_sel)
            ref, rgrad = ref_smooth_l1(pred, target, w_in, w_out, sigma, divisor, selector, n_sel)
            _check_value('loss_smooth_l1_value_rel', got, ref, rows * D, LT.SMOOTH_L1_VALUE_REL)
            _check_grad('loss_smooth_l1_grad', grad, rgrad, LT.SMOOTH_L1_GRAD)
            # unselected slices are exactly 0 (written, not left as the NaN pre-fill)
            chosen = torch.zeros(rows, n_sel, dtype=torch.bool)
            sel = torch.zeros(rows, dtype=torch.long) if selector is None else selector
            ok = (sel >= 0) & (sel < n_sel)
            chosen[ok.nonzero().view(-1), sel[ok]] = True
            assert bool((grad.view(rows, n_sel, D)[~chosen] == 0).all())
            # the planted elements: value and gradient are continuous across the threshold, so the three gradients are +-1 x scale
            row0 = grad.view(rows, n_sel, D)[0, s0, :3].double() * divisor / UPSTREAM
            if w_out is not None:
                wo0 = w_out[0, :3].double() if w_out.dim() == 2 else w_out[0].double()
                row0 = row0 / wo0 if float(torch.as_tensor(wo0).min()) > 0 else None
            if row0 is not None:
                assert float((row0 - torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64)).abs().max()) < 1e-6


def test_smooth_l1_more_than_two_workgroups(m, dev):
    rows, D = 2 * m.LOSS_ROWS_PER_WG + 1, 6
    g = torch.Generator().manual_seed(4)
    target = torch.randn(rows, D, generator=g).float()
    pred = (target.repeat(1, 2) + torch.randn(rows, 2 * D, generator=g) * 0.2).float()
    selector = torch.randint(-1, 3, (rows,), generator=g)
    w = (torch.rand(rows, generator=g) > 0.5).float()
    got, grad = run_smooth_l1(m, dev, pred, target, w, w, 3.0, 12.0, selector, 2)
    ref, rgrad = ref_smooth_l1(pred, target, w, w, 3.0, 12.0, selector, 2)
    _check_value('loss_smooth_l1_value_rel', got, ref, rows * D, LT.SMOOTH_L1_VALUE_REL)
    _check_grad('loss_smooth_l1_grad', grad, rgrad, LT.SMOOTH_L1_GRAD)
    got0, _ = run_smooth_l1(m, dev, pred[:0], target[:0], None, None, 1.0, 1.0, None, 1)      # rows == 0: loss 0
    assert got0 == 0.0


# ------------------------------------------------------------------------------------------------------------- module level
def _rpn_inputs(B, A, seed):
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(B, A, 2, generator=g).float()
    box = (torch.randn(B, A, 6, generator=g) * 0.3).float()
    label = torch.full((B, A), -1.0)
    pick = torch.randperm(B * A, generator=g)[:256]
    label.view(-1)[pick] = torch.randint(0, 2, (256,), generator=g).float()
    tl, tr = (torch.randn(B, A, 4, generator=g) * 0.3).float(), (torch.randn(B, A, 4, generator=g) * 0.3).float()
    inside = (label == 1).float()
    outside = (label >= 0).float() / 256.0
    return cls, box, label, tl, tr, inside, outside


def _rcnn_inputs(n, n_cls, G, seed):
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(0, n_cls, (n,), generator=g).float()
    fg = (label > 0).float()
    cls = torch.randn(n, n_cls, generator=g).float()
    bbox = (torch.randn(n, 6 * n_cls, generator=g) * 0.5).float()
    dim = (torch.randn(n, 5 * n_cls, generator=g) * 0.5).float()
    kpts = torch.randn(n, 6, G, generator=g).float()
    tl, tr = torch.randn(1, n, 4, generator=g).float(), torch.randn(1, n, 4, generator=g).float()
    tdim = torch.randn(1, n, 5, generator=g).float()
    klabel = torch.stack((torch.randint(0, 4 * G, (n,), generator=g), torch.randint(0, G, (n,), generator=g),
                          torch.randint(0, G, (n,), generator=g)), 1).view(1, n, 3)
    kweight = torch.stack((fg * (torch.rand(n, generator=g) > 0.5).float(), fg, fg * 0.0), 1).view(1, n, 3)   # W > 1, W > 1, W = 0
    ws_in = (fg.view(1, n, 1) * torch.ones(1, n, 4)).float()
    ws_out = ws_in * torch.rand(1, n, 4, generator=g)
    return [cls, bbox, dim, kpts], [label, tl, tr, tdim, klabel, kweight, ws_in, ws_out]


def _module_run(fn, preds, device, dtype):
    """One forward + backward of `fn(leaves)` (a tuple of scalar losses, weighted by distinct upstream gradients)."""
    leaves = [p.to(device=device, dtype=dtype).requires_grad_(True) for p in preds]
    out = fn(leaves)
    sum((0.7 + 0.3 * i) * l for i, l in enumerate(out)).backward()
    assert all(t.grad is not None and t.grad.shape == t.shape for t in leaves)
    return [l.detach().cpu() for l in out], [t.grad.cpu() for t in leaves]


def _module_case(fn_gpu, fn_ref, preds, dev, sizes):
    """twice on the device (bit-equal), once in float64 on the CPU; values and the gradient of every prediction tensor compared"""
    first, second = _module_run(fn_gpu, preds, dev, torch.float32), _module_run(fn_gpu, preds, dev, torch.float32)
    for a, b in zip(first[0] + first[1], second[0] + second[1]):
        assert torch.equal(_bits(a), _bits(b)), 'not repeatable bit for bit'
    ref = _module_run(fn_ref, preds, 'cpu', torch.float64)
    for a, b, size in zip(first[0], ref[0], sizes):
        _check_value('loss_module_value_rel', a, b, size, LT.MODULE_VALUE_REL)
    for a, b in zip(first[1], ref[1]):
        _check_grad('loss_module_grad', a, b, LT.MODULE_GRAD)


def test_rpn_losses_module(m, dev):
    from stereo_rcnn_amd.model.stereo_rcnn import losses
    B, A = 2, 1000
    cls, box, label, tl, tr, inside, outside = _rpn_inputs(B, A, 21)
    rest = [label, tl, tr, inside, outside]
    rest_dev = [t.to(dev) for t in rest]
    _module_case(lambda lv: losses.rpn_losses(lv[0], lv[1], *rest_dev), lambda lv: R.rpn_losses(lv[0], lv[1], *rest), [cls, box], dev,
                 [B * A * 2, B * A * 6])


def test_rcnn_losses_module_and_multi_task_loss(m, dev):
    from stereo_rcnn_amd.model.stereo_rcnn import losses
    n, n_cls, G = 128, 2, 28
    preds, targets = _rcnn_inputs(n, n_cls, G, 22)
    targets_dev = [t.to(dev) for t in targets]
    _module_case(lambda lv: losses.rcnn_losses(*lv, *targets_dev), lambda lv: R.rcnn_losses(*lv, *targets), preds, dev,
                 [n * n_cls, n * 6, n * 5, n * 6 * G])
    # multi_task_loss: the backward reaches every prediction tensor and the uncertainties
    cls, box, label, tl, tr, inside, outside = _rpn_inputs(1, 500, 23)
    rest = [label, tl, tr, inside, outside]
    rest_dev = [t.to(dev) for t in rest]
    uncert = torch.tensor([0.1, -0.2, 0.3, 0.0, -0.1, 0.2])

    def total(mod, rest_, targets_):
        return lambda lv: (mod.multi_task_loss(mod.rpn_losses(lv[0], lv[1], *rest_) + mod.rcnn_losses(*lv[2:6], *targets_), lv[6]),)

    everything = [cls, box] + preds + [uncert]
    got = _module_run(total(losses, rest_dev, targets_dev), everything, dev, torch.float32)
    ref = _module_run(total(R, rest, targets), everything, 'cpu', torch.float64)
    _check_value('loss_module_value_rel', got[0][0], ref[0][0], n * 6 * G, LT.MODULE_VALUE_REL)
    for a, b in zip(got[1], ref[1]):
        assert float(a.abs().max()) > 0
        _check_grad('loss_module_grad', a, b, LT.MODULE_GRAD)


def test_smooth_l1_loss_reference_signature(m, dev):
    """_smooth_l1_loss as the reference calls it: (B, A, 6) with per-anchor weights expanded to 6 columns (taken per row, no
    copy), sigma = 3, dim = [1] -> divided by B * 6; and the (n, D) default."""
    from stereo_rcnn_amd.model.utils import net_utils
    B, A = 2, 700
    g = torch.Generator().manual_seed(8)
    pred, tg = torch.randn(B, A, 6, generator=g).float(), torch.randn(B, A, 6, generator=g).float()
    wi, wo = (torch.rand(B, A, generator=g) > 0.5).float(), torch.rand(B, A, generator=g).float()
    leaf = pred.to(dev).requires_grad_(True)
    wi_d, wo_d = wi.to(dev).unsqueeze(2).expand(B, A, 6), wo.to(dev).unsqueeze(2).expand(B, A, 6)
    arg, per_row = net_utils._weight_arg(wi_d, leaf)
    assert per_row == 1 and arg.data_ptr() == wi_d.data_ptr() and tuple(arg.shape) == (B, A)       # no copy, not expanded
    loss = net_utils._smooth_l1_loss(leaf, tg.to(dev), wi_d, wo_d, sigma=3)
    loss.backward()
    r_leaf = pred.double().requires_grad_(True)
    ref = R.smooth_l1_loss(r_leaf, tg, wi.unsqueeze(2), wo.unsqueeze(2), sigma=3, dim=(1,))
    ref.backward()
    _check_value('loss_module_value_rel', loss.detach().cpu(), ref.detach(), B * A * 6, LT.MODULE_VALUE_REL)
    _check_grad('loss_module_grad', leaf.grad.cpu(), r_leaf.grad, LT.MODULE_GRAD)
    leaf2 = pred[0, :, :5].contiguous().to(dev).requires_grad_(True)
    loss2 = net_utils._smooth_l1_loss(leaf2, tg[0, :, :5].contiguous().to(dev))
    ref2 = R.smooth_l1_loss(pred[0, :, :5], tg[0, :, :5])
    _check_value('loss_module_value_rel', loss2.detach().cpu(), ref2, A * 5, LT.MODULE_VALUE_REL)


def test_cpu_tensors_raise(m):
    from stereo_rcnn_amd.model.stereo_rcnn import losses
    from stereo_rcnn_amd.model.utils import net_utils
    with pytest.raises(NotImplementedError):
        losses.cross_entropy_rows(torch.zeros(4, 2), torch.zeros(4, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        net_utils._smooth_l1_loss(torch.zeros(4, 6), torch.zeros(4, 6))
    preds, targets = _rcnn_inputs(8, 2, 28, 1)
    with pytest.raises(NotImplementedError):
        losses.rcnn_losses(*preds, *targets)
