"""GPU: training.forward_train / train_step with forward_precision='f16x3' (srcnn_conv2d_forward_f16x3 in front of every layer that
has a graph) on the small case and the float64 graph of tests/forward_train_ref.py, with both backward precisions.

The six losses and every parameter gradient are compared with the float64 graph built from the f16x3-forward run's OWN taps (its
ReLU masks, targets and dropout masks), the fp32 forward's error against its own float64 graph measured in the same run beside
them (tests/train_f16x3_forward_tolerances.py).  The discrete outcome of the proposal and target layers is compared with the
fp32-forward run of the same seed: the labels, weights and every other integer-valued tensor exactly, the proposals row for row
(same proposal in the same row; its coordinates, decoded from RPN deltas that differ by the split's rounding, within the project's
end-to-end proposal figure tolerances.PROPOSAL_MATCH_PX).  On the MI355X the selections came out equal, so equality is what is
asserted; the failure message lists the rows that differ."""
import pytest
import torch

import forward_train_ref as C
import tolerances
import train_f16x3_forward_tolerances as TT
from tolerances import observe

pytestmark = pytest.mark.gpu


def _run(dev, model, fp=None, bp=None):
    from stereo_rcnn_amd import training
    for p in model.parameters():
        p.grad = None
    taps = {}
    args = [t.to(dev) if i != 2 else t for i, t in enumerate(C.inputs())]          # im_info stays on the host
    kw = {}
    if fp is not None:
        kw['forward_precision'] = fp
    if bp is not None:
        kw['backward_precision'] = bp
    out = training.forward_train(model, *args, generator=torch.Generator(device=dev).manual_seed(11), taps=taps, **kw)
    sum(out[8:14]).backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return [o.detach().cpu() for o in out], grads, {k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in taps.items()}


@pytest.fixture(scope='module')
def case(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import training
    mp = pytest.MonkeyPatch()
    C.patch_cfg(mp)
    try:
        model = C.make_model(dev)
        r = {}
        r['f32'] = _run(dev, model, 'f32', 'f32')
        r['f16x3/f32'] = _run(dev, model, 'f16x3', 'f32')
        r['f16x3/f16x3'] = _run(dev, model, 'f16x3', 'f16x3')
        r['again'] = _run(dev, model, 'f16x3', 'f16x3')
        r['default'] = _run(dev, model)
        trainable = set(training.trainable_parameters(model))
        state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        ref16 = C.run_reference(state, r['f16x3/f32'][2], trainable=trainable)
        ref32 = C.run_reference(state, r['f32'][2], trainable=trainable)
    finally:
        mp.undo()
    return dict(r=r, trainable=trainable, ref16=ref16, ref32=ref32)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def test_the_two_precisions_are_independent(case):
    """The backward's precision does not reach the forward: outputs and taps of the two f16x3-forward runs are bit-equal, so one
    float64 graph serves both."""
    a, b = case['r']['f16x3/f32'], case['r']['f16x3/f16x3']
    assert len(a[0]) == 15 and _same(a[0], b[0])
    for k in a[2]:
        va, vb = a[2][k], b[2][k]
        assert _same(va, vb) if isinstance(va, list) else torch.equal(va, vb), k
    assert set(a[1]) == set(b[1]) == case['trainable']
    # ... and it is another forward than the fp32 engine's: the split is really running
    assert not torch.equal(a[2]['RPN_Conv.0'], case['r']['f32'][2]['RPN_Conv.0'])
    # the frozen part stays on the fp32 engine, bit for bit
    assert torch.equal(a[2]['RCNN_layer0'], case['r']['f32'][2]['RCNN_layer0'])
    assert torch.equal(a[2]['RCNN_layer1.0.2.out'], case['r']['f32'][2]['RCNN_layer1.0.2.out'])


def test_repeatable(case):
    a, b = case['r']['f16x3/f16x3'], case['r']['again']
    assert _same(a[0], b[0])
    assert all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_defaults_keep_their_bits_after_an_f16x3_run(case):
    a, b = case['r']['f32'], case['r']['default']
    assert _same(a[0], b[0])
    assert set(a[1]) == set(b[1]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def test_losses_against_float64(case):
    out16, out32 = case['r']['f16x3/f32'][0], case['r']['f32'][0]
    for i, name in enumerate(C.LOSS_NAMES):
        v16 = observe('train_f16x3_fwd_loss_' + name, _rel(out16[8 + i], case['ref16'][0][name]))
        v32 = observe('train_f16x3_fwd_fp32_loss_' + name, _rel(out32[8 + i], case['ref32'][0][name]))
        print('%s: f16x3 forward %.3e, fp32 forward %.3e' % (name, v16, v32))
        assert bool(torch.isfinite(out16[8 + i]))
        lim = TT.LIMITS.get('train_f16x3_fwd_loss_' + name)
        if lim is not None:
            assert v16 <= lim, (name, v16, lim)
        assert v16 <= TT.LOSS_CLASS, (name, v16)


@pytest.mark.parametrize('bp', ['f32', 'f16x3'])
def test_gradients_against_float64(case, bp):
    grads, bad, worst16, worst32 = case['r']['f16x3/' + bp][1], [], 0.0, 0.0
    assert set(grads) == case['trainable']
    for name in sorted(case['trainable']):
        key = 'train_f16x3_fwd_%s_grad_%s' % (bp, name)
        v16 = observe(key, _rel(grads[name], case['ref16'][1][name]))
        v32 = observe('train_f16x3_fwd_fp32_grad_' + name, _rel(case['r']['f32'][1][name], case['ref32'][1][name]))
        worst16, worst32 = max(worst16, v16), max(worst32, v32)
        assert torch.isfinite(grads[name]).all(), name
        lim = TT.LIMITS.get(key)
        if lim is not None and v16 > lim:
            bad.append('%s: %.3e beyond the measured limit %.3e' % (name, v16, lim))
    print('forward_train gradients vs float64, f16x3 forward, %s backward: worst %.3e; fp32 forward and backward worst %.3e over %d '
          'parameters' % (bp, worst16, worst32, len(case['trainable'])))
    observe('train_f16x3_fwd_%s_grad_worst' % bp, worst16), observe('train_f16x3_fwd_fp32_grad_worst', worst32)
    assert not bad, bad
    # fp32-class, whatever the table holds: float16's own 2^-11 would show here as 5e-4
    assert worst16 <= TT.GRAD_CLASS, worst16


def _rows_that_differ(a, b, tol):
    a2, b2 = a.reshape(-1, a.shape[-1]).double(), b.reshape(-1, b.shape[-1]).double()
    d = (a2 - b2).abs().amax(1)
    return [(int(i), float(d[i])) for i in torch.nonzero(d > tol).flatten()]


def test_selections_equal_the_fp32_forward_runs(case):
    t16, t32 = case['r']['f16x3/f32'][2], case['r']['f32'][2]
    px = tolerances.PROPOSAL_MATCH_PX
    report = []
    for k in ('rois_left', 'rois_right'):
        assert t16[k].shape == t32[k].shape
        rows = _rows_that_differ(t16[k], t32[k], px)
        observe('train_f16x3_fwd_%s_px' % k, float((t16[k].double() - t32[k].double()).abs().max()))
        if rows:
            report.append('%s: %d rows hold another proposal, first (row, px) %s' % (k, len(rows), rows[:8]))
    for k in ('anchor_targets', 'proposal_targets'):
        assert len(t16[k]) == len(t32[k])
        for i, (a, b) in enumerate(zip(t16[k], t32[k])):
            assert a.shape == b.shape, (k, i)
            integral = (not a.is_floating_point()) or bool((b == b.round()).all())
            if integral:                         # labels, weights, counts: the selection itself
                n = int((a != b).sum())
                if n:
                    report.append('%s[%d]: %d integer-valued entries differ, first at %s' % (k, i, n, torch.nonzero(a != b)[:8].tolist()))
            else:                                # targets computed from the selected boxes: the same entries are in use
                n = int(((a != 0) != (b != 0)).sum())
                if n:
                    report.append('%s[%d]: the non-zero pattern differs in %d entries' % (k, i, n))
            if k == 'proposal_targets' and i < 2:
                rows = _rows_that_differ(a, b, px)
                if rows:
                    report.append('%s[%d]: %d sampled rois differ, first (row, px) %s' % (k, i, len(rows), rows[:8]))
    assert torch.equal(case['r']['f16x3/f32'][0][14], case['r']['f32'][0][14]), 'rois_label differs'
    assert not report, report


def test_train_step_runs(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import training
    mp = pytest.MonkeyPatch()
    C.patch_cfg(mp)
    try:
        model = C.make_model(dev)
        before = model.RCNN_toplayer.weight.detach().clone()
        uncert = torch.full((6,), -1.0, device=dev, requires_grad=True)
        opt = training.make_optimizer(model, uncert)
        batch = [t.to(dev) if i != 2 else t for i, t in enumerate(C.inputs())]      # im_info on the CPU
        res = training.train_step(model, opt, uncert, batch, clip_norm=10., generator=torch.Generator(device=dev).manual_seed(11),
                                  forward_precision='f16x3')
    finally:
        mp.undo()
    assert bool(torch.isfinite(res['grad_norm'])) and float(res['grad_norm']) > 0 and bool(torch.isfinite(res['loss']))
    for name in training.LOSS_NAMES:
        assert bool(torch.isfinite(res[name])), name
    assert not torch.equal(before, model.RCNN_toplayer.weight.detach())
    for k, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), k
