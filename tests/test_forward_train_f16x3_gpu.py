"""GPU: training.forward_train / train_step with backward_precision='f16x3' (srcnn_conv2d_backward_f16x3 behind every layer that
has a graph) on the small case and the float64 graph of tests/forward_train_ref.py.  The forward is the exact-fp32 engine either
way, so outputs and losses are bit-equal to the default call; the gradients are compared with the float64 graph's, the default
path's error measured in the same run beside them (tests/train_f16x3_tolerances.py)."""
import pytest
import torch

import forward_train_ref as C
import train_f16x3_tolerances as TT
from tolerances import observe

pytestmark = pytest.mark.gpu


def _run(dev, model, bp):
    from stereo_rcnn_amd import training
    for p in model.parameters():
        p.grad = None
    taps = {}
    args = [t.to(dev) if i != 2 else t for i, t in enumerate(C.inputs())]          # im_info stays on the host
    out = training.forward_train(model, *args, generator=torch.Generator(device=dev).manual_seed(11), taps=taps, backward_precision=bp)
    sum(out[8:14]).backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return [o.detach().cpu() for o in out], grads, taps


@pytest.fixture(scope='module')
def case(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import training
    mp = pytest.MonkeyPatch()
    C.patch_cfg(mp)
    try:
        model = C.make_model(dev)
        out32, grads32, taps = _run(dev, model, 'f32')
        out16, grads16, _ = _run(dev, model, 'f16x3')
        trainable = set(training.trainable_parameters(model))
        state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        _, ref_grads = C.run_reference(state, taps, trainable=trainable)
    finally:
        mp.undo()
    return dict(out32=out32, out16=out16, grads32=grads32, grads16=grads16, trainable=trainable, ref_grads=ref_grads)


def test_the_forward_is_untouched(case):
    assert len(case['out16']) == 15
    for i, (a, b) in enumerate(zip(case['out16'], case['out32'])):
        assert torch.equal(a, b), 'output %d differs from the default call' % i


def test_gradient_set(case):
    assert set(case['grads16']) == case['trainable'] == set(case['grads32'])


def _norm_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def test_gradients_against_float64(case):
    bad, worst16, worst32 = [], 0.0, 0.0
    for name in sorted(case['trainable']):
        ref = case['ref_grads'][name]
        v16 = observe('train_f16x3_grad_' + name, _norm_err(case['grads16'][name], ref))
        v32 = observe('train_f16x3_fp32_grad_' + name, _norm_err(case['grads32'][name], ref))
        worst16, worst32 = max(worst16, v16), max(worst32, v32)
        assert torch.isfinite(case['grads16'][name]).all(), name
        lim = TT.LIMITS.get('train_f16x3_grad_' + name)
        if lim is not None and v16 > lim:
            bad.append('%s: %.3e beyond the measured limit %.3e' % (name, v16, lim))
    print('forward_train gradients vs float64: f16x3 worst %.3e, fp32 backward worst %.3e over %d parameters'
          % (worst16, worst32, len(case['trainable'])))
    observe('train_f16x3_grad_worst', worst16), observe('train_f16x3_fp32_grad_worst', worst32)
    assert not bad, bad
    # fp32-class, whatever the table holds: float16's own 2^-11 would show here as 5e-4
    assert worst16 <= TT.WORST_LIMIT, worst16


def test_train_step_runs(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import training
    mp = pytest.MonkeyPatch()
    C.patch_cfg(mp)
    try:
        model = C.make_model(dev)
        uncert = torch.full((6,), -1.0, device=dev, requires_grad=True)
        opt = training.make_optimizer(model, uncert)
        batch = [t.to(dev) if i != 2 else t for i, t in enumerate(C.inputs())]      # im_info on the CPU
        assert not batch[2].is_cuda
        res = training.train_step(model, opt, uncert, batch, clip_norm=10., generator=torch.Generator(device=dev).manual_seed(11),
                                  backward_precision='f16x3')
    finally:
        mp.undo()
    assert bool(torch.isfinite(res['grad_norm'])) and float(res['grad_norm']) > 0 and bool(torch.isfinite(res['loss']))
    for k, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), k


def test_unknown_backward_precision_is_refused(dev):
    from stereo_rcnn_amd import autograd
    with pytest.raises(ValueError):
        autograd.linear(torch.zeros(3, 64, device=dev), torch.zeros(5, 64, device=dev), backward_precision='bf16')
