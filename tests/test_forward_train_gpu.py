"""GPU: stereo_rcnn_amd.training.forward_train -- one call, ten outputs with six live losses, backward() of their sum -- against
the same graph in float64 on the CPU (tests/forward_train_ref.py), which takes every discrete decision (rois, target-layer
outputs, dropout masks, ReLU masks) from the product's taps.

Bounds.  Every tensor is compared as max |difference| / max |reference|.  For scale the same graph runs in float32 eager torch
on the CPU against the float64 reference: a product tensor more than ten times further from float64 than float32 eager torch is
a defect (with a floor of 64 u for tensors float32 eager happens to hit exactly).  tests/train_tolerances.py holds twice the
measured value of every tensor on top.
"""
import pytest
import torch

import forward_train_ref as C
import train_tolerances as TT
from tolerances import observe

pytestmark = pytest.mark.gpu

OUTPUTS = {'cls_prob': 2, 'bbox_pred': 3, 'dim_orien_pred': 4, 'kpts_prob': 5, 'left_border_prob': 6, 'right_border_prob': 7}
FLOOR = 64 * 2.0 ** -24


@pytest.fixture(scope='module')
def case(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import training
    mp = pytest.MonkeyPatch()
    C.patch_cfg(mp)
    try:
        model = C.make_model(dev)
        out, grads, taps = C.run_product(dev, model=model)
        out2, grads2, _ = C.run_product(dev, model=model)
        trainable = set(training.trainable_parameters(model))
        state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        ref_out, ref_grads = C.run_reference(state, taps, trainable=trainable)
        f32_out, f32_grads = C.run_reference(state, taps, dtype=torch.float32, trainable=trainable)
        requires = {k: p.requires_grad for k, p in model.named_parameters()}
    finally:
        mp.undo()
    return dict(out=out, grads=grads, out2=out2, grads2=grads2, taps=taps, trainable=trainable, ref_out=ref_out, ref_grads=ref_grads,
                f32_out=f32_out, f32_grads=f32_grads, requires=requires)


def _norm_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def _check(name, got, ref, f32):
    v, scale = observe('forward_train_' + name, _norm_err(got, ref)), _norm_err(f32, ref)
    print('forward_train %s: normalised error %.3e (float32 eager %.3e)' % (name, v, scale))
    bad = []
    if v > 10 * max(scale, FLOOR):
        bad.append('%s: %.3e beyond ten times float32 eager (%.3e)' % (name, v, scale))
    lim = TT.LIMITS.get('forward_train_' + name)
    if lim is not None and v > lim:
        bad.append('%s: %.3e beyond the measured limit %.3e' % (name, v, lim))
    return bad


def test_the_case_exercises_the_losses(case):
    labels, anchor_labels = case['out'][14], case['taps']['anchor_targets'][0]
    assert int((labels > 0).sum()) >= 1 and int((labels == 0).sum()) >= 1
    assert int((anchor_labels == 1).sum()) >= 1 and int((anchor_labels == 0).sum()) >= 1
    assert int(case['taps']['proposal_status'].sum()) == 0
    for name in ('dropout1', 'dropout2'):
        keep = float(case['taps'][name].float().mean())
        assert 0.7 < keep < 0.9, (name, keep)
    assert case['out'][0].shape == (1, 16, 5) and case['out'][2].shape == (1, 16, 2) and case['out'][5].shape == (16, 112)


def test_losses_and_outputs_against_float64(case):
    bad = []
    for i, name in enumerate(C.LOSS_NAMES):
        got = case['out'][8 + i]
        assert got.dim() == 0 and bool(torch.isfinite(got)) and float(case['ref_out'][name]) > 0, name
        bad += _check(name, got, case['ref_out'][name], case['f32_out'][name])
    for name, i in OUTPUTS.items():
        got = case['out'][i]
        bad += _check(name, got.reshape(case['ref_out'][name].shape), case['ref_out'][name], case['f32_out'][name])
    assert not bad, bad


def test_gradient_set_is_the_references(case):
    import re
    got = set(case['grads'])
    assert got == case['trainable'] == set(case['ref_grads'])
    assert {k for k, r in case['requires'].items() if r} == got
    # resnet.py:288-309 spelled out: no stem, no first stage, no BatchNorm; everything else
    assert not any(k.startswith(('RCNN_layer0.', 'RCNN_layer1.')) or re.search(r'\.bn\d\.|downsample\.1\.', k) for k in got)
    for k in ('RCNN_layer2.0.0.conv1.weight', 'RCNN_layer4.0.2.conv3.weight', 'RCNN_layer3.0.0.downsample.0.weight', 'RCNN_toplayer.bias',
              'RCNN_smooth3.weight', 'RCNN_latlayer1.weight', 'RCNN_rpn.RPN_Conv.weight', 'RCNN_rpn.RPN_cls_score.bias',
              'RCNN_rpn.RPN_bbox_pred_left_right.weight', 'RCNN_top.0.weight', 'RCNN_top.3.bias', 'RCNN_kpts.0.weight',
              'RCNN_kpts.12.weight', 'RCNN_kpts.12.bias', 'kpts_class.weight', 'RCNN_cls_score.weight', 'RCNN_bbox_pred.bias',
              'RCNN_dim_orien_pred.weight'):
        assert k in got, k


def test_gradients_against_float64(case):
    bad = []
    for name in sorted(case['ref_grads']):
        got, ref = case['grads'][name], case['ref_grads'][name]
        assert got.shape == ref.shape and bool(torch.isfinite(got).all()), name
        if float(ref.abs().max()) == 0:
            assert float(got.abs().max()) == 0, name
            continue
        assert float(got.abs().max()) > 0, name
        bad += _check('grad.' + name, got, ref, case['f32_grads'][name])
    assert not bad, bad


def test_second_call_is_bit_equal(case):
    for i in range(8, 14):
        assert torch.equal(case['out'][i], case['out2'][i]), C.LOSS_NAMES[i - 8]
    assert set(case['grads']) == set(case['grads2'])
    for k in case['grads']:
        assert torch.equal(case['grads'][k], case['grads2'][k]), k


def test_a_pre_nms_count_beyond_the_proposal_kernel_is_refused(dev, monkeypatch):
    """The reference's default cfg.TRAIN.RPN_PRE_NMS_TOP_N (12000) on the case's 8604 anchors: refused, not lowered."""
    from stereo_rcnn_amd import training
    from stereo_rcnn_amd.model.utils.config import cfg
    C.patch_cfg(monkeypatch)
    monkeypatch.setattr(cfg.TRAIN, 'RPN_PRE_NMS_TOP_N', 12000)
    args = [t.to(dev) if i != 2 else t for i, t in enumerate(C.inputs())]
    with pytest.raises(ValueError, match='RPN_PRE_NMS_TOP_N'):
        training.forward_train(C.make_model(dev), *args, generator=torch.Generator(device=dev).manual_seed(1))
