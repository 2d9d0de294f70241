"""GPU: forward_train / train_step with the BN fold and the weight re-layout on the device (TrainWeights.prepare(device_fold=True),
autograd.fold_all, csrc/train_fold.hip) on the case of tests/forward_train_ref.py (R-50, one 104 x 328 pair).  The kernels carry
the eager folds' arithmetic operation for operation, so everything is a bit-equality against TrainWeights.prepare(): the six losses
and EVERY parameter gradient, and the parameters after two steps."""
import pytest
import torch

import forward_train_ref as C

pytestmark = pytest.mark.gpu

GEN_SEED = 11


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def env(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import training
    mp = pytest.MonkeyPatch()
    C.patch_cfg(mp)
    try:
        yield training, [t.to(dev) if i != 2 else t for i, t in enumerate(C.inputs())]          # im_info stays on the host
    finally:
        mp.undo()


def _run(training, batch, dev, device_fold, fp, bp):
    from stereo_rcnn_amd import engine
    model = C.make_model(dev)
    weights = training.TrainWeights(model).prepare(device_fold=device_fold)
    engine.reset_f16x3_maxima()
    out = training.forward_train(model, *batch, generator=torch.Generator(device=dev).manual_seed(GEN_SEED), forward_precision=fp,
                                 backward_precision=bp, weights=weights)
    sum(out[8:14]).backward()
    return out[8:14], {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, model, weights


@pytest.mark.parametrize('fp,bp', [('f16x3', 'f16x3'), ('f32', 'f32')])
def test_losses_and_every_gradient_keep_their_bits(env, dev, fp, bp):
    training, batch = env
    losses0, grads0, model, weights0 = _run(training, batch, dev, False, fp, bp)
    losses1, grads1, _, weights1 = _run(training, batch, dev, True, fp, bp)
    assert len(weights1.layers) == len(weights0.layers) == len(weights1.specs())          # same keys, none twice
    for name, a, b in zip(C.LOSS_NAMES, losses0, losses1):
        assert torch.equal(_bits(a), _bits(b)), name
    assert set(grads0) == set(grads1) == set(training.trainable_parameters(model))
    for k in grads0:
        assert grads1[k].shape == grads0[k].shape and grads1[k].is_contiguous(), k
        assert torch.equal(_bits(grads0[k]), _bits(grads1[k])), k


def test_two_steps_equal_two_steps_with_prepared_weights_alone(env, dev):
    training, batch = env
    params = []
    for device_fold in (False, True):
        model = C.make_model(dev)
        uncert = torch.full((6,), -1.0, device=dev, requires_grad=True)
        opt = training.make_optimizer(model, uncert)
        for step in range(2):
            res = training.train_step(model, opt, uncert, batch, generator=torch.Generator(device=dev).manual_seed(GEN_SEED + step),
                                      forward_precision='f16x3', backward_precision='f16x3', prepared_weights=True,
                                      device_fold=device_fold)
        params.append(({k: p.detach().clone() for k, p in model.named_parameters()}, uncert.detach().clone(), res['loss']))
    (p0, u0, l0), (p1, u1, l1) = params
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(_bits(u0), _bits(u1))
    for k in p0:
        assert torch.equal(_bits(p0[k]), _bits(p1[k])), k
