"""GPU: forward_train / train_step with the f16x3 weights prepared once per step (training.TrainWeights, csrc/train_weights.hip) on
the case of tests/forward_train_ref.py (R-50, one 104 x 328 pair).  The prepared planes and words carry the bits the calls compute
for themselves, so everything is a bit-equality: the six losses and EVERY parameter gradient, and the parameters after two steps --
the second step fails for a TrainWeights that is not refreshed after the optimiser's raw-pointer update.  TrainWeights.specs() is
the one statement of the graph layers: it names every trainable parameter exactly once, and its two folds (autograd.fold_spec per
layer, autograd.fold_all for the list) agree bit for bit in both directions."""
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


def _run(training, batch, dev, prepared, fp='f16x3', bp='f16x3'):
    from stereo_rcnn_amd import engine
    model = C.make_model(dev)
    weights = training.TrainWeights(model).prepare() if prepared else None
    engine.reset_f16x3_maxima()
    out = training.forward_train(model, *batch, generator=torch.Generator(device=dev).manual_seed(GEN_SEED), forward_precision=fp,
                                 backward_precision=bp, weights=weights)
    sum(out[8:14]).backward()
    return out[8:14], {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, model, weights


@pytest.mark.parametrize('fp,bp', [('f16x3', 'f16x3'), ('f32', 'f16x3'), ('f16x3', 'f32')])
def test_losses_and_every_gradient_keep_their_bits(env, dev, fp, bp):
    training, batch = env
    losses0, grads0, model, _ = _run(training, batch, dev, False, fp, bp)
    losses1, grads1, _, weights = _run(training, batch, dev, True, fp, bp)
    assert len(weights.layers) == len(weights.specs())                     # no key twice
    for name, a, b in zip(C.LOSS_NAMES, losses0, losses1):
        assert torch.equal(_bits(a), _bits(b)), name
    assert set(grads0) == set(grads1) == set(training.trainable_parameters(model))
    for k in grads0:
        assert torch.equal(_bits(grads0[k]), _bits(grads1[k])), k


def test_two_steps_equal_two_steps_without(env, dev):
    training, batch = env
    params = []
    for prepared in (False, True):
        model = C.make_model(dev)
        uncert = torch.full((6,), -1.0, device=dev, requires_grad=True)
        opt = training.make_optimizer(model, uncert)
        for step in range(2):
            res = training.train_step(model, opt, uncert, batch, generator=torch.Generator(device=dev).manual_seed(GEN_SEED + step),
                                      forward_precision='f16x3', backward_precision='f16x3', prepared_weights=prepared)
        params.append(({k: p.detach().clone() for k, p in model.named_parameters()}, uncert.detach().clone(), res['loss']))
    (p0, u0, l0), (p1, u1, l1) = params
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(_bits(u0), _bits(u1))
    for k in p0:
        assert torch.equal(_bits(p0[k]), _bits(p1[k])), k


def test_the_layer_list_names_every_trainable_parameter_once(env, dev):
    training, _ = env
    model = C.make_model(dev)
    named = [t.data_ptr() for _, s in training.TrainWeights(model).specs() for part in s.parts for t in part if t is not None]
    assert len(set(named)) == len(named)
    assert sorted(named) == sorted(p.data_ptr() for p in training.trainable_parameters(model).values())


def test_the_eager_fold_and_the_device_fold_agree(env, dev):
    from stereo_rcnn_amd import autograd
    training, _ = env
    model = C.make_model(dev)
    named = training.TrainWeights(model).specs()
    specs = [s for _, s in named]
    folds, grads = [], []
    for folded in ([autograd.fold_spec(s) for s in specs], autograd.fold_all(specs)):
        g = torch.Generator(device=dev).manual_seed(GEN_SEED)
        total = 0.
        for w, b in folded:                             # one scalar whose gradient with respect to every folded element is its own
            total = total + (w * torch.randn(w.shape, device=dev, generator=g)).sum()
            if b is not None and b.requires_grad:       # (a bias that is a frozen BN's shift alone depends on no parameter)
                total = total + (b * torch.randn(b.shape, device=dev, generator=g)).sum()
        total.backward()
        folds.append(folded)
        grads.append({k: p.grad for k, p in model.named_parameters() if p.grad is not None})
        for p in model.parameters():
            p.grad = None
    for (key, s), (w0, b0), (w1, b1) in zip(named, *folds):
        assert tuple(w0.shape) == tuple(w1.shape) == tuple(s.shape) and torch.equal(_bits(w0), _bits(w1)), key
        assert (b0 is None) == (b1 is None) == (not s.has_b) and (b0 is None or torch.equal(_bits(b0), _bits(b1))), key
    assert set(grads[0]) == set(grads[1]) == set(training.trainable_parameters(model))
    for k in grads[0]:
        assert torch.equal(_bits(grads[0][k]), _bits(grads[1][k])), k
