"""GPU: forward_precision / backward_precision 'auto' is nothing but autograd.choose_engine applied per call: a run with 'auto'
equals, bit for bit, the run in which every layer is forced to the engine the rule names for it -- on single layers through
autograd's public functions, and on the whole forward_train of tests/forward_train_ref.py's case with the decision list the run
recorded (autograd.record_engines) replayed as explicit precisions (autograd.replay_engines)."""
import pytest
import torch

import forward_train_ref as C

pytestmark = pytest.mark.gpu

GEN_SEED = 11
# (B, Cin, H, W, Cout, k, stride, pad): GEMMs on either side of the rule's thresholds
LAYERS = {'small': (1, 32, 5, 7, 24, 1, 1, 0), 'mid': (2, 64, 24, 40, 64, 3, 1, 1), 'large': (2, 64, 120, 200, 64, 3, 2, 1)}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def A(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import autograd
    return autograd


def _layer(A, dev, name, fp, bp):
    B, cin, H, W, cout, k, s, p = LAYERS[name]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, cin, H, W, generator=g).to(dev).requires_grad_(True)
    w = (torch.randn(cout, cin, k, k, generator=g) * 0.05).to(dev).requires_grad_(True)
    b = torch.randn(cout, generator=g).to(dev).requires_grad_(True)
    with A.record_engines() as log:
        y = A.conv2d(x, w, b, stride=s, padding=p, relu=True, forward_precision=fp, backward_precision=bp)
    y.backward(torch.randn(y.shape, generator=g).to(dev) * 1e-3)
    return (y, x.grad, w.grad, b.grad), log


@pytest.mark.parametrize('name', sorted(LAYERS))
@pytest.mark.parametrize('fp,bp', [('auto', 'auto'), ('auto', 'f32'), ('f32', 'auto'), ('f16x3', 'auto')])
def test_single_layer(A, dev, name, fp, bp):
    B, cin, H, W, cout, k, s, p = LAYERS[name]
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    M, K = B * OH * OW, k * k * cin
    want_f = A.choose_engine('forward', M, cout, K) if fp == 'auto' else fp
    want_b = A.choose_engine('backward', M, cout, K) if bp == 'auto' else bp
    got, log = _layer(A, dev, name, fp, bp)
    assert log == [(M, cout, K, want_f, want_b)]
    forced, _ = _layer(A, dev, name, want_f, want_b)
    for a, b in zip(got, forced):
        assert torch.equal(_bits(a), _bits(b))


def test_a_layer_resolved_to_fp32_scans_nothing(A, dev):
    from stereo_rcnn_amd import engine
    assert A.choose_engine('forward', 35, 24, 32) == 'f32' and A.choose_engine('backward', 35, 24, 32) == 'f32'
    engine.reset_f16x3_maxima()
    (y, *_), _ = _layer(A, dev, 'small', 'auto', 'auto')
    assert engine.F16X3_MAXIMA == {'scans': 0, 'reused': 0} and A._known_maximum(y) is None


@pytest.fixture(scope='module')
def env(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import training
    mp = pytest.MonkeyPatch()
    C.patch_cfg(mp)
    try:
        yield training, [t.to(dev) if i != 2 else t for i, t in enumerate(C.inputs())]
    finally:
        mp.undo()


def _train(training, batch, dev, fp, bp, replay=None):
    from stereo_rcnn_amd import autograd
    model = C.make_model(dev)
    run = lambda: training.forward_train(model, *batch, generator=torch.Generator(device=dev).manual_seed(GEN_SEED),
                                         forward_precision=fp, backward_precision=bp)
    with autograd.record_engines() as log:
        if replay is None:
            out = run()
        else:
            with autograd.replay_engines(replay):
                out = run()
    sum(out[8:14]).backward()
    return out[8:14], {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, log


@pytest.mark.parametrize('fp,bp', [('auto', 'auto'), ('auto', 'f32'), ('f32', 'auto')])
def test_forward_train_equals_the_forced_run(A, env, dev, fp, bp):
    training, batch = env
    losses, grads, engines = _train(training, batch, dev, fp, bp)
    assert len(engines) >= 60
    frozen = 0
    for M, N, K, f, b in engines:
        assert f in ('f32', 'f16x3') and b in ('f32', 'f16x3')
        if fp == 'auto' and f != A.choose_engine('forward', M, N, K):
            frozen += 1                                         # a frozen stage: without_graph() keeps it on fp32
            assert f == 'f32'
        assert b == (A.choose_engine('backward', M, N, K) if bp == 'auto' else bp)
        if fp != 'auto':
            assert f == fp
    assert frozen <= 9 + 1                                      # at most RCNN_layer1's ten convolutions (FIXED_BLOCKS = 1)
    # the same run with every layer forced: explicit precisions replace the keywords call by call
    losses2, grads2, engines2 = _train(training, batch, dev, 'f32', 'f32', replay=[(f, b) for _, _, _, f, b in engines])
    assert engines2 == engines
    for name, a, b in zip(C.LOSS_NAMES, losses, losses2):
        assert torch.equal(_bits(a), _bits(b)), name
    assert set(grads) == set(grads2)
    for k in grads:
        assert torch.equal(_bits(grads[k]), _bits(grads2[k])), k
