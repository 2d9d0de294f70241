"""GPU: training.forward_train with reuse_maxima on the small case of tests/forward_train_ref.py, set up as
tests/test_forward_train_f16x3_forward_gpu.py sets it up.  Handing a layer's max |y| to its consumers changes who finds a maximum,
never the maximum: all fifteen outputs, the taps and every parameter gradient are bit-equal with and without it, while
engine.F16X3_MAXIMA shows that passes over activations were really skipped."""
import pytest
import torch

import forward_train_ref as C

pytestmark = pytest.mark.gpu


def _run(dev, model, engine, **kw):
    from stereo_rcnn_amd import training
    for p in model.parameters():
        p.grad = None
    taps = {}
    args = [t.to(dev) if i != 2 else t for i, t in enumerate(C.inputs())]          # im_info stays on the host
    engine.reset_f16x3_maxima()
    out = training.forward_train(model, *args, generator=torch.Generator(device=dev).manual_seed(11), taps=taps, **kw)
    sum(out[8:14]).backward()
    torch.cuda.synchronize()
    counters = dict(engine.F16X3_MAXIMA)
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return ([o.detach().cpu() for o in out], grads,
            {k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in taps.items()}, counters)


@pytest.fixture(scope='module')
def case(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import engine
    mp = pytest.MonkeyPatch()
    C.patch_cfg(mp)
    try:
        model = C.make_model(dev)
        r = {}
        for fp, bp in (('f16x3', 'f16x3'), ('f32', 'f16x3'), ('f32', 'f32')):
            for reuse in (True, False):
                r[fp, bp, reuse] = _run(dev, model, engine, forward_precision=fp, backward_precision=bp, reuse_maxima=reuse)
        r['default'] = _run(dev, model, engine)
    finally:
        mp.undo()
    return r


def _bits_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def _assert_same_run(a, b):
    assert len(a[0]) == len(b[0]) == 15
    for i, (p, q) in enumerate(zip(a[0], b[0])):
        assert _bits_equal(p, q), 'output %d' % i
    assert set(a[2]) == set(b[2])
    for k in a[2]:
        va, vb = a[2][k], b[2][k]
        if isinstance(va, list):
            assert len(va) == len(vb) and all(_bits_equal(p, q) for p, q in zip(va, vb)), k
        else:
            assert _bits_equal(va, vb), k
    assert set(a[1]) == set(b[1]) and len(a[1]) > 0
    for k in a[1]:
        assert _bits_equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize('fp,bp', [('f16x3', 'f16x3'), ('f32', 'f16x3')])
def test_reuse_keeps_every_bit_and_skips_scans(case, fp, bp):
    on, off = case[fp, bp, True], case[fp, bp, False]
    _assert_same_run(on, off)
    print('forward %s, backward %s: with reuse %s, without %s' % (fp, bp, on[3], off[3]))
    assert off[3]['reused'] == 0 and off[3]['scans'] > 0
    assert on[3]['reused'] > 0
    assert on[3]['scans'] + on[3]['reused'] == off[3]['scans']
    assert on[3]['scans'] < off[3]['scans']


def test_fp32_precisions_never_touch_the_maxima(case):
    for reuse in (True, False):
        assert case['f32', 'f32', reuse][3] == {'scans': 0, 'reused': 0}
        _assert_same_run(case['f32', 'f32', reuse], case['default'])
    assert case['default'][3] == {'scans': 0, 'reused': 0}
