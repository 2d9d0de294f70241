"""CPU: stereo_rcnn_amd.autograd.Precision, the one place the two precision strings are validated, and the six public functions
that build it from their three keyword arguments.  Every call below is refused before it touches a tensor's device, and before
any other check of the function (the tensors here are CPU tensors, which these functions otherwise answer with NotImplementedError)."""
import pytest
import torch

BACKWARD = "backward_precision must be 'f32' or 'f16x3' \\(got 'bf16'\\)"
FORWARD = "forward_precision must be 'f32' or 'f16x3' \\(got 'bf16'\\)"


def test_the_value():
    from stereo_rcnn_amd.autograd import Precision
    p = Precision()
    assert (p.forward, p.backward, p.reuse_maxima) == ('f32', 'f32', True)
    q = Precision('f16x3', 'f32', 0)
    assert (q.forward, q.backward, q.reuse_maxima) == ('f16x3', 'f32', False) and q.reuse_maxima is False
    assert q.without_graph() == Precision('f32', 'f32', False) and q.forward == 'f16x3'          # a new value: q is as it was
    with pytest.raises(AttributeError):
        q.forward = 'f32'
    with pytest.raises(ValueError, match=BACKWARD):
        Precision('f32', 'bf16')
    with pytest.raises(ValueError, match=FORWARD):
        Precision('bf16', 'f32')
    with pytest.raises(ValueError, match=FORWARD):                 # both unknown: the forward's message
        Precision('bf16', 'bf16')


def _public_calls(**kw):
    from stereo_rcnn_amd import autograd, training
    x, w = torch.zeros(1, 1, 1, 32), torch.zeros(8, 32, 1, 1)
    model = torch.nn.Linear(1, 1)
    optimizer = torch.optim.SGD(model.parameters(), lr=0.1)
    batch = (None,) * 9
    return {'conv2d': lambda: autograd.conv2d(x.permute(0, 3, 1, 2), w, **kw),
            'conv2d_nhwc': lambda: autograd.conv2d_nhwc(x, w, **kw),
            'linear': lambda: autograd.linear(x.view(1, 32), w.view(8, 32), **kw),
            'conv_transpose2x2': lambda: autograd.conv_transpose2x2(x, torch.zeros(32, 8, 2, 2), **kw),
            'forward_train': lambda: training.forward_train(model, *batch, **kw),
            'train_step': lambda: training.train_step(model, optimizer, torch.zeros(6), batch, **kw)}


@pytest.mark.parametrize('keyword, text', [('backward_precision', BACKWARD), ('forward_precision', FORWARD)])
def test_every_public_function_refuses_an_unknown_precision(keyword, text):
    for others in ({}, {'reuse_maxima': False}):
        for name, call in _public_calls(**dict(others, **{keyword: 'bf16'})).items():
            with pytest.raises(ValueError, match=text):
                call()
    # both unknown: the forward's message, from every function
    for name, call in _public_calls(forward_precision='bf16', backward_precision='bf16').items():
        with pytest.raises(ValueError, match=FORWARD):
            call()
    # the other keyword valid and not the default: still the bad one's message
    other = 'forward_precision' if keyword == 'backward_precision' else 'backward_precision'
    for name, call in _public_calls(**{keyword: 'bf16', other: 'f16x3'}).items():
        with pytest.raises(ValueError, match=text):
            call()
