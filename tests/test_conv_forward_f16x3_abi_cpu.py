"""CPU: srcnn_conv2d_forward_f16x3 validates every argument before its first launch, as srcnn_conv2d_backward_f16x3 does
(tests/test_conv_backward_f16x3_abi_cpu.py).  No call reaches a launch.  Also the Python surface that needs no device: the
forward_precision keyword's refusal and trainval_net's flag."""
import ctypes

import pytest

P = 4096            # a non-null, 16-byte aligned "device pointer" (never dereferenced: every call below is refused first)
BIG = 1 << 40


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import _lib
    return _lib.lib()


def _desc(**kw):
    """A valid 3x3 / stride 1 / pad 1 layer, 64 -> 96 channels on a 2 x 10 x 12 map with bias, residual and ReLU; keyword
    arguments override."""
    from stereo_rcnn_amd import _lib
    d = _lib.ConvFwdF16x3Desc()
    d.x = d.w = d.bias = d.residual = d.y = P
    d.B, d.H, d.W, d.Cin, d.x_cstride = 2, 10, 12, 64, 64
    d.OH, d.OW, d.Cout = 10, 12, 96
    d.KH, d.KW, d.stride, d.pad = 3, 3, 1, 1
    d.y_cstride, d.y_coffset, d.relu = 96, 0, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(L, ws=P, ws_bytes=BIG, **kw):
    return L.srcnn_conv2d_forward_f16x3(ctypes.byref(_desc(**kw)), ws, ws_bytes, None)


def _q(L, **kw):
    return L.srcnn_conv2d_forward_f16x3_workspace_bytes(ctypes.byref(_desc(**kw)))


def _refused(L, text, **kw):
    rc = _call(L, **kw)
    assert rc == -1, rc
    assert text in L.srcnn_last_error(), L.srcnn_last_error()
    assert _q(L, **kw) == 0


def test_signature(L):
    from stereo_rcnn_amd import _lib
    assert L.srcnn_conv2d_forward_f16x3.restype is ctypes.c_int
    assert L.srcnn_conv2d_forward_f16x3_workspace_bytes.restype is ctypes.c_size_t
    names = [n for n, _ in _lib.ConvFwdF16x3Desc._fields_]
    assert names[:5] == ['x', 'w', 'bias', 'residual', 'y'] and names[-2:] == ['tile_mr', 'tile_nr']
    # no fused-head, second-input or upsample fields, no mode / precision: a struct of its own
    assert not {'head_w', 'head_wf', 'x2', 'up_top', 'mode', 'precision', 'splits'} & set(names)
    assert ctypes.sizeof(_lib.ConvFwdF16x3Desc) == 5 * 8 + 19 * 4 + 4          # five pointers, nineteen ints, tail padding


def test_null_pointers(L):
    assert L.srcnn_conv2d_forward_f16x3(None, P, BIG, None) == -1 and b'null' in L.srcnn_last_error()
    assert L.srcnn_conv2d_forward_f16x3_workspace_bytes(None) == 0
    _refused(L, b'null', x=None)
    _refused(L, b'null', w=None)
    _refused(L, b'null', y=None)
    assert _call(L, ws=None) == -3 and b'workspace' in L.srcnn_last_error()
    assert _q(L, bias=None) > 0 and _q(L, residual=None) > 0 and _q(L, bias=None, residual=None, relu=0) > 0


def test_formats(L):
    _refused(L, b'format', x_format=1)
    _refused(L, b'format', y_format=1)


def test_shapes_and_strides(L):
    for field in ('B', 'H', 'W', 'OH', 'OW', 'Cout', 'Cin', 'KH', 'KW', 'stride'):
        _refused(L, b'shape', **{field: -1})
        _refused(L, b'shape', **{field: 0})
    _refused(L, b'shape', pad=-1)
    _refused(L, b'shape', OH=9)
    _refused(L, b'shape', stride=2)
    _refused(L, b'multiple of 32', Cin=48, x_cstride=48)
    _refused(L, b'stride', x_cstride=32)
    _refused(L, b'stride', x_cstride=66)
    _refused(L, b'stride', y_cstride=95)
    _refused(L, b'stride', y_cstride=100, y_coffset=8)
    _refused(L, b'stride', y_coffset=-4)
    _refused(L, b'aligned', x=P + 4)
    _refused(L, b'aligned', w=P + 8)
    _refused(L, b'tile', tile_mr=3)
    _refused(L, b'tile', tile_nr=-1)
    _refused(L, b'too large', B=1 << 20, H=1 << 10, W=1 << 10, OH=1 << 10, OW=1 << 10)


def test_workspace_query(L):
    Cp, K = 96, 9 * 64
    need = _q(L)
    assert 2 * 2 * Cp * K + 8 <= need <= 2 * 2 * Cp * K + 3 * 256          # two f16 planes and the two scale words
    assert _q(L, Cout=70, y_cstride=70) == need                             # Cp: Cout rounded up to 32
    assert _q(L, tile_mr=1, tile_nr=1) == need == _q(L, tile_mr=2, tile_nr=2)
    assert _call(L, ws_bytes=need - 1) == -3 and b'workspace' in L.srcnn_last_error()
    assert _call(L, ws_bytes=0) == -3


def test_unknown_forward_precision_is_refused():
    import torch
    from stereo_rcnn_amd import autograd, training
    x, w = torch.zeros(1, 1, 1, 32), torch.zeros(8, 32, 1, 1)
    for call in (lambda: autograd.conv2d_nhwc(x, w, forward_precision='bf16'),
                 lambda: autograd.conv2d(x.permute(0, 3, 1, 2), w, forward_precision='bf16'),
                 lambda: autograd.linear(x.view(1, 32), w.view(8, 32), forward_precision='bf16'),
                 lambda: autograd.conv_transpose2x2(x, torch.zeros(32, 8, 2, 2), forward_precision='bf16')):
        with pytest.raises(ValueError, match="forward_precision must be 'f32' or 'f16x3'"):
            call()
    import inspect
    for f in (autograd.conv2d, autograd.conv2d_nhwc, autograd.linear, autograd.conv_transpose2x2, training.forward_train,
              training.train_step):
        assert inspect.signature(f).parameters['forward_precision'].default == 'f32', f.__name__
        assert inspect.signature(f).parameters['backward_precision'].default == 'f32', f.__name__


def test_trainval_flag():
    from stereo_rcnn_amd import trainval_net
    base = ['--kitti-path', 'kitti', '--split', 'train.txt']
    assert trainval_net.parse_args(base).forward_precision == 'f32'
    assert trainval_net.parse_args(base + ['--forward-precision', 'f16x3']).forward_precision == 'f16x3'
    args = trainval_net.parse_args(base + ['--forward-precision', 'f16x3', '--backward-precision', 'f32'])
    assert (args.forward_precision, args.backward_precision) == ('f16x3', 'f32')
    assert trainval_net.parse_args(base + ['--forward-precision', 'f32']).forward_precision == 'f32'
    with pytest.raises(SystemExit):
        trainval_net.parse_args(base + ['--forward-precision', 'bf16'])
