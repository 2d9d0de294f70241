"""CPU: srcnn_conv2d_backward_f16x3 validates every argument before its first launch, as srcnn_conv2d_backward does
(tests/test_conv_backward_abi_cpu.py) -- the same refusals, except that precision must be 1 here.  No call reaches a launch."""
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
    """A valid 3x3 / stride 1 / pad 1 layer, 64 -> 96 channels on a 2 x 10 x 12 map, precision 1; keyword arguments override."""
    from stereo_rcnn_amd import _lib
    d = _lib.ConvBwdDesc()
    d.x = d.w = d.y = d.dy = d.dx = d.dw = d.db = P
    d.B, d.H, d.W, d.Cin, d.x_cstride = 2, 10, 12, 64, 64
    d.OH, d.OW, d.Cout = 10, 12, 96
    d.KH, d.KW, d.stride, d.pad = 3, 3, 1, 1
    d.y_cstride, d.y_coffset, d.relu = 96, 0, 1
    d.precision = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(L, ws=P, ws_bytes=BIG, **kw):
    return L.srcnn_conv2d_backward_f16x3(ctypes.byref(_desc(**kw)), ws, ws_bytes, None)


def _q(L, **kw):
    return L.srcnn_conv2d_backward_f16x3_workspace_bytes(ctypes.byref(_desc(**kw)))


def _refused(L, text, **kw):
    rc = _call(L, **kw)
    assert rc == -1, rc
    assert text in L.srcnn_last_error(), L.srcnn_last_error()
    assert _q(L, **kw) == 0


def test_precision(L):
    _refused(L, b'precision', precision=0)
    _refused(L, b'precision', precision=2)
    assert _q(L) > 0
    # ... and the fp32 entry keeps refusing this descriptor
    assert L.srcnn_conv2d_backward(ctypes.byref(_desc()), P, BIG, None) == -1 and b'precision' in L.srcnn_last_error()


def test_null_pointers(L):
    assert L.srcnn_conv2d_backward_f16x3(None, P, BIG, None) == -1 and b'null' in L.srcnn_last_error()
    assert L.srcnn_conv2d_backward_f16x3_workspace_bytes(None) == 0
    _refused(L, b'null', dy=None)
    _refused(L, b'null', dx=None, dw=None, db=None)
    _refused(L, b'null', x=None)
    _refused(L, b'null', w=None)
    _refused(L, b'null', y=None)
    assert _call(L, ws=None) == -3 and b'workspace' in L.srcnn_last_error()
    assert _q(L, x=None, dw=None) > 0 and _q(L, w=None, dx=None) > 0 and _q(L, y=None, relu=0) > 0


def test_unsupported_fields(L):
    _refused(L, b'mode', mode=1)
    _refused(L, b'mode', mode=2)
    _refused(L, b'format', x_format=1)
    _refused(L, b'format', y_format=1)
    _refused(L, b'fused head', head_w=P)
    _refused(L, b'fused head', head_wf=P)
    _refused(L, b'second input', x2=P)
    _refused(L, b'upsample', up_top=P)


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
    _refused(L, b'tile', tile_mr=3)
    _refused(L, b'tile', tile_nr=-1)
    _refused(L, b'splits', splits=-1)
    _refused(L, b'too large', B=1 << 20, H=1 << 10, W=1 << 10, OH=1 << 10, OW=1 << 10)


def test_workspace_query(L):
    M, Cp, K = 2 * 10 * 12, 96, 9 * 64
    one = _q(L, splits=1)
    # masked gradient + bias partials + the two f16 weight planes (the bytes of one fp32 copy) + the scale words
    assert one >= 4 * (M * Cp + Cp + 64 * 9 * Cp) + 16
    fp32 = L.srcnn_conv2d_backward_workspace_bytes(ctypes.byref(_desc(splits=1, precision=0)))
    assert fp32 < one <= fp32 + 256
    assert _q(L, splits=2) >= one + 2 * 4 * 96 * K
    assert _q(L, splits=1000) == _q(L, splits=8)
    assert _q(L, splits=4, dw=None, x=None) == _q(L, splits=1, dw=None, x=None)
    assert _q(L, splits=1, dx=None, w=None) < one
    assert _call(L, ws_bytes=one - 1, splits=1) == -3 and b'workspace' in L.srcnn_last_error()
    assert _call(L, ws_bytes=0, splits=1) == -3
    assert _call(L, ws_bytes=one, splits=2) == -3


def test_engine_refuses_an_unknown_precision():
    from stereo_rcnn_amd import engine
    with pytest.raises(ValueError):
        engine.conv2d_backward(None, None, 1, 1, 1, None, None, 1, 1, precision='bf16')
