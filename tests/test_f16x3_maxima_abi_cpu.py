"""CPU: the three entries that hand max |x| from layer to layer (srcnn_conv2d_forward_f16x3_maxima,
srcnn_conv2d_backward_f16x3_maxima, srcnn_absmax; include/srcnn_hip.h) validate every argument before their first launch, refuse
what the plain entries refuse with the plain entries' codes and messages, and leave the two descriptors as they were.  No call
reaches a launch.  Also the Python surface that needs no device: the reuse_maxima keyword, trainval_net's flag, and the fact the
record of maxima in stereo_rcnn_amd.autograd rests on (a tensor's Python identity across Function.apply)."""
import ctypes
import inspect

import pytest

P = 4096            # a non-null, 16-byte aligned "device pointer" (never dereferenced: every call below is refused first)
Q = 8192            # another one
BIG = 1 << 40


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import _lib
    return _lib.lib()


def _fwd_desc(**kw):
    """tests/test_conv_forward_f16x3_abi_cpu.py's valid layer: 3x3 / stride 1 / pad 1, 64 -> 96 channels on a 2 x 10 x 12 map."""
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


def _bwd_desc(**kw):
    """tests/test_conv_backward_f16x3_abi_cpu.py's valid layer, precision 1."""
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


def _fwd(L, x_amax=P, y_amax=Q, ws=P, ws_bytes=BIG, **kw):
    return L.srcnn_conv2d_forward_f16x3_maxima(ctypes.byref(_fwd_desc(**kw)), x_amax, y_amax, ws, ws_bytes, None)


def _bwd(L, x_amax=P, ws=P, ws_bytes=BIG, **kw):
    return L.srcnn_conv2d_backward_f16x3_maxima(ctypes.byref(_bwd_desc(**kw)), x_amax, ws, ws_bytes, None)


def _err(L):
    return L.srcnn_last_error()


def test_symbols_and_descriptors(L):
    from stereo_rcnn_amd import _lib
    for name in ('srcnn_conv2d_forward_f16x3_maxima', 'srcnn_conv2d_backward_f16x3_maxima', 'srcnn_absmax'):
        assert name in _lib.declared_symbols()
        assert getattr(L, name).restype is ctypes.c_int, name
    # the existing descriptors are the existing entries' ABI: unchanged
    assert ctypes.sizeof(_lib.ConvFwdF16x3Desc) == 5 * 8 + 19 * 4 + 4
    assert ctypes.sizeof(_lib.ConvBwdDesc) == 8 * 8 + 22 * 4 + 4 * 8
    assert len(_lib.ConvBwdDesc._fields_) == 34 and len(_lib.ConvFwdF16x3Desc._fields_) == 24


def test_misaligned_words_are_refused(L):
    for kw in (dict(x_amax=P + 2), dict(y_amax=Q + 1), dict(x_amax=None, y_amax=Q + 2), dict(x_amax=P + 3, y_amax=None)):
        assert _fwd(L, **kw) == -1 and b'aligned' in _err(L), (kw, _err(L))
    assert _bwd(L, x_amax=P + 2) == -1 and b'aligned' in _err(L)
    assert _bwd(L, x_amax=P + 1) == -1 and b'aligned' in _err(L)


def test_aliased_words_are_refused(L):
    assert _fwd(L, x_amax=P, y_amax=P) == -1 and b'alias' in _err(L)
    assert _fwd(L, x_amax=Q, y_amax=Q) == -1 and b'alias' in _err(L)


def test_the_plain_forward_refusals_come_back_unchanged(L):
    """Code and message of the plain entry for the same descriptor, whichever words are given."""
    cases = [dict(x=None), dict(OH=9), dict(Cin=48, x_cstride=48), dict(w=None), dict(x=P + 4), dict(tile_mr=3), dict(x_format=1)]
    texts = [b'null', b'shape', b'multiple of 32', b'null', b'aligned', b'tile', b'format']
    for kw, text in zip(cases, texts):
        rc0 = L.srcnn_conv2d_forward_f16x3(ctypes.byref(_fwd_desc(**kw)), P, BIG, None)
        msg0 = _err(L)
        assert rc0 == -1 and text in msg0
        for words in (dict(), dict(x_amax=None), dict(y_amax=None), dict(x_amax=None, y_amax=None)):
            assert _fwd(L, **dict(kw, **words)) == rc0 and _err(L) == msg0, (kw, words, _err(L))
    assert L.srcnn_conv2d_forward_f16x3_maxima(None, P, Q, P, BIG, None) == -1 and b'null' in _err(L)
    need = L.srcnn_conv2d_forward_f16x3_workspace_bytes(ctypes.byref(_fwd_desc()))
    assert need > 0
    assert L.srcnn_conv2d_forward_f16x3(ctypes.byref(_fwd_desc()), P, need - 1, None) == -3
    msg0 = _err(L)
    assert _fwd(L, ws_bytes=need - 1) == -3 and _err(L) == msg0 and b'workspace' in msg0
    assert _fwd(L, ws=None) == -3 and b'workspace' in _err(L)


def test_the_plain_backward_refusals_come_back_unchanged(L):
    cases = [dict(x=None), dict(OH=9), dict(Cin=48, x_cstride=48), dict(dy=None), dict(precision=0)]
    for kw in cases:
        rc0 = L.srcnn_conv2d_backward_f16x3(ctypes.byref(_bwd_desc(**kw)), P, BIG, None)
        msg0 = _err(L)
        assert rc0 == -1 and msg0
        for x_amax in (P, None):
            assert _bwd(L, x_amax=x_amax, **kw) == rc0 and _err(L) == msg0, (kw, _err(L))
    assert L.srcnn_conv2d_backward_f16x3_maxima(None, P, P, BIG, None) == -1 and b'null' in _err(L)
    need = L.srcnn_conv2d_backward_f16x3_workspace_bytes(ctypes.byref(_bwd_desc()))
    assert need > 0
    assert L.srcnn_conv2d_backward_f16x3(ctypes.byref(_bwd_desc()), P, need - 1, None) == -3
    msg0 = _err(L)
    assert _bwd(L, ws_bytes=need - 1) == -3 and _err(L) == msg0 and b'workspace' in msg0


def test_absmax_refusals(L):
    assert L.srcnn_absmax(None, 4, 32, 32, Q, None) == -1 and b'null' in _err(L)
    assert L.srcnn_absmax(P, 4, 32, 32, None, None) == -1 and b'null' in _err(L)
    for rows, length in ((0, 32), (-1, 32), (4, 0), (4, -8)):
        assert L.srcnn_absmax(P, rows, length, 32, Q, None) == -1 and b'shape' in _err(L), (rows, length)
    assert L.srcnn_absmax(P, 4, 32, 31, Q, None) == -1 and b'stride' in _err(L)
    assert L.srcnn_absmax(P + 2, 4, 32, 32, Q, None) == -1 and b'aligned' in _err(L)
    assert L.srcnn_absmax(P, 4, 32, 32, Q + 2, None) == -1 and b'aligned' in _err(L)


def test_reuse_maxima_defaults_to_true():
    from stereo_rcnn_amd import autograd, engine, training
    for f in (autograd.conv2d, autograd.conv2d_nhwc, autograd.linear, autograd.conv_transpose2x2, training.forward_train,
              training.train_step):
        assert inspect.signature(f).parameters['reuse_maxima'].default is True, f.__name__
    for f in (engine.conv2d_train_f16x3, engine.conv2d_backward):
        assert inspect.signature(f).parameters['x_amax'].default is None, f.__name__
    assert inspect.signature(engine.conv2d_train_f16x3).parameters['y_amax'].default is None
    assert set(engine.F16X3_MAXIMA) == {'scans', 'reused'}
    engine.F16X3_MAXIMA['scans'] = 3
    engine.reset_f16x3_maxima()
    assert engine.F16X3_MAXIMA == {'scans': 0, 'reused': 0}


def test_trainval_flag():
    from stereo_rcnn_amd import trainval_net
    base = ['--kitti-path', 'kitti', '--split', 'train.txt']
    assert trainval_net.parse_args(base).reuse_maxima is True
    assert trainval_net.parse_args(base + ['--no-reuse-maxima']).reuse_maxima is False
    args = trainval_net.parse_args(base + ['--forward-precision', 'f16x3', '--no-reuse-maxima'])
    assert (args.forward_precision, args.reuse_maxima) == ('f16x3', False)


def test_tensor_identity_survives_function_apply():
    """What autograd's record of maxima is keyed on: forward() sees the very input object, and apply() returns the very object
    forward() returned.  (The record is written on what apply() returned either way.)"""
    import torch
    seen = {}

    class F(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w):
            seen['x'] = x
            seen['y'] = x * w
            return seen['y']

        @staticmethod
        def backward(ctx, g):
            return g, g

    x, w = torch.ones(3), torch.ones(3, requires_grad=True)
    y = F.apply(x, w)
    assert seen['x'] is x and seen['y'] is y and y.requires_grad


def test_the_record_of_maxima_misses_what_is_not_the_recorded_tensor():
    """stereo_rcnn_amd.autograd's record on CPU tensors (no launch): a hit needs the same object at the same version."""
    import gc
    import torch
    from stereo_rcnn_amd import autograd
    t, word = torch.ones(2, 3, 4, 32), torch.zeros(1, dtype=torch.int32)
    autograd._record_maximum(t, word)
    assert autograd._known_maximum(t) is word
    assert autograd._known_maximum(t[:1]) is None and autograd._known_maximum(t.view(6, 1, 4, 32)) is None
    assert autograd._known_maximum(torch.cat((t[:1], t[1:]), 0)) is None
    assert autograd._known_maximum(t.detach()) is None                  # another object over the same memory
    assert autograd._known_maximum(t.contiguous()) is word              # .contiguous() of a contiguous tensor is the tensor
    t.add_(0)
    assert autograd._known_maximum(t) is None                           # changed in place since
    key = id(t)
    del t
    gc.collect()
    assert key not in autograd._MAXIMA                                  # the entry leaves with its tensor
