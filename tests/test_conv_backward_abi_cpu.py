"""CPU: srcnn_conv2d_backward validates every argument before its first launch (include/srcnn_hip.h, "convolution backward"),
so each refusal is checkable on a host without a GPU -- the pattern of tests/test_losses_abi_cpu.py.  No call here reaches a
launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096            # a non-null, 16-byte aligned "device pointer" (never dereferenced: every call below is refused first)
BIG = 1 << 40       # workspace bytes that would do


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import _lib
    return _lib.lib()


def _desc(**kw):
    """A valid 3x3 / stride 1 / pad 1 layer, 64 -> 96 channels on a 2 x 10 x 12 map; keyword arguments override fields."""
    from stereo_rcnn_amd import _lib
    d = _lib.ConvBwdDesc()
    d.x = d.w = d.y = d.dy = d.dx = d.dw = d.db = P
    d.B, d.H, d.W, d.Cin, d.x_cstride = 2, 10, 12, 64, 64
    d.OH, d.OW, d.Cout = 10, 12, 96
    d.KH, d.KW, d.stride, d.pad = 3, 3, 1, 1
    d.y_cstride, d.y_coffset, d.relu = 96, 0, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(L, ws=P, ws_bytes=BIG, **kw):
    return L.srcnn_conv2d_backward(ctypes.byref(_desc(**kw)), ws, ws_bytes, None)


def _refused(L, rc, text):
    assert rc == -1, rc
    assert text in L.srcnn_last_error(), L.srcnn_last_error()


def test_version(L):
    assert L.srcnn_version() >= 280


def test_null_pointers(L):
    assert L.srcnn_conv2d_backward(None, P, BIG, None) == -1 and b'null' in L.srcnn_last_error()
    _refused(L, _call(L, dy=None), b'null')
    _refused(L, _call(L, dx=None, dw=None, db=None), b'null')          # nothing requested
    _refused(L, _call(L, x=None), b'null')                             # dw needs x
    _refused(L, _call(L, w=None), b'null')                             # dx needs w
    _refused(L, _call(L, y=None), b'null')                             # relu needs the saved output
    assert _call(L, ws=None) == -3 and b'workspace' in L.srcnn_last_error()
    # ... and what is not needed may be null
    q = L.srcnn_conv2d_backward_workspace_bytes
    assert q(ctypes.byref(_desc(x=None, dw=None))) > 0 and q(ctypes.byref(_desc(w=None, dx=None))) > 0
    assert q(ctypes.byref(_desc(y=None, relu=0))) > 0


def test_unsupported_fields(L):
    _refused(L, _call(L, mode=1), b'mode')
    _refused(L, _call(L, mode=2), b'mode')
    _refused(L, _call(L, precision=1), b'precision')
    _refused(L, _call(L, x_format=1), b'format')
    _refused(L, _call(L, y_format=1), b'format')
    _refused(L, _call(L, head_w=P), b'fused head')
    _refused(L, _call(L, head_wf=P), b'fused head')
    _refused(L, _call(L, x2=P), b'second input')
    _refused(L, _call(L, up_top=P), b'upsample')


def test_shapes_and_strides(L):
    for field in ('B', 'H', 'W', 'OH', 'OW', 'Cout', 'Cin', 'KH', 'KW', 'stride'):
        _refused(L, _call(L, **{field: -1}), b'shape')
        _refused(L, _call(L, **{field: 0}), b'shape')
    _refused(L, _call(L, pad=-1), b'shape')
    _refused(L, _call(L, OH=9), b'shape')                               # not the forward's output size
    _refused(L, _call(L, stride=2), b'shape')
    _refused(L, _call(L, Cin=48, x_cstride=48), b'multiple of 32')
    _refused(L, _call(L, x_cstride=32), b'stride')                      # smaller than Cin
    _refused(L, _call(L, x_cstride=66), b'stride')                      # not a multiple of 4
    _refused(L, _call(L, y_cstride=95), b'stride')
    _refused(L, _call(L, y_cstride=100, y_coffset=8), b'stride')
    _refused(L, _call(L, y_coffset=-4), b'stride')
    _refused(L, _call(L, x=P + 4), b'aligned')
    _refused(L, _call(L, tile_mr=3), b'tile')
    _refused(L, _call(L, tile_nr=-1), b'tile')
    _refused(L, _call(L, splits=-1), b'splits')
    _refused(L, _call(L, B=1 << 20, H=1 << 10, W=1 << 10, OH=1 << 10, OW=1 << 10), b'too large')


def test_workspace_query(L):
    q = lambda **kw: L.srcnn_conv2d_backward_workspace_bytes(ctypes.byref(_desc(**kw)))
    assert q(B=-1) == 0 and q(Cout=-5) == 0 and q(H=0) == 0 and q(mode=1) == 0
    assert L.srcnn_conv2d_backward_workspace_bytes(None) == 0
    M, Cp, K = 2 * 10 * 12, 96, 9 * 64
    one = q(splits=1)
    assert one >= 4 * (M * Cp + Cp + 64 * 9 * Cp)                      # masked gradient + bias partials + re-laid weights
    assert q(splits=2) >= one + 2 * 4 * 96 * K > one
    assert q(splits=4) >= q(splits=2) + 2 * 4 * 96 * K
    assert q(splits=1000) == q(splits=8)                                # M / 32 = 7.5: no more slices than K tiles
    assert q(splits=1, dw=None, x=None) == one                          # slices belong to the weight gradient
    assert q(splits=4, dw=None, x=None) == one
    assert q(splits=1, dx=None, w=None) < one                           # no re-laid weights without dx
    assert q(splits=0) >= one
    # too small a workspace: refused with its own code, before any launch
    assert _call(L, ws_bytes=one - 1, splits=1) == -3 and b'workspace' in L.srcnn_last_error()
    assert _call(L, ws_bytes=0, splits=1) == -3
    assert _call(L, ws_bytes=one, splits=2) == -3


def _header_struct_fields():
    """(name, size) of every field of srcnn_conv_bwd_desc as the header declares it (pointers 8 bytes, int / float 4)."""
    hdr = open(os.path.join(ROOT, 'include', 'srcnn_hip.h')).read()
    body = re.search(r'typedef struct srcnn_conv_bwd_desc \{(.*?)\} srcnn_conv_bwd_desc;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r'((?:const\s+)?(?:float|int|void))\s+(.*)$', decl, re.S)
        assert m, decl
        for name in m.group(2).split(','):
            name = name.strip()
            fields.append((name.lstrip('* '), 8 if name.startswith('*') else 4))
    return fields


def test_struct_matches_the_header():
    from stereo_rcnn_amd import _lib
    fields = _header_struct_fields()
    assert [n for n, _ in fields] == [f[0] for f in _lib.ConvBwdDesc._fields_]
    off = 0
    for name, size in fields:
        off = (off + size - 1) // size * size
        assert getattr(_lib.ConvBwdDesc, name).offset == off and getattr(_lib.ConvBwdDesc, name).size == size, name
        off += size
    assert ctypes.sizeof(_lib.ConvBwdDesc) == (off + 7) // 8 * 8


def test_python_entry_points_refuse_cpu_tensors():
    import torch
    from stereo_rcnn_amd import autograd
    with pytest.raises(NotImplementedError):
        autograd.conv2d(torch.zeros(1, 32, 4, 4), torch.zeros(8, 32, 1, 1))
    with pytest.raises(NotImplementedError):
        autograd.linear(torch.zeros(3, 64), torch.zeros(5, 64))
