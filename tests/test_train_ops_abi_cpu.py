"""CPU: the three adjoint entry points of csrc/train_ops.hip validate every argument before their first launch (include/srcnn_hip.h,
"training: remaining adjoints"), so each refusal is checkable on a host without a GPU -- the pattern of
tests/test_conv_backward_abi_cpu.py.  No call here reaches a launch.  The Python entry points refuse CPU tensors."""
import pytest

P = 4096            # a non-null, 16-byte aligned "device pointer" (never dereferenced: every call below is refused first)


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import _lib
    return _lib.lib()


def _refused(L, rc, text):
    assert rc == -1, rc
    assert text in L.srcnn_last_error(), L.srcnn_last_error()


def test_version(L):
    assert L.srcnn_version() >= 290


def test_upsample_add_backward_refusals(L):
    f = L.srcnn_upsample_add_backward          # (dy, B, H, W, C, d_top, TH, TW, stream)
    _refused(L, f(None, 2, 7, 21, 8, P, 4, 11, None), b'null')
    _refused(L, f(P, 2, 7, 21, 8, None, 4, 11, None), b'null')
    good = [2, 7, 21, 8, 4, 11]                 # B, H, W, C, TH, TW
    for i in range(6):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            _refused(L, f(P, a[0], a[1], a[2], a[3], P, a[4], a[5], None), b'shape')
    _refused(L, f(P, 2, 3, 21, 8, P, 4, 11, None), b'shape')            # H < TH
    _refused(L, f(P, 2, 7, 10, 8, P, 4, 11, None), b'shape')            # W < TW
    _refused(L, f(P, 2, 7, 21, 12, P, 4, 11, None), b'stride')          # C % 8
    _refused(L, f(P, 2, 7, 21, 12, P, 4, 11, None), b'multiple of 8')
    _refused(L, f(P + 4, 2, 7, 21, 8, P, 4, 11, None), b'aligned')
    _refused(L, f(P, 70000, 7, 21, 8, P, 4, 11, None), b'shape')        # beyond the launch grid


def test_subsample2_backward_refusals(L):
    f = L.srcnn_subsample2_backward            # (dy, B, OH, OW, C, dx, H, W, stream)
    _refused(L, f(None, 2, 4, 11, 8, P, 7, 21, None), b'null')
    _refused(L, f(P, 2, 4, 11, 8, None, 7, 21, None), b'null')
    good = [2, 4, 11, 8, 7, 21]
    for i in range(6):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            _refused(L, f(P, a[0], a[1], a[2], a[3], P, a[4], a[5], None), b'shape')
    _refused(L, f(P, 2, 3, 11, 8, P, 7, 21, None), b'shape')            # OH is not ceil(H / 2)
    _refused(L, f(P, 2, 4, 10, 8, P, 7, 21, None), b'shape')
    _refused(L, f(P, 2, 4, 11, 20, P, 7, 21, None), b'stride')
    _refused(L, f(P, 2, 4, 11, 8, P + 8, 7, 21, None), b'aligned')


def test_pixel_shuffle2_refusals(L):
    f = L.srcnn_pixel_shuffle2                 # (x, M, h, w, Cq, y, inverse, stream)
    _refused(L, f(None, 3, 14, 14, 256, P, 0, None), b'null')
    _refused(L, f(P, 3, 14, 14, 256, None, 1, None), b'null')
    good = [3, 14, 14, 256]
    for i in range(4):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            _refused(L, f(P, a[0], a[1], a[2], a[3], P, 0, None), b'shape')
    _refused(L, f(P, 3, 14, 14, 256, P, 2, None), b'shape')
    _refused(L, f(P, 3, 14, 14, 256, P, -1, None), b'shape')
    _refused(L, f(P, 3, 14, 14, 4, P, 0, None), b'stride')
    _refused(L, f(P + 4, 3, 14, 14, 256, P, 0, None), b'aligned')


def test_conv_backward_still_refuses_mode_1(L):
    import ctypes
    from stereo_rcnn_amd import _lib
    d = _lib.ConvBwdDesc()
    d.x = d.w = d.y = d.dy = d.dx = d.dw = d.db = P
    d.B, d.H, d.W, d.Cin, d.x_cstride, d.OH, d.OW, d.Cout = 3, 14, 14, 256, 256, 14, 14, 1024
    d.KH, d.KW, d.stride, d.pad, d.y_cstride, d.relu, d.mode = 1, 1, 1, 0, 1024, 1, 1
    _refused(L, L.srcnn_conv2d_backward(ctypes.byref(d), P, 1 << 40, None), b'mode')


def test_python_entry_points_refuse_cpu_tensors():
    import torch
    from stereo_rcnn_amd import autograd
    with pytest.raises(NotImplementedError):
        autograd.upsample_add(torch.zeros(1, 2, 2, 8), torch.zeros(1, 4, 4, 8))
    with pytest.raises(NotImplementedError):
        autograd.subsample2(torch.zeros(1, 3, 3, 8))
    with pytest.raises(NotImplementedError):
        autograd.conv_transpose2x2(torch.zeros(1, 2, 2, 32), torch.zeros(32, 8, 2, 2), torch.zeros(8), True)
    with pytest.raises(NotImplementedError):
        autograd.conv2d_nhwc(torch.zeros(1, 4, 4, 32), torch.zeros(8, 32, 1, 1))
    with pytest.raises(NotImplementedError):
        autograd.pixel_shuffle2(torch.zeros(1, 2, 2, 32), 8)


def test_forward_train_refuses_a_cpu_model():
    import torch
    from stereo_rcnn_amd import training
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    model = resnet(('__background__', 'Car'), 50)
    model.create_architecture()
    z = torch.zeros
    with pytest.raises(NotImplementedError):
        training.forward_train(model, z(1, 3, 64, 96), z(1, 3, 64, 96), torch.tensor([[64., 96., 1.]]), z(1, 2, 5), z(1, 2, 5),
                               z(1, 2, 5), z(1, 2, 5), z(1, 2, 6), torch.tensor([2]))
