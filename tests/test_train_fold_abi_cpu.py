"""CPU: the C ABI of the device-side weight fold as the header-derived binding sees it (include/srcnn_hip.h, "frozen-BN fold +
engine layout of every weight" -> stereo_rcnn_amd._lib): the descriptor, the three entries, the workspace query, every refusal
before the first launch, and the Python keywords that reach it (train_step's device_fold, trainval_net's --device-fold).  The
descriptor's layout against the C compiler's is tests/test_abi_header_cpu.py's, with every structure."""
import ctypes
import glob
import os

import pytest

from stereo_rcnn_amd import _lib

FIELDS = ['w', 'bias', 'grad_w', 'grad_b', 'bn_weight', 'bn_bias', 'bn_mean', 'bn_var', 'dst_w', 'dst_b', 'rows', 'n_parts', 'kind',
          'Cout', 'KH', 'KW', 'Cin']
P, Z, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
RECORD = 144                # the header: bytes of one table record


def test_the_entries_are_declared_by_the_one_header():
    new = ['srcnn_train_fold_workspace_bytes', 'srcnn_train_weights_fold', 'srcnn_train_weights_fold_backward']
    assert set(new) <= set(_lib.declared_symbols())
    assert _lib.HEADER.structs['srcnn_train_fold_desc'] is _lib.TrainFoldDesc
    assert [os.path.basename(p) for p in glob.glob(os.path.join(os.path.dirname(_lib.HEADER_PATH), '*.h'))] == ['srcnn_hip.h']
    assert (_lib.TRAIN_FOLD_CONV, _lib.TRAIN_FOLD_LINEAR, _lib.TRAIN_FOLD_DECONV2X2) == (0, 1, 2)
    assert _lib.TRAIN_FOLD_LAYERS_PER_BLOCK * RECORD + 16 <= 4096          # a block of records fits HIP's kernel-argument block


def test_descriptor_and_signatures():
    D = _lib.TrainFoldDesc
    assert [f[0] for f in D._fields_] == FIELDS
    assert [f[1] for f in D._fields_] == [P * 3] * 4 + [P] * 6 + [I * 3] + [I] * 6
    assert ctypes.sizeof(D) == 18 * 8 + 9 * 4 + 4           # the pointers, the ints, padding to the pointers' alignment
    S = _lib._SIGNATURES
    desc, host = ctypes.POINTER(D), ctypes.POINTER(P)
    assert S['srcnn_train_fold_workspace_bytes'] == (Z, [I])
    assert S['srcnn_train_weights_fold'] == (I, [desc, I, P, Z, P])
    assert S['srcnn_train_weights_fold_backward'] == (I, [desc, I, host, host, P, Z, P])


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    return _lib.lib()


def test_workspace_bytes(L):
    q = L.srcnn_train_fold_workspace_bytes
    assert q(0) == 0 and q(-3) == 0
    for n in (1, 2, 24, 25, 113):
        assert q(n) == -(-n * RECORD // 256) * 256, n


ADDR = 4096         # a non-null, 16-byte aligned "device pointer" (never dereferenced: every call below is refused first)


def _layer(n=1, **kw):
    """n copies of a valid two-part 3x3 layer with a bias (40 = 16 + 24 rows, Cin 64); kw changes the LAST one.  A tuple value
    (index, v) sets one element of an array field."""
    d = (_lib.TrainFoldDesc * n)()
    for i in range(n):
        for p in range(2):
            d[i].w[p] = d[i].bias[p] = d[i].grad_w[p] = d[i].grad_b[p] = ADDR
        d[i].dst_w = d[i].dst_b = ADDR
        d[i].rows[0], d[i].rows[1] = 16, 24
        d[i].n_parts, d[i].kind, d[i].Cout, d[i].KH, d[i].KW, d[i].Cin = 2, _lib.TRAIN_FOLD_CONV, 40, 3, 3, 64
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d[n - 1], k)[v[0]] = v[1]
        else:
            setattr(d[n - 1], k, v)
    return d


def _grads(n, value=ADDR):
    return (P * n)(*[value] * n)


REFUSALS = [
    (dict(w=(1, None)), 'layer 1: null pointer: w', 'f'),
    (dict(w=(0, ADDR + 4)), 'layer 1: w must be 16-byte aligned', 'f'),
    (dict(dst_w=None), 'layer 1: null pointer: dst_w', 'f'),
    (dict(dst_w=ADDR + 8), 'layer 1: dst_w must be 16-byte aligned', 'f'),
    (dict(dst_b=None), 'layer 1: null pointer: dst_b', 'f'),
    (dict(dst_b=ADDR + 2), 'layer 1: dst_b must be 4-byte aligned', 'f'),
    (dict(bias=(1, None)), 'layer 1: every part carries a bias, or none', 'fb'),
    (dict(bias=(1, ADDR + 1)), 'layer 1: bias must be 4-byte aligned', 'fb'),
    (dict(grad_w=(1, None)), 'layer 1: null pointer: grad_w', 'b'),
    (dict(grad_w=(0, ADDR + 4)), 'layer 1: grad_w must be 16-byte aligned', 'b'),
    (dict(grad_b=(0, None)), 'layer 1: null pointer: grad_b', 'b'),
    (dict(n_parts=4), 'layer 1: n_parts must be 1, 2 or 3', 'fb'),
    (dict(n_parts=0), 'layer 1: n_parts must be 1, 2 or 3', 'fb'),
    (dict(Cout=0), 'layer 1: bad shape: sizes must be positive', 'fb'),
    (dict(KW=-1), 'layer 1: bad shape: sizes must be positive', 'fb'),
    (dict(rows=(1, 0)), 'layer 1: bad shape: the rows of a part must be positive', 'fb'),
    (dict(Cin=48), 'layer 1: Cin must be a positive multiple of 32', 'fb'),
    (dict(rows=(1, 23)), 'layer 1: the rows of the parts do not sum to Cout', 'fb'),
    (dict(kind=3), 'layer 1: unknown layout kind', 'fb'),
    (dict(kind=-1), 'layer 1: unknown layout kind', 'fb'),
    (dict(kind=1), 'layer 1: bad shape: the linear kind is 1x1', 'fb'),
    (dict(kind=2), 'layer 1: bad shape: the deconvolution kind is one 2x2 part', 'fb'),
    (dict(KH=12, KW=11), 'layer 1: bad shape: KH KW above 128', 'fb'),
    (dict(Cout=1 << 19, rows=(0, (1 << 19) - 24), KH=8, KW=8), 'layer 1: bad shape: a layer of 2^31 elements or more', 'fb'),
    (dict(bn_weight=ADDR), 'layer 1: null pointer: a frozen BN needs all of', 'fb'),
    (dict(bn_weight=ADDR, bn_bias=ADDR, bn_mean=ADDR, bn_var=ADDR), 'layer 1: a frozen BN folds into a single convolution part', 'fb'),
]


@pytest.mark.parametrize('kw,text,which', REFUSALS)
def test_refused_before_any_launch_naming_the_layer(L, kw, text, which):
    d = _layer(2, **kw)
    if 'f' in which:
        rc = L.srcnn_train_weights_fold(d, 2, ADDR, 1 << 20, None)
        assert rc == _lib.ERR_ARG and text in L.srcnn_last_error().decode(), (rc, L.srcnn_last_error())
    if 'b' in which:
        rc = L.srcnn_train_weights_fold_backward(d, 2, _grads(2), _grads(2), ADDR, 1 << 20, None)
        assert rc == _lib.ERR_ARG and text in L.srcnn_last_error().decode(), (rc, L.srcnn_last_error())


def test_refused_lists_workspaces_and_gradient_arrays(L):
    fold, back = L.srcnn_train_weights_fold, L.srcnn_train_weights_fold_backward
    d, g = _layer(1), _grads(1)
    for call, text in ((lambda: fold(None, 1, ADDR, 1 << 20, None), 'null layers_host'),
                     (lambda: back(None, 1, g, g, ADDR, 1 << 20, None), 'null layers_host'),
                     (lambda: fold(d, 0, ADDR, 1 << 20, None), 'n_layers'),
                     (lambda: back(d, -1, g, g, ADDR, 1 << 20, None), 'n_layers'),
                     (lambda: fold(d, 1, None, 1 << 20, None), 'null workspace'),
                     (lambda: back(d, 1, g, g, None, 1 << 20, None), 'null workspace'),
                     (lambda: fold(d, 1, ADDR + 4, 1 << 20, None), 'workspace must be 16-byte aligned'),
                     (lambda: back(d, 1, None, g, ADDR, 1 << 20, None), 'null dw_folded_host'),
                     (lambda: back(d, 1, g, None, ADDR, 1 << 20, None), 'null dw_folded_host'),
                     (lambda: back(d, 1, _grads(1, ADDR + 4), g, ADDR, 1 << 20, None), 'layer 0: dw_folded must be 16-byte aligned'),
                     (lambda: back(d, 1, g, _grads(1, ADDR + 2), ADDR, 1 << 20, None), 'layer 0: db_folded must be 4-byte aligned')):
        rc = call()
        assert rc == _lib.ERR_ARG and text in L.srcnn_last_error().decode(), (rc, text, L.srcnn_last_error())


def test_a_deconvolution_bias_gradient_is_not_taken(L):
    d = _layer(1, n_parts=1, kind=_lib.TRAIN_FOLD_DECONV2X2, KH=2, KW=2, rows=(0, 40), bias=(1, None))
    rc = L.srcnn_train_weights_fold_backward(d, 1, _grads(1), _grads(1), ADDR, 1 << 20, None)
    assert rc == _lib.ERR_ARG and 'layer 0: db_folded of a deconvolution is not taken' in L.srcnn_last_error().decode()


def test_a_small_workspace_is_refused(L):
    for n, nbytes in ((1, 255), (2, 511), (25, 25 * RECORD)):
        d = _layer(n)
        assert L.srcnn_train_weights_fold(d, n, ADDR, nbytes, None) == _lib.ERR_WORKSPACE
        assert 'workspace too small' in L.srcnn_last_error().decode()
        assert L.srcnn_train_weights_fold_backward(d, n, _grads(n), _grads(n), ADDR, nbytes, None) == _lib.ERR_WORKSPACE
        assert 'workspace too small' in L.srcnn_last_error().decode()


def test_a_backward_without_gradients_launches_nothing(L):
    # (ADDR is no device memory: a launch would fault)
    assert L.srcnn_train_weights_fold_backward(_layer(3), 3, _grads(3, None), _grads(3, None), ADDR, 1 << 20, None) == _lib.OK


def test_device_fold_needs_prepared_weights():
    from stereo_rcnn_amd import training
    with pytest.raises(ValueError, match='prepared_weights'):
        training.train_step(None, None, None, None, prepared_weights=False, device_fold=True)


def test_trainval_net_flags():
    from stereo_rcnn_amd import trainval_net
    base = ['--kitti-path', 'k', '--split', 's']
    a = trainval_net.parse_args(base)
    assert a.device_fold is False and a.prepared_weights is False
    a = trainval_net.parse_args(base + ['--prepared-weights'])
    assert a.device_fold is False and a.prepared_weights is True
    a = trainval_net.parse_args(base + ['--device-fold'])
    assert a.device_fold is True and a.prepared_weights is True             # implied
