"""CPU: the C ABI of the once-per-step weight preparation as the header-derived binding sees it (include/srcnn_hip.h, "weights
prepared once per step" -> stereo_rcnn_amd._lib): the descriptor's documented field order, the four entries' signatures, the
workspace query's growth.  The descriptor's layout against the C compiler's is tests/test_abi_header_cpu.py's, with every structure."""
import ctypes
import glob
import os

import pytest

from stereo_rcnn_amd import _lib

FIELDS = ['w', 'w_amax', 'w_hi', 'w_lo', 'wt_hi', 'wt_lo', 'Cout', 'KH', 'KW', 'Cin']
P, Z, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def test_descriptor_field_order():
    assert [f[0] for f in _lib.TrainWeightDesc._fields_] == FIELDS
    assert [f[1] for f in _lib.TrainWeightDesc._fields_] == [P] * 6 + [I] * 4
    assert ctypes.sizeof(_lib.TrainWeightDesc) == 6 * 8 + 4 * 4


def test_signatures():
    S = _lib._SIGNATURES
    desc = ctypes.POINTER(_lib.TrainWeightDesc)
    assert S['srcnn_train_weights_workspace_bytes'] == (Z, [I])
    assert S['srcnn_train_weights_prepare'] == (I, [desc, I, P, Z, P])
    fwd, bwd = ctypes.POINTER(_lib.ConvFwdF16x3Desc), ctypes.POINTER(_lib.ConvBwdDesc)
    assert S['srcnn_conv2d_forward_f16x3_prepared'] == (I, [fwd, P, P, P, P, P, Z, P, Z, P])
    assert S['srcnn_conv2d_backward_f16x3_prepared'] == (I, [bwd, P, P, P, P, Z, P, Z, P])
    # the _maxima entries with the word, the plane pair and the planes' size in between
    assert S['srcnn_conv2d_forward_f16x3_prepared'][1][:3] == S['srcnn_conv2d_forward_f16x3_maxima'][1][:3]
    assert S['srcnn_conv2d_backward_f16x3_prepared'][1][:2] == S['srcnn_conv2d_backward_f16x3_maxima'][1][:2]


def test_the_entries_are_declared_by_the_one_header():
    new = ['srcnn_conv2d_backward_f16x3_prepared', 'srcnn_conv2d_forward_f16x3_prepared', 'srcnn_train_weights_prepare',
           'srcnn_train_weights_workspace_bytes']
    assert set(new) <= set(_lib.declared_symbols())
    assert _lib.HEADER.structs['srcnn_train_weight_desc'] is _lib.TrainWeightDesc
    assert [os.path.basename(p) for p in glob.glob(os.path.join(os.path.dirname(_lib.HEADER_PATH), '*.h'))] == ['srcnn_hip.h']


RECORD, PER_BLOCK = 80, 48          # include/srcnn_hip.h: bytes of one table record, layers of one kernel-argument block


def test_a_block_of_records_fits_the_argument_block():
    assert PER_BLOCK * RECORD + 16 <= 4096


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    return _lib.lib()


def test_workspace_bytes_grow_by_one_record_per_layer(L):
    q = L.srcnn_train_weights_workspace_bytes
    rec = RECORD
    assert q(0) == 0 and q(-3) == 0
    for n in (1, 3, 4, 48, 49, 200):
        assert q(n) == -(-n * rec // 256) * 256, n


ADDR = 4096         # a non-null, 16-byte aligned "device pointer" (never dereferenced: every call below is refused first)


def _layer(**kw):
    d = (_lib.TrainWeightDesc * 1)()
    d[0].w = d[0].w_amax = d[0].w_hi = d[0].w_lo = d[0].wt_hi = d[0].wt_lo = ADDR
    d[0].Cout, d[0].KH, d[0].KW, d[0].Cin = 40, 3, 3, 64
    for k, v in kw.items():
        setattr(d[0], k, v)
    return d


@pytest.mark.parametrize('kw,n,ws,nbytes,code,text', [
    (dict(w=None), 1, ADDR, 1 << 20, 'ERR_ARG', 'layer 0: null pointer: w'),
    (dict(w_amax=None), 1, ADDR, 1 << 20, 'ERR_ARG', 'w_amax'),
    (dict(wt_hi=None), 1, ADDR, 1 << 20, 'ERR_ARG', 'null pointer: a plane'),
    (dict(w_lo=ADDR + 2), 1, ADDR, 1 << 20, 'ERR_ARG', 'aligned'),
    (dict(w=ADDR + 4), 1, ADDR, 1 << 20, 'ERR_ARG', 'aligned'),
    (dict(Cin=48), 1, ADDR, 1 << 20, 'ERR_ARG', 'multiple of 32'),
    (dict(Cout=0), 1, ADDR, 1 << 20, 'ERR_ARG', 'positive'),
    (dict(Cout=1 << 19, KH=7, KW=7, Cin=512), 1, ADDR, 1 << 20, 'ERR_ARG', '2^31'),
    ({}, 0, ADDR, 1 << 20, 'ERR_ARG', 'n_layers'),
    ({}, 1, None, 1 << 20, 'ERR_ARG', 'null workspace'),
    ({}, 1, ADDR, 255, 'ERR_WORKSPACE', 'workspace too small'),
])
def test_prepare_refuses_before_any_launch(L, kw, n, ws, nbytes, code, text):
    rc = L.srcnn_train_weights_prepare(_layer(**kw), n, ws, nbytes, None)
    assert rc == getattr(_lib, code) and text in L.srcnn_last_error().decode(), (rc, L.srcnn_last_error())
