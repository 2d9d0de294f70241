"""CPU: the C ABI of the guarded optimiser pair as the header-derived binding sees it (include/srcnn_hip.h, "optimiser step over
accumulated gradients, skipped when not finite" -> stereo_rcnn_amd._lib): the one header declares its two entries, they bind,
every refusal comes before the first launch (so it is checkable without a GPU -- the pattern of tests/test_optim_abi_cpu.py), and
the Python keywords that reach it (SGD.step's guard / grad_scale, train_step's accum_steps / guard) refuse what they must."""
import ctypes
import glob
import inspect
import os

import pytest

from stereo_rcnn_amd import _lib

NEW = ['srcnn_grad_norm_guarded', 'srcnn_sgd_step_guarded']
P = 4096            # a non-null, 16-byte aligned "device pointer" (never dereferenced: every call below is refused first)
BIG = 1 << 40
INF = float('inf')
NAN = float('nan')


def test_the_entries_are_declared_by_the_one_header():
    assert set(NEW) <= set(_lib.declared_symbols())
    assert [os.path.basename(p) for p in glob.glob(os.path.join(os.path.dirname(_lib.HEADER_PATH), '*.h'))] == ['srcnn_hip.h']
    text = open(_lib.HEADER_PATH).read()
    # the arithmetic is stated as the header states srcnn_sgd_step's
    for phrase in ("g' = g * grad_scale", 'out[2] = out[0] is finite', 'momentum * 0 + d', 'overflow'):
        assert phrase in text, phrase


def test_signatures():
    S = _lib._SIGNATURES
    I, F, V, Z = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    hp, hl, hf, hi = ctypes.POINTER(V), ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(F), ctypes.POINTER(I)
    assert S['srcnn_grad_norm_guarded'] == (I, [hp, hl, I, F, F, V, V, Z, V])
    assert S['srcnn_sgd_step_guarded'] == (I, [hp, hp, hp, hl, hf, hf, hi, I, F, I, F, V, V, V, V])
    # the plain pair's arguments in the plain pair's order, the new ones put in: grad_scale; grad_scale, ok, skipped
    plain_norm, plain_step = S['srcnn_grad_norm'][1], S['srcnn_sgd_step'][1]
    assert S['srcnn_grad_norm_guarded'][1] == plain_norm[:4] + [F] + plain_norm[4:]
    assert S['srcnn_sgd_step_guarded'][1] == plain_step[:10] + [F] + plain_step[10:11] + [V, V] + plain_step[11:]


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    return _lib.lib()


def _refused(L, rc, text, code=None):
    assert rc == (_lib.ERR_ARG if code is None else code), rc
    assert text in L.srcnn_last_error(), L.srcnn_last_error()


def _ptrs(*v):
    return (ctypes.c_void_p * len(v))(*v)


def _ll(*v):
    return (ctypes.c_longlong * len(v))(*v)


def _f(*v):
    return (ctypes.c_float * len(v))(*v)


def _i(*v):
    return (ctypes.c_int * len(v))(*v)


def test_symbols_resolve(L):
    for name in NEW:
        assert getattr(L, name).argtypes == _lib._SIGNATURES[name][1]


def test_grad_norm_guarded_refusals(L):
    f = L.srcnn_grad_norm_guarded   # (g_host, numel_host, n_tensors, clip_norm, grad_scale, out, workspace, workspace_bytes, stream)
    _refused(L, f(None, _ll(8), 1, 10.0, 1.0, P, P, BIG, None), b'null')
    _refused(L, f(_ptrs(P), None, 1, 10.0, 1.0, P, P, BIG, None), b'null')
    _refused(L, f(_ptrs(P), _ll(8), 0, 10.0, 1.0, P, P, BIG, None), b'n_tensors')
    _refused(L, f(_ptrs(P), _ll(-1), 1, 10.0, 1.0, P, P, BIG, None), b'negative numel')
    _refused(L, f(_ptrs(P, None), _ll(8, 8), 2, 10.0, 1.0, P, P, BIG, None), b'null gradient')
    _refused(L, f(_ptrs(P, P + 2), _ll(8, 8), 2, 10.0, 1.0, P, P, BIG, None), b'aligned')
    for clip in (0.0, -1.0, NAN, -INF):
        _refused(L, f(_ptrs(P), _ll(8), 1, clip, 1.0, P, P, BIG, None), b'clip_norm')
    for scale in (0.0, -0.5, INF, NAN):
        _refused(L, f(_ptrs(P), _ll(8), 1, 10.0, scale, P, P, BIG, None), b'grad_scale')
    _refused(L, f(_ptrs(P), _ll(8), 1, 10.0, 1.0, None, P, BIG, None), b'null out')
    _refused(L, f(_ptrs(P), _ll(8), 1, 10.0, 1.0, P, None, BIG, None), b'null out')
    _refused(L, f(_ptrs(P), _ll(8), 1, 10.0, 1.0, P + 2, P, BIG, None), b'aligned')
    need = L.srcnn_grad_norm_workspace_bytes(1, _ll(1 << 20))
    _refused(L, f(_ptrs(P), _ll(1 << 20), 1, 10.0, 1.0, P, P, need - 1, None), b'workspace too small', code=_lib.ERR_WORKSPACE)
    # + infinity is "do not clip" and passes the argument checks: the next refusal is the workspace's
    _refused(L, f(_ptrs(P), _ll(1 << 20), 1, INF, 0.5, P, P, need - 1, None), b'workspace too small', code=_lib.ERR_WORKSPACE)
    _refused(L, f(_ptrs(P), _ll(1 << 62), 1, 10.0, 1.0, P, P, BIG, None), b'too many chunks')


def test_sgd_step_guarded_refusals(L):
    f = L.srcnn_sgd_step_guarded    # (p, g, m, numel, lr, wd, clipped, n_tensors, momentum, first_step, grad_scale, coef, ok, skipped, stream)
    one, n8, lr, wd, cl = _ptrs(P), _ll(8), _f(0.1), _f(0.0), _i(1)
    _refused(L, f(None, one, one, n8, lr, wd, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'null')
    _refused(L, f(one, None, one, n8, lr, wd, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'null')
    _refused(L, f(one, one, one, None, lr, wd, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'null')
    _refused(L, f(one, one, one, n8, None, wd, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'null')
    _refused(L, f(one, one, one, n8, lr, None, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'null')
    _refused(L, f(one, one, one, n8, lr, wd, cl, 0, 0.9, 0, 1.0, None, P, None, None), b'n_tensors')
    _refused(L, f(one, one, one, _ll(-8), lr, wd, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'negative numel')
    _refused(L, f(one, one, one, n8, lr, wd, cl, 1, -0.5, 0, 1.0, None, P, None, None), b'momentum')
    _refused(L, f(one, one, None, n8, lr, wd, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'm_host')
    _refused(L, f(one, one, _ptrs(None), n8, lr, wd, cl, 1, 0.9, 1, 1.0, None, P, None, None), b'null momentum buffer')
    _refused(L, f(_ptrs(None), one, one, n8, lr, wd, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'null parameter')
    _refused(L, f(one, _ptrs(None), one, n8, lr, wd, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'null gradient')
    _refused(L, f(_ptrs(P + 2), one, one, n8, lr, wd, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'aligned')
    _refused(L, f(one, _ptrs(P + 1), one, n8, lr, wd, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'aligned')
    _refused(L, f(one, one, _ptrs(P + 3), n8, lr, wd, cl, 1, 0.9, 0, 1.0, None, P, None, None), b'aligned')
    for scale in (0.0, -1.0, INF, NAN):
        _refused(L, f(one, one, one, n8, lr, wd, cl, 1, 0.9, 0, scale, None, P, None, None), b'grad_scale')
    _refused(L, f(one, one, one, n8, lr, wd, cl, 1, 0.9, 0, 1.0, P + 2, P, None, None), b'coef')
    _refused(L, f(one, one, one, n8, lr, wd, cl, 1, 0.9, 0, 1.0, None, None, None, None), b'ok')
    _refused(L, f(one, one, one, n8, lr, wd, cl, 1, 0.9, 0, 1.0, None, P + 2, None, None), b'ok')
    _refused(L, f(one, one, one, n8, lr, wd, cl, 1, 0.9, 0, 1.0, None, P, P + 2, None), b'skipped')
    two = _ptrs(P, P + 64)
    _refused(L, f(two, _ptrs(P, None), two, _ll(8, 8), _f(0.1, 0.1), _f(0, 0), _i(1, 1), 2, 0.9, 0, 1.0, None, P, P, None), b'null gradient')


def test_python_keywords():
    import torch
    from stereo_rcnn_amd import optim, training
    step = inspect.signature(optim.SGD.step).parameters
    assert list(step)[:4] == ['self', 'clip_norm', 'clip_params', 'closure']
    assert step['guard'].kind is inspect.Parameter.KEYWORD_ONLY and step['guard'].default is False
    assert step['grad_scale'].kind is inspect.Parameter.KEYWORD_ONLY and step['grad_scale'].default == 1.0
    ts = inspect.signature(training.train_step).parameters
    assert ts['accum_steps'].default == 1 and ts['guard'].default is False
    assert list(ts)[:4] == ['model', 'optimizer', 'uncert', 'batch']
    w = torch.zeros(4, requires_grad=True)
    opt = optim.SGD([w], lr=0.1, momentum=0.9)
    assert opt.skipped_steps is None and 'skipped_steps' not in opt.state_dict()
    w.grad = torch.ones(4)
    for bad in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError, match='grad_scale'):
            opt.step(grad_scale=bad)
    assert not opt.state                                        # refused before a momentum buffer was made
    with pytest.raises(NotImplementedError):                    # CPU tensors: as the plain step
        opt.step(guard=True)
    with pytest.raises(NotImplementedError):
        optim.grad_norm_guarded([torch.ones(3)], 10.0)
    for n in (0, -2):
        with pytest.raises(ValueError, match='accum_steps'):
            training.train_step(None, None, None, None, accum_steps=n)
    with pytest.raises(ValueError, match='sequence of 3'):
        training.train_step(None, None, None, [(), ()], accum_steps=3)
