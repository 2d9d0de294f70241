"""CPU: the optimiser entry points of csrc/optim.hip (srcnn_grad_norm, srcnn_grad_scale, srcnn_sgd_step) validate every argument
before their first launch (include/srcnn_hip.h, "training: optimiser step"), so each refusal is checkable on a host without a GPU
-- the pattern of tests/test_train_ops_abi_cpu.py.  No call here reaches a launch.  The Python optimiser refuses CPU tensors and
what it does not implement."""
import ctypes
import os

import pytest

P = 4096            # a non-null, 16-byte aligned "device pointer" (never dereferenced: every call below is refused first)
BIG = 1 << 40


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import _lib
    return _lib.lib()


def _refused(L, rc, text, code=-1):
    assert rc == code, rc
    assert text in L.srcnn_last_error(), L.srcnn_last_error()


def _ptrs(*v):
    return (ctypes.c_void_p * len(v))(*v)


def _ll(*v):
    return (ctypes.c_longlong * len(v))(*v)


def _f(*v):
    return (ctypes.c_float * len(v))(*v)


def _i(*v):
    return (ctypes.c_int * len(v))(*v)


def test_version_and_constants(L):
    from stereo_rcnn_amd import _lib
    assert L.srcnn_version() >= 300
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'srcnn_hip.h')).read()
    assert '#define SRCNN_OPT_CHUNK %d\n' % _lib.OPT_CHUNK in header
    assert '#define SRCNN_OPT_TENSORS_PER_LAUNCH %d\n' % _lib.OPT_TENSORS_PER_LAUNCH in header
    assert 'training: optimiser step' in header
    # the list of one launch travels in the kernel's arguments: 48 bytes per tensor and the chunk table within HIP's 4096
    assert _lib.OPT_TENSORS_PER_LAUNCH * (48 + 4) + 64 <= 4096


def test_workspace_query_grows_with_the_chunk_count(L):
    from stereo_rcnn_amd import _lib
    C = _lib.OPT_CHUNK
    q = L.srcnn_grad_norm_workspace_bytes
    assert q(1, _ll(0)) >= 4                        # a list without elements still gets its one slot
    assert q(1, _ll(1)) >= 4 and q(1, _ll(C)) == q(1, _ll(1))
    sizes = [q(1, _ll(n * 64 * C)) for n in range(1, 6)]
    assert sizes == [n * 64 * 4 for n in range(1, 6)], sizes          # one float per chunk (256-byte granules)
    assert q(1, _ll(64 * C + 1)) > q(1, _ll(64 * C))
    # chunks are per tensor: 64 tensors of C + 1 elements are 128 chunks, one tensor of 64 * (C + 1) elements is 65
    assert q(64, _ll(*([C + 1] * 64))) == 128 * 4 and q(1, _ll(64 * (C + 1))) == 512
    assert q(0, _ll(1)) == 0 and q(1, None) == 0 and q(1, _ll(-1)) == 0


def test_grad_norm_refusals(L):
    f = L.srcnn_grad_norm           # (g_host, numel_host, n_tensors, clip_norm, out, workspace, workspace_bytes, stream)
    _refused(L, f(None, _ll(8), 1, 10.0, P, P, BIG, None), b'null')
    _refused(L, f(_ptrs(P), None, 1, 10.0, P, P, BIG, None), b'null')
    _refused(L, f(_ptrs(P), _ll(8), 0, 10.0, P, P, BIG, None), b'n_tensors')
    _refused(L, f(_ptrs(P), _ll(8), -1, 10.0, P, P, BIG, None), b'n_tensors')
    _refused(L, f(_ptrs(P), _ll(-1), 1, 10.0, P, P, BIG, None), b'negative numel')
    _refused(L, f(_ptrs(P, None), _ll(8, 8), 2, 10.0, P, P, BIG, None), b'null gradient')
    _refused(L, f(_ptrs(P, P + 2), _ll(8, 8), 2, 10.0, P, P, BIG, None), b'aligned')
    _refused(L, f(_ptrs(P), _ll(8), 1, 0.0, P, P, BIG, None), b'clip_norm')
    _refused(L, f(_ptrs(P), _ll(8), 1, -1.0, P, P, BIG, None), b'clip_norm')
    _refused(L, f(_ptrs(P), _ll(8), 1, 10.0, None, P, BIG, None), b'null out')
    _refused(L, f(_ptrs(P), _ll(8), 1, 10.0, P, None, BIG, None), b'null out')
    need = L.srcnn_grad_norm_workspace_bytes(1, _ll(1 << 20))
    _refused(L, f(_ptrs(P), _ll(1 << 20), 1, 10.0, P, P, need - 1, None), b'workspace too small', code=-3)
    _refused(L, f(_ptrs(P), _ll(1 << 62), 1, 10.0, P, P, BIG, None), b'too many chunks')


def test_grad_scale_refusals(L):
    f = L.srcnn_grad_scale          # (g_host, numel_host, n_tensors, coef, stream)
    _refused(L, f(None, _ll(8), 1, P, None), b'null')
    _refused(L, f(_ptrs(P), None, 1, P, None), b'null')
    _refused(L, f(_ptrs(P), _ll(8), 0, P, None), b'n_tensors')
    _refused(L, f(_ptrs(P), _ll(-3), 1, P, None), b'negative numel')
    _refused(L, f(_ptrs(None), _ll(8), 1, P, None), b'null gradient')
    _refused(L, f(_ptrs(P + 1), _ll(8), 1, P, None), b'aligned')
    _refused(L, f(_ptrs(P), _ll(8), 1, None, None), b'coef')


def test_sgd_step_refusals(L):
    f = L.srcnn_sgd_step            # (p, g, m, numel, lr, wd, clipped, n_tensors, momentum, first_step, coef, stream)
    one, n8, lr, wd, cl = _ptrs(P), _ll(8), _f(0.1), _f(0.0), _i(1)
    _refused(L, f(None, one, one, n8, lr, wd, cl, 1, 0.9, 0, None, None), b'null')
    _refused(L, f(one, None, one, n8, lr, wd, cl, 1, 0.9, 0, None, None), b'null')
    _refused(L, f(one, one, one, None, lr, wd, cl, 1, 0.9, 0, None, None), b'null')
    _refused(L, f(one, one, one, n8, None, wd, cl, 1, 0.9, 0, None, None), b'null')
    _refused(L, f(one, one, one, n8, lr, None, cl, 1, 0.9, 0, None, None), b'null')
    _refused(L, f(one, one, one, n8, lr, wd, cl, 0, 0.9, 0, None, None), b'n_tensors')
    _refused(L, f(one, one, one, n8, lr, wd, cl, -2, 0.9, 0, None, None), b'n_tensors')
    _refused(L, f(one, one, one, _ll(-8), lr, wd, cl, 1, 0.9, 0, None, None), b'negative numel')
    _refused(L, f(one, one, one, n8, lr, wd, cl, 1, -0.5, 0, None, None), b'momentum')
    _refused(L, f(one, one, None, n8, lr, wd, cl, 1, 0.9, 0, None, None), b'm_host')                  # momentum != 0 needs buffers
    _refused(L, f(one, one, _ptrs(None), n8, lr, wd, cl, 1, 0.9, 1, None, None), b'null momentum buffer')
    _refused(L, f(_ptrs(None), one, one, n8, lr, wd, cl, 1, 0.9, 0, None, None), b'null parameter')
    _refused(L, f(one, _ptrs(None), one, n8, lr, wd, cl, 1, 0.9, 0, None, None), b'null gradient')
    _refused(L, f(_ptrs(P + 2), one, one, n8, lr, wd, cl, 1, 0.9, 0, None, None), b'aligned')
    _refused(L, f(one, _ptrs(P + 1), one, n8, lr, wd, cl, 1, 0.9, 0, None, None), b'aligned')
    _refused(L, f(one, one, _ptrs(P + 3), n8, lr, wd, cl, 1, 0.9, 0, None, None), b'aligned')
    _refused(L, f(one, one, one, n8, lr, wd, cl, 1, 0.9, 0, P + 2, None), b'coef')
    # the second entry of a list is checked as the first is
    two = _ptrs(P, P + 64)
    _refused(L, f(two, _ptrs(P, None), two, _ll(8, 8), _f(0.1, 0.1), _f(0, 0), _i(1, 1), 2, 0.9, 0, None, None), b'null gradient')


def test_python_optimizer_refusals():
    import torch
    from stereo_rcnn_amd import optim
    from stereo_rcnn_amd.model.utils import net_utils
    w = torch.zeros(4, requires_grad=True)
    with pytest.raises(ValueError):
        optim.SGD([w], lr=0.1, momentum=0.9, nesterov=True)
    with pytest.raises(ValueError):
        optim.SGD([w], lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError):
        optim.SGD([w], lr=0.1, maximize=True)
    with pytest.raises(ValueError):
        optim.SGD([w], lr=-1.0)
    opt = optim.SGD([w], lr=0.1, momentum=0.9, weight_decay=1e-4)
    assert opt.step() is None                        # no gradient anywhere: nothing to do, as torch
    w.grad = torch.ones(4)
    with pytest.raises(NotImplementedError):
        opt.step()
    with pytest.raises(NotImplementedError):
        opt.step(clip_norm=10.0)
    assert torch.equal(w.detach(), torch.zeros(4))
    with pytest.raises(NotImplementedError):
        optim.grad_norm([torch.ones(3)], 10.0)
    lin = torch.nn.Linear(3, 2)
    lin(torch.ones(1, 3)).sum().backward()
    with pytest.raises(NotImplementedError):
        net_utils.clip_gradient(lin, 10.0)
    # the groups carry torch.optim.SGD's keys: a state dict moves between the two classes
    ref = torch.optim.SGD([torch.zeros(4, requires_grad=True)], lr=0.1, momentum=0.9, weight_decay=1e-4)
    assert set(opt.state_dict()['param_groups'][0]) == set(ref.state_dict()['param_groups'][0])
    ref.load_state_dict(opt.state_dict())
    opt.load_state_dict(ref.state_dict())
    net_utils.adjust_learning_rate(opt, 0.1)
    assert abs(opt.param_groups[0]['lr'] - 0.01) < 1e-12


def test_make_optimizer_follows_the_reference_recipe():
    import torch
    from stereo_rcnn_amd import optim, training
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    from stereo_rcnn_amd.model.utils.config import cfg
    T = cfg.TRAIN
    assert (T.LEARNING_RATE, T.MOMENTUM, T.WEIGHT_DECAY, T.DOUBLE_BIAS, T.BIAS_DECAY) == (0.001, 0.9, 0.0001, False, False)
    model = resnet(('__background__', 'Car'), 50)
    model.create_architecture()
    uncert = torch.full((6,), -1.0, requires_grad=True)
    opt = training.make_optimizer(model, uncert)
    assert isinstance(opt, optim.SGD)
    names = training.trainable_parameters(model)
    assert len(opt.param_groups) == len(names) + 1
    for (key, p), g in zip(names.items(), opt.param_groups):
        assert len(g['params']) == 1 and g['params'][0] is p and g['momentum'] == 0.9
        if 'bias' in key:
            assert g['lr'] == 0.001 and g['weight_decay'] == 0, key
        else:
            assert g['lr'] == 0.001 and g['weight_decay'] == 0.0001, key
    last = opt.param_groups[-1]
    assert last['params'][0] is uncert and last['lr'] == 0.001 and last['weight_decay'] == 0 and last['momentum'] == 0.9
