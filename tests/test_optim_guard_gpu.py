"""GPU: the guarded optimiser pair -- srcnn_grad_norm_guarded + srcnn_sgd_step_guarded (include/srcnn_hip.h) and
optim.SGD.step(guard=..., grad_scale=...) -- against the plain pair on copies and against the float32 restatement of
tests/optim_guard_ref.py.  EVERY comparison is equality of bits; there is no tolerance in this file.

One list for every test, 65 tensors (one more than a launch takes): 1, 3, 4, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 5 and 0
elements, then 57 of 3..11 elements.  The 2 CHUNK + 5 tensor's gradient lies 4 bytes past a 16-byte boundary (the scalar path, in
the norm and in the step); the CHUNK tensor is not clipped (it is outside the norm's list, as `uncert` is); learning rates and
weight decays differ from tensor to tensor.  Every tensor is a slice of a buffer of its own with guard floats on both sides."""
import ctypes

import numpy as np
import pytest
import torch

import optim_guard_ref as G
import optim_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 12345.0
CLIP = 10.0
MOMENTUM = 0.9
MISALIGNED, UNCLIPPED, EMPTY = 6, 4, 7          # positions in _sizes()


@pytest.fixture(scope='module')
def lib(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import _lib
    _lib.lib()
    return _lib


def _sizes(lib):
    C = lib.OPT_CHUNK
    sizes = [1, 3, 4, C - 1, C, C + 1, 2 * C + 5, 0] + [3 + (i % 9) for i in range(lib.OPT_TENSORS_PER_LAUNCH + 1 - 8)]
    assert len(sizes) == 65 and sizes[MISALIGNED] == 2 * C + 5 and sizes[EMPTY] == 0 and sizes[UNCLIPPED] == C
    return sizes


def _hyper(i):
    """Per-tensor (lr, weight decay, clipped)."""
    return 0.01 * (1 + i % 3), (0.0 if i % 2 else 1e-3), i != UNCLIPPED


@pytest.fixture(scope='module')
def data(lib):
    """Host arrays, made once and never written: parameters, momentum buffers, gradients (norm of the clipped ones ~ 145)."""
    sizes = _sizes(lib)
    rng = np.random.RandomState(21)
    make = lambda: [rng.randn(n).astype(F32) for n in sizes]
    return dict(sizes=sizes, p=make(), m=make(), g=make())


def _u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


class Slot(object):
    """One device tensor inside a guard-filled buffer: 16-byte aligned, or 4 bytes past such a boundary."""

    def __init__(self, values, dev, odd=False):
        n = values.size
        self.buf = torch.full((n + 12,), GUARD, dtype=torch.float32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.off = 5 if odd else 4
        self.t = self.buf[self.off:self.off + n]
        self.t.copy_(torch.from_numpy(values))
        assert n == 0 or self.t.data_ptr() % 16 == (4 if odd else 0)

    def bits(self):
        return self.t.cpu().numpy().view(np.uint32)

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:self.off] == GUARD).all() and (b[self.off + self.t.numel():] == GUARD).all())


class Device(object):
    """The list on the device, in the order `order` (a permutation of the positions of _sizes())."""

    def __init__(self, lib, dev, data, grads=None, order=None, momentum=MOMENTUM):
        self.lib, self.dev, self.momentum = lib, dev, momentum
        self.order = list(range(len(data['sizes']))) if order is None else list(order)
        grads = data['g'] if grads is None else grads
        self.p = [Slot(data['p'][i], dev) for i in self.order]
        self.m = [Slot(data['m'][i], dev) for i in self.order]
        self.g = [Slot(grads[i], dev, odd=(i == MISALIGNED)) for i in self.order]
        self.out = torch.full((3,), GUARD, dtype=torch.float32, device=dev)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)

    def set_grads(self, grads):
        for slot, i in zip(self.g, self.order):
            slot.t.copy_(torch.from_numpy(grads[i]))

    def _lists(self, slots):
        n = len(slots)
        return ((ctypes.c_void_p * n)(*[s.t.data_ptr() for s in slots]), (ctypes.c_longlong * n)(*[s.t.numel() for s in slots]))

    def norm(self, guarded, scale=1.0, clip=CLIP):
        """The norm over the clipped tensors, in list order."""
        L = self.lib.lib()
        slots = [s for s, i in zip(self.g, self.order) if _hyper(i)[2]]
        ptrs, numel = self._lists(slots)
        nbytes = L.srcnn_grad_norm_workspace_bytes(len(slots), numel)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        if guarded:
            rc = L.srcnn_grad_norm_guarded(ptrs, numel, len(slots), clip, scale, self.out.data_ptr(), ws.data_ptr(), nbytes, self.lib.stream())
        else:
            rc = L.srcnn_grad_norm(ptrs, numel, len(slots), clip, self.out.data_ptr(), ws.data_ptr(), nbytes, self.lib.stream())
        self.lib.check(rc, 'norm')
        return self.out.cpu().numpy()

    def step(self, guarded, first, scale=1.0, count=True):
        L = self.lib.lib()
        n = len(self.order)
        p, numel = self._lists(self.p)
        g, _ = self._lists(self.g)
        m = self._lists(self.m)[0] if self.momentum != 0 else None
        lr = (ctypes.c_float * n)(*[_hyper(i)[0] for i in self.order])
        wd = (ctypes.c_float * n)(*[_hyper(i)[1] for i in self.order])
        cl = (ctypes.c_int * n)(*[int(_hyper(i)[2]) for i in self.order])
        coef = self.out.data_ptr() + 4
        if guarded:
            rc = L.srcnn_sgd_step_guarded(p, g, m, numel, lr, wd, cl, n, self.momentum, int(first), scale, coef, self.out.data_ptr() + 8,
                                          self.skipped.data_ptr() if count else None, self.lib.stream())
        else:
            rc = L.srcnn_sgd_step(p, g, m, numel, lr, wd, cl, n, self.momentum, int(first), coef, self.lib.stream())
        self.lib.check(rc, 'step')

    def bits(self):
        """({position: parameter bits}, {position: momentum buffer bits})."""
        return ({i: s.bits() for s, i in zip(self.p, self.order)}, {i: s.bits() for s, i in zip(self.m, self.order)})

    def guards_intact(self):
        return all(s.guards_intact() for s in self.p + self.m + self.g)

    def count(self):
        return int(self.skipped.cpu()[0])


def restated(data, grads, order, first, scale, momentum=MOMENTUM, p=None, m=None, clip=CLIP):
    """The restatement's (out, {position: p bits}, {position: m bits}) for the list in `order`."""
    p = data['p'] if p is None else p
    m = data['m'] if m is None else m
    out = G.grad_norm_guarded_f32([grads[i] for i in order if _hyper(i)[2]], clip, scale)
    ps, ms = {}, {}
    for i in order:
        lr, wd, clipped = _hyper(i)
        pn, mn = G.sgd_step_guarded_f32(p[i], grads[i], m[i], lr, wd, momentum, first, scale, out[2], out[1] if clipped else None)
        ps[i], ms[i] = _u32(pn), _u32(m[i] if mn is None else mn)
    return out, ps, ms


def _same(a, b):
    assert set(a) == set(b)
    return [i for i in a if not np.array_equal(a[i], b[i])] == []


def _bad_grads(data, kind):
    g = [a.copy() for a in data['g']]
    if kind == 'inf':
        g[MISALIGNED][-1] = np.inf                   # the last element of the last chunk of the misaligned tensor
    elif kind == 'nan':
        g[0][0] = np.nan                             # the first element of tensor 0
    elif kind == 'overflow':
        g[5][7] = g[5][4096] = 3e19                  # finite, but each square (9e38) is beyond float32
        assert np.isfinite(g[5]).all()
    else:
        # scaled by 0.5 each square (2.25e38) fits, the float32 sum of the two in one chunk (threads 1 and 2) does not
        assert kind == 'chunk sum overflows'
        g[5][7] = g[5][8] = 3e19
    return g


def _out_equal(want, got):
    """(norm, coefficient, ok) of the restatement and of the device: the same bits, but that a NaN norm is any NaN."""
    want = np.array(want, F32)
    if np.isnan(want[0]):
        return bool(np.isnan(got[0])) and np.array_equal(want[1:].view(np.uint32), got[1:].view(np.uint32))
    return np.array_equal(want.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('momentum', [MOMENTUM, 0.0])
def test_scale_one_is_the_plain_pair(lib, dev, data, first, momentum):
    plain, guarded = Device(lib, dev, data, momentum=momentum), Device(lib, dev, data, momentum=momentum)
    a, b = plain.norm(False), guarded.norm(True, 1.0)
    assert np.array_equal(a[:2].view(np.uint32), b[:2].view(np.uint32)) and a[2] == F32(GUARD) and b[2] == 1.0
    assert b[1] < 1.0                                # the step is clipped
    plain.step(False, first)
    guarded.step(True, first, 1.0)
    (pp, pm), (gp, gm) = plain.bits(), guarded.bits()
    assert _same(pp, gp) and _same(pm, gm)
    out, rp, rm = restated(data, data['g'], guarded.order, first, 1.0, momentum)
    assert np.array_equal(_u32(np.array(out)), b.view(np.uint32))
    assert _same(gp, rp) and _same(gm, rm)
    assert any(not np.array_equal(gp[i], _u32(data['p'][i])) for i in gp)
    assert guarded.count() == 0 and guarded.guards_intact() and plain.guards_intact()


@pytest.mark.parametrize('scale', [0.5, 0.25])
def test_scaled_gradients_follow_the_restatement(lib, dev, data, scale):
    d = Device(lib, dev, data)
    got = d.norm(True, scale)
    d.step(True, 0, scale)
    out, rp, rm = restated(data, data['g'], d.order, 0, scale)
    print('scale %g: norm %.9g, coefficient %.9g, ok %g' % (scale, got[0], got[1], got[2]))
    assert np.array_equal(_u32(np.array(out)), got.view(np.uint32)) and got[2] == 1.0
    gp, gm = d.bits()
    assert _same(gp, rp) and _same(gm, rm)
    assert all(np.array_equal(s.bits(), _u32(data['g'][i])) for s, i in zip(d.g, d.order))      # the gradients are only read
    assert d.count() == 0 and d.guards_intact()


@pytest.mark.parametrize('kind,scale', [('inf', 0.5), ('nan', 0.5), ('overflow', 1.0), ('chunk sum overflows', 0.5)])
def test_a_bad_step_is_skipped_and_counted(lib, dev, data, kind, scale):
    bad = _bad_grads(data, kind)
    d = Device(lib, dev, data, grads=bad)
    start_p, start_m = d.bits()
    for calls in (1, 2):
        out = d.norm(True, scale)
        assert out[2] == 0.0 and not np.isfinite(out[0])
        assert _out_equal(G.grad_norm_guarded_f32([bad[i] for i in d.order if _hyper(i)[2]], CLIP, scale), out)
        d.step(True, 0, scale)
        p, m = d.bits()
        assert _same(p, start_p) and _same(m, start_m)
        assert d.count() == calls
    d.set_grads(data['g'])
    out = d.norm(True, scale)
    d.step(True, 0, scale)
    want, rp, rm = restated(data, data['g'], d.order, 0, scale)
    p, m = d.bits()
    assert out[2] == 1.0 and _out_equal(want, out) and _same(p, rp) and _same(m, rm) and not _same(p, start_p)
    assert d.count() == 2 and d.guards_intact()


def test_a_bad_step_without_a_counter(lib, dev, data):
    d = Device(lib, dev, data, grads=_bad_grads(data, 'inf'))
    start_p, start_m = d.bits()
    assert d.norm(True)[2] == 0.0
    d.step(True, 0, count=False)
    p, m = d.bits()
    assert _same(p, start_p) and _same(m, start_m) and d.count() == 0 and d.guards_intact()


def test_a_bad_first_step_leaves_zero_buffers_and_the_next_step_is_the_first(lib, dev, data):
    d = Device(lib, dev, data, grads=_bad_grads(data, 'nan'))
    start_p, _ = d.bits()
    assert d.norm(True)[2] == 0.0
    d.step(True, 1)
    p, m = d.bits()
    assert _same(p, start_p) and all(not v.any() for v in m.values())               # every buffer: + 0
    assert d.count() == 1 and d.guards_intact()
    d.set_grads(data['g'])
    assert d.norm(True)[2] == 1.0
    d.step(True, 0)
    plain = Device(lib, dev, data)
    plain.norm(False)
    plain.step(False, 1)
    (gp, gm), (pp, pm) = d.bits(), plain.bits()
    assert _same(gp, pp) and _same(gm, pm)
    assert d.count() == 1 and d.guards_intact()


def test_a_permuted_list_follows_the_restatement_of_the_permuted_list(lib, dev, data):
    # (the entries have no grid argument: what can move is the list order, which the norm's summation order follows)
    order = list(np.random.RandomState(3).permutation(len(data['sizes'])))
    d = Device(lib, dev, data, order=order)
    got = d.norm(True, 0.5)
    d.step(True, 0, 0.5)
    out, rp, rm = restated(data, data['g'], order, 0, 0.5)
    assert np.array_equal(_u32(np.array(out)), got.view(np.uint32))
    gp, gm = d.bits()
    assert _same(gp, rp) and _same(gm, rm) and d.guards_intact()


def _optimizer(dev, data, momentum=MOMENTUM):
    from stereo_rcnn_amd import optim
    params = [torch.from_numpy(v).to(dev).requires_grad_(True) for v in data['p']]
    groups = [{'params': [p], 'lr': _hyper(i)[0], 'weight_decay': _hyper(i)[1]} for i, p in enumerate(params)]
    return optim.SGD(groups, lr=0.5, momentum=momentum), params, [p for i, p in enumerate(params) if _hyper(i)[2]]


def _set_grads(params, grads, dev):
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g).to(dev)


def test_sgd_guard_against_the_plain_step(lib, dev, data):
    a, pa, ca = _optimizer(dev, data)
    b, pb, cb = _optimizer(dev, data)
    rng = np.random.RandomState(5)
    for step in range(2):                            # a first step and one that reads the buffers
        grads = [rng.randn(n).astype(F32) for n in data['sizes']]
        _set_grads(pa, grads, dev), _set_grads(pb, grads, dev)
        a.step(clip_norm=CLIP, clip_params=ca)
        b.step(clip_norm=CLIP, clip_params=cb, guard=True)
        assert a.last_norm.shape == (2,) and b.last_norm.shape == (3,)
        assert np.array_equal(_u32(a.last_norm.cpu().numpy()), _u32(b.last_norm.cpu().numpy()[:2])) and float(b.last_norm[2]) == 1.0
    assert all(np.array_equal(_u32(x.detach().cpu().numpy()), _u32(y.detach().cpu().numpy())) for x, y in zip(pa, pb))
    sa, sb = a.state_dict(), b.state_dict()
    assert sa['param_groups'] == sb['param_groups'] and set(sa['state']) == set(sb['state'])
    for k in sa['state']:
        assert set(sa['state'][k]) == set(sb['state'][k]) == {'momentum_buffer'}
        assert np.array_equal(_u32(sa['state'][k]['momentum_buffer'].cpu().numpy()), _u32(sb['state'][k]['momentum_buffer'].cpu().numpy()))
    assert a.skipped_steps is None
    assert b.skipped_steps.dtype == torch.int32 and b.skipped_steps.shape == (1,) and int(b.skipped_steps) == 0
    # the counter is no part of the state: torch.optim.SGD takes the dict as it is
    other = torch.optim.SGD([{'params': [torch.zeros_like(p).requires_grad_(True)]} for p in pb], lr=0.1, momentum=0.5)
    other.load_state_dict(sb)
    assert other.param_groups[1]['lr'] == _hyper(1)[0] and other.param_groups[0]['momentum'] == MOMENTUM


def test_sgd_grad_scale_against_the_restatement(lib, dev, data):
    opt, params, clipped = _optimizer(dev, data)
    _set_grads(params, data['g'], dev)
    opt.step(clip_norm=CLIP, clip_params=clipped, grad_scale=0.5)
    order = list(range(len(data['sizes'])))
    out, rp, rm = restated(data, data['g'], order, 1, 0.5)
    assert np.array_equal(_u32(np.array(out)), _u32(opt.last_norm.cpu().numpy()))
    for i, p in enumerate(params):
        assert np.array_equal(_u32(p.detach().cpu().numpy()), rp[i]), i
        if data['sizes'][i]:
            first_m = R.sgd_step_f32(data['p'][i], (data['g'][i] * F32(0.5)).astype(F32), None, _hyper(i)[0], _hyper(i)[1], MOMENTUM, True,
                                     out[1] if _hyper(i)[2] else None)[1]
            assert np.array_equal(_u32(opt.state[p]['momentum_buffer'].cpu().numpy()), _u32(first_m)), i
    assert int(opt.skipped_steps) == 0               # a grad_scale other than 1 is guarded


def test_sgd_guard_skips_a_bad_step_clipped_or_not(lib, dev, data):
    for clip_norm in (CLIP, None):
        opt, params, clipped = _optimizer(dev, data)
        _set_grads(params, data['g'], dev)
        opt.step(clip_norm=clip_norm, clip_params=clipped, guard=True)
        ref, ref_params, ref_clipped = _optimizer(dev, data)
        _set_grads(ref_params, data['g'], dev)
        ref.step(clip_norm=clip_norm, clip_params=ref_clipped)
        assert all(np.array_equal(_u32(x.detach().cpu().numpy()), _u32(y.detach().cpu().numpy())) for x, y in zip(params, ref_params))
        if clip_norm is None:                        # the norm over every gradient with clip_norm = +inf: coefficient 1, not used
            assert float(opt.last_norm[1]) == 1.0 and float(opt.last_norm[2]) == 1.0
        before = [p.detach().clone() for p in params]
        before_m = [opt.state[p]['momentum_buffer'].clone() for p in params]
        # the unclipped tensor's gradient is outside clip_params' norm: the Inf goes where `ok` is taken from
        _set_grads(params, _bad_grads(data, 'inf'), dev)
        opt.step(clip_norm=clip_norm, clip_params=clipped, guard=True)
        assert float(opt.last_norm[2]) == 0.0 and int(opt.skipped_steps) == 1
        assert all(torch.equal(p.detach(), q) for p, q in zip(params, before))
        assert all(torch.equal(opt.state[p]['momentum_buffer'], q) for p, q in zip(params, before_m))
