"""GPU: srcnn_conv2d_forward_f16x3 (the training forward on the f16 MFMA by the 3 x f16 split, per-tensor power-of-two scales found
on the device; stereo_rcnn_amd/csrc/conv_forward_f16x3.hip) through engine.conv2d_train_f16x3, against float64 torch on the same
float32 inputs (tests/conv_forward_f16x3_ref.py).

The first assertion per element is the DERIVED bound of tests/conv_forward_f16x3_ref.py; tests/conv_forward_f16x3_tolerances.py holds
twice the measured max |err| / max |ref| on top, the exact-fp32 engine's value for the same case beside it.  y is pre-filled with
NaN inside sentinel guards, the channels of y outside the view with the sentinel, and the floats of x behind Cin are NaN: an element
left unwritten shows as NaN, a write outside the view changes a sentinel, a read behind Cin poisons the result.  The cases
(conv_forward_f16x3_ref.CASES) are the smallest at which each path can go wrong.
"""
import ctypes

import pytest
import torch

import conv_backward_f16x3_ref as R3
import conv_backward_f16x3_tolerances as BT
import conv_backward_tolerances as B32
import conv_backward_ref as RB
import conv_forward_f16x3_ref as RF
import conv_forward_f16x3_tolerances as CT
from tolerances import observe

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARD = 256


@pytest.fixture(scope='module')
def m(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import engine
    return engine


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_KEEP = object()


class Case(object):
    """Inputs on the device and the float64 reference (computed once) of one case; keyword arguments replace inputs."""

    def __init__(self, name, dev, x=None, w=None, bias=_KEEP, res=_KEEP):
        c = dict(RF.make_case(name))
        if x is not None:
            c['x'] = x
        if w is not None:
            c['w'] = w
        if bias is not _KEEP:
            c['bias'] = bias
        if res is not _KEEP:
            c['res'] = res
        self.c, self.name, self.dev = c, name, dev
        self.x, self.w = c['x'].to(dev), c['w'].to(dev)
        self.bias = None if c['bias'] is None else c['bias'].to(dev)
        self.res = None if c['res'] is None else c['res'].to(dev)
        self.ref, self.S, self.E = RF.case_reference(c)
        self.k_terms = c['k'] ** 2 * c['cin']
        self.xmax, self.wmax = float(c['x'][..., :c['cin']].abs().max()), float(c['w'].abs().max())

    def run(self, engine, tile=None, precision='f16x3'):
        c = self.c
        shape = (c['B'], c['OH'], c['OW'], c['ycs'])
        numel = shape[0] * shape[1] * shape[2] * shape[3]
        buf = torch.full((numel + 2 * GUARD,), SENTINEL, device=self.dev)
        full = buf[GUARD:GUARD + numel].view(shape)
        full[..., c['yco']:c['yco'] + c['cout']] = float('nan')
        cw = engine.ConvW(self.w, self.bias, c['k'], c['k'], c['stride'], c['pad'], c['relu'])
        if precision == 'f16x3':
            engine.conv2d_train_f16x3(cw, self.x, c['B'], c['H'], c['W'], full, c['OH'], c['OW'], residual=self.res, x_cstride=c['xcs'],
                                      y_cstride=c['ycs'], y_coffset=c['yco'], tile=tile)
        else:
            engine.conv2d(cw, self.x, c['B'], c['H'], c['W'], full, c['OH'], c['OW'], residual=self.res, x_cstride=c['xcs'],
                          y_cstride=c['ycs'], y_coffset=c['yco'], precision='f32', plan=(0, 0, 0, 0, 0))
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), 'stray write'
        got = full.cpu()
        outside = torch.ones(c['ycs'], dtype=torch.bool)
        outside[c['yco']:c['yco'] + c['cout']] = False
        assert bool((got[..., outside] == SENTINEL).all()), 'channels of y outside the view were written'
        return got[..., c['yco']:c['yco'] + c['cout']].contiguous()

    def check(self, got, label):
        """The derived per-element bound; returns the normalised error."""
        assert not bool(torch.isnan(got).any()), '%s: %d elements NaN (left unwritten, or a read behind Cin?)' % (label, int(torch.isnan(got).sum()))
        err = (got.double() - self.ref).abs()
        lim = RF.bound(self.k_terms, self.S, self.E, self.xmax, self.wmax)
        worst = float((err / lim).max())
        norm = float(err.max() / self.ref.abs().max())
        print('%s: max err / bound %.4f, normalised %.3e' % (label, worst, norm))
        assert worst <= 1.0, (label, worst, int((err > lim).sum()))
        return norm


_cases = {}


def _case(name, engine, dev):
    if name not in _cases:
        _cases[name] = Case(name, dev)
        _cases[name].y = _cases[name].run(engine)
    return _cases[name]


@pytest.mark.parametrize('name', sorted(RF.CASES))
def test_forward_meets_the_derived_bound(m, dev, name):
    c = _case(name, m, dev)
    v = c.check(c.y, name)
    key = 'conv_fwd_f16x3_%s' % name
    observe(key, v)
    fp32 = c.run(m, precision='f32')
    f = observe('conv_fwd_f16x3_fp32_%s' % name, float((fp32.double() - c.ref).abs().max() / c.ref.abs().max()))
    print('%s: f16x3 %.3e, fp32 engine %.3e' % (name, v, f))
    lim = CT.LIMITS.get(key)
    if lim is not None:
        assert v <= lim, (name, v, lim)
    if c.c['relu']:
        assert float(c.y.min()) == 0.0 and 0.2 < float((c.y > 0).float().mean()) < 0.9


def test_repeatable(m, dev):
    for name in sorted(RF.CASES):
        c = _case(name, m, dev)
        assert _bits_equal(c.run(m), c.y), name


@pytest.mark.parametrize('name', ['ragged_3x3', 'two_k_tiles_wide', 'single_k_tile'])
def test_every_tile_gives_the_same_bits(m, dev, name):
    c = _case(name, m, dev)
    for tile in ((1, 1), (1, 2), (2, 1), (2, 2)):
        assert _bits_equal(c.run(m, tile=tile), c.y), (name, tile)
    # ... and half an override (one of the two left 0) is the heuristic
    assert _bits_equal(c.run(m, tile=(2, 0)), c.y)


@pytest.mark.parametrize('name', ['ragged_3x3', 'residual_relu'])
def test_power_of_two_scaling_is_exact(m, dev, name):
    """x * 2^-40 and w * 2^20, bias and residual None: y * 2^-20 bit for bit -- each scale follows its tensor."""
    base = RF.make_case(name)
    a = Case(name, dev, bias=None, res=None)
    ya = a.run(m)
    b = Case(name, dev, x=base['x'] * 2.0 ** -40, w=base['w'] * 2.0 ** 20, bias=None, res=None)
    yb = b.run(m)
    assert float(ya.abs().max()) > 0 and _bits_equal(yb, ya * 2.0 ** -20)
    a.check(ya, name + ' without epilogue'), b.check(yb, name + ' scaled')


def test_an_element_beyond_the_float16_range(m, dev):
    base = RF.make_case('ragged_3x3')
    x = base['x'].clone()
    x[1, 3, 4, 5] = 1e5                      # above float16's 65504: the scale brings it to [2^14, 2^15)
    c = Case('ragged_3x3', dev, x=x)
    assert c.xmax == 1e5
    y = c.run(m)
    assert bool(torch.isfinite(y).all())
    c.check(y, 'ragged_3x3 with an element of 1e5')


@pytest.mark.parametrize('name', ['ragged_3x3', 'residual_relu', 'single_k_tile'])
def test_all_zero_input(m, dev, name):
    base = RF.make_case(name)
    x = torch.zeros_like(base['x'])
    x[..., base['cin']:] = float('nan')
    c = Case(name, dev, x=x)
    y = c.run(m)
    want = torch.zeros_like(y)
    if c.c['bias'] is not None:
        want = want + c.c['bias']
    if c.c['res'] is not None:
        want = want + c.c['res']
    if c.c['relu']:
        want = torch.relu(want)
    assert _bits_equal(y, want)


def test_workspace_one_byte_short(m, dev):
    """SRCNN_ERR_WORKSPACE before any launch: y keeps its fill."""
    from stereo_rcnn_amd import _lib
    L = _lib.lib()
    c = _case('ragged_3x3', m, dev).c
    x, w = c['x'].to(dev), c['w'].to(dev)
    y = torch.full((c['B'], c['OH'], c['OW'], c['cout']), SENTINEL, device=dev)
    d = _lib.ConvFwdF16x3Desc()
    d.x, d.w, d.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    d.B, d.H, d.W, d.Cin, d.x_cstride = c['B'], c['H'], c['W'], c['cin'], c['xcs']
    d.OH, d.OW, d.Cout = c['OH'], c['OW'], c['cout']
    d.KH, d.KW, d.stride, d.pad = c['k'], c['k'], c['stride'], c['pad']
    d.y_cstride, d.y_coffset = c['cout'], 0
    need = L.srcnn_conv2d_forward_f16x3_workspace_bytes(ctypes.byref(d))
    assert need > 0
    ws = torch.full((need + GUARD,), 77, dtype=torch.uint8, device=dev)
    rc = L.srcnn_conv2d_forward_f16x3(ctypes.byref(d), ws.data_ptr(), need - 1, _lib.stream())
    torch.cuda.synchronize()
    assert rc == -3 and b'workspace' in L.srcnn_last_error()
    assert bool((y == SENTINEL).all()) and bool((ws == 77).all())
    # the exact size is accepted and stays inside it
    _lib.check(L.srcnn_conv2d_forward_f16x3(ctypes.byref(d), ws.data_ptr(), need, _lib.stream()), 'srcnn_conv2d_forward_f16x3')
    torch.cuda.synchronize()
    assert bool((ws[need:] == 77).all()) and not bool(torch.isnan(y).any()) and not bool((y == SENTINEL).any())


@pytest.mark.parametrize('bp', ['f32', 'f16x3'])
def test_autograd(m, dev, bp):
    """autograd.conv2d_nhwc(forward_precision='f16x3') on ragged_3x3 with either backward: y is the direct call's bits; dx, dw, db
    against float64 autograd (masked with the forward's own y) within the backward's limits for this very case."""
    from stereo_rcnn_amd import autograd
    base = _case('ragged_3x3', m, dev)
    c = base.c
    x = c['x'][..., :c['cin']].contiguous().to(dev).requires_grad_(True)
    w = c['w'].permute(0, 3, 1, 2).contiguous().to(dev).requires_grad_(True)          # (Cout, Cin, KH, KW) as nn.Conv2d holds it
    b = c['bias'].to(dev).requires_grad_(True)
    y = autograd.conv2d_nhwc(x, w, b, c['stride'], c['pad'], relu=True, backward_precision=bp, forward_precision='f16x3')
    assert _bits_equal(y.detach().cpu(), base.y)
    bc = R3.make_case('ragged_3x3')
    assert torch.equal(bc['x'], c['x']) and torch.equal(bc['w'], c['w'])              # the backward's case, its dy
    dy = bc['dy_full']
    y.backward(dy.to(dev))
    ref = RB.conv_backward(x.detach().cpu(), c['w'], dy, c['stride'], c['pad'], y32=base.y, relu=True)
    got = {'dx': x.grad.cpu(), 'dw': w.grad.permute(0, 2, 3, 1).contiguous().cpu(), 'db': b.grad.cpu()}
    M = c['B'] * c['OH'] * c['OW']
    k_terms = {'dx': c['k'] ** 2 * c['cout'], 'dw': M, 'db': M}
    gmax, bmax = float(ref['g'].abs().max()), {'dx': base.wmax, 'dw': base.xmax}
    for n in ('dx', 'dw', 'db'):
        err = (got[n].double() - ref[n]).abs()
        if bp == 'f32' or n == 'db':         # the derived bounds of the two backwards' own tests, then their measured limits
            lim = RB.bound(k_terms[n], 64 if n == 'dw' else 0, ref['S_' + n])
        else:
            lim = R3.bound(k_terms[n], 64 if n == 'dw' else 0, ref['S_' + n], gmax, bmax[n])
        assert float((err / lim).max()) <= 1.0, (bp, n, float((err / lim).max()))
        v = float(err.max() / ref[n].abs().max())
        table = BT.LIMITS['conv_bwd_f16x3_ragged_3x3_' + n] if bp == 'f16x3' else B32.LIMITS['conv_bwd_ragged_3x3_' + n]
        print('autograd %s %s: %.3e (limit %.3e)' % (bp, n, v, table))
        observe('conv_fwd_f16x3_autograd_%s_%s' % (bp, n), v)
        assert v <= table, (bp, n, v, table)
