"""GPU: srcnn_conv2d_backward_f16x3 (dx, dw on the f16 MFMA by the 3 x f16 split, per-tensor power-of-two scales found on the
device; stereo_rcnn_amd/csrc/conv_backward_f16x3.hip) through engine.conv2d_backward(precision='f16x3'), against float64 torch
autograd on the same float32 inputs (tests/conv_backward_ref.py).

The first assertion per element is the DERIVED bound of tests/conv_backward_f16x3_ref.py (db: the fp32 pass's bound,
conv_backward_ref.bound -- it is that pass); tests/conv_backward_f16x3_tolerances.py holds twice the measured max |err| / max |ref|
on top, the fp32 backward's value for the same case beside it.  Outputs are pre-filled with NaN inside sentinel guards: an element
left unwritten shows as NaN, a write outside the tensor changes a sentinel.  The cases (conv_backward_f16x3_ref.CASES) are the
smallest at which each path can go wrong.
"""
import itertools

import pytest
import torch

import conv_backward_f16x3_ref as R3
import conv_backward_f16x3_tolerances as CT
import conv_backward_ref as R
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


class Case(object):
    """Inputs on the device, the float64 reference (computed once) and the engine's weights of one case."""

    def __init__(self, name, engine, dev, dy_full=None):
        c = R3.make_case(name)
        self.c, self.name = c, name
        dy_full = c['dy_full'] if dy_full is None else dy_full
        cin, cout = c['cin'], c['cout']
        self.x, self.dy_full = c['x'].to(dev), dy_full.to(dev)
        self.y = None if c['y32'] is None else c['y32'].to(dev)
        self.cw = engine.ConvW(c['w'].to(dev), None, c['k'], c['k'], c['stride'], c['pad'], c['relu'])
        dy = dy_full[..., c['yco']:c['yco'] + cout].contiguous()
        self.ref = R.conv_backward(c['x'][..., :cin].contiguous(), c['w'], dy, c['stride'], c['pad'], y32=c['y32'], relu=c['relu'])
        self.M = c['B'] * c['OH'] * c['OW']
        self.k_terms = {'dx': c['k'] ** 2 * cout, 'dw': self.M, 'db': self.M}
        self.shapes = {'dx': (c['B'], c['H'], c['W'], c['xcs']), 'dw': (cout, c['k'], c['k'], cin), 'db': (cout,)}
        self.amax = float(self.ref['g'].abs().max())
        self.bmax = {'dx': float(c['w'].abs().max()), 'dw': float(c['x'][..., :cin].abs().max())}

    def run(self, engine, want=('dx', 'dw', 'db'), splits=0, tile=None, g_out=None, precision='f16x3'):
        c = self.c
        bufs = {}
        for n in want:
            numel = 1
            for v in self.shapes[n]:
                numel *= v
            buf = torch.full((numel + 2 * GUARD,), SENTINEL, device=self.x.device)
            view = buf[GUARD:GUARD + numel].view(self.shapes[n])
            view[...] = float('nan')
            if n == 'dx' and c['xcs'] > c['cin']:
                view[..., c['cin']:] = SENTINEL                      # floats beyond Cin must be left alone
            bufs[n] = (buf, view)
        engine.conv2d_backward(self.cw, self.x, c['B'], c['H'], c['W'], self.y, self.dy_full, c['OH'], c['OW'], want=want, splits=splits,
                               x_cstride=c['xcs'], y_cstride=c['ycs'], y_coffset=c['yco'], g_out=g_out,
                               out={n: v for n, (_, v) in bufs.items()}, tile=tile, precision=precision)
        torch.cuda.synchronize()
        res = {}
        for n, (buf, view) in bufs.items():
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), '%s: stray write' % n
            got = view.cpu()
            if n == 'dx' and c['xcs'] > c['cin']:
                assert bool((got[..., c['cin']:] == SENTINEL).all()), 'dx: floats beyond Cin were written'
                got = got[..., :c['cin']].contiguous()
            res[n] = got
        return res

    def check(self, res, splits, label):
        """The derived per-element bound; returns the normalised errors."""
        norm = {}
        for n, got in res.items():
            ref, S = self.ref[n], self.ref['S_' + n]
            assert not bool(torch.isnan(got).any()), '%s %s: %d elements NaN (left unwritten?)' % (label, n, int(torch.isnan(got).sum()))
            err = (got.double() - ref).abs()
            if n == 'db':
                lim = R.bound(self.k_terms[n], 0, S)
            else:
                lim = R3.bound(self.k_terms[n], (splits or 64) if n == 'dw' else 0, S, self.amax, self.bmax[n])
            worst = float((err / lim).max())
            norm[n] = float(err.max() / ref.abs().max())
            print('%s %s: max err / bound %.4f, normalised %.3e' % (label, n, worst, norm[n]))
            assert worst <= 1.0, (label, n, worst, int((err > lim).sum()))
        return norm


_cases = {}


def _case(name, engine, dev):
    if name not in _cases:
        _cases[name] = Case(name, engine, dev)
        _cases[name].full = _cases[name].run(engine)
    return _cases[name]


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('name', sorted(R3.CASES))
def test_gradients_meet_the_derived_bound(m, dev, name):
    c = _case(name, m, dev)
    norm = c.check(c.full, 0, name)
    fp32 = c.run(m, precision='f32')
    for n, v in norm.items():
        key = 'conv_bwd_f16x3_%s_%s' % (name, n)
        observe(key, v)
        f = observe('conv_bwd_f16x3_fp32_%s_%s' % (name, n), float((fp32[n].double() - c.ref[n]).abs().max() / c.ref[n].abs().max()))
        print('%s %s: f16x3 %.3e, fp32 backward %.3e' % (name, n, v, f))
        lim = CT.LIMITS.get(key)
        if lim is not None:
            assert v <= lim, (name, n, v, lim)
    assert _bits_equal(c.full['db'], fp32['db'])                # the same pass
    if name.startswith('stride2'):       # input pixels no output pixel reads through any tap: written, and exactly 0
        dx, ref = c.full['dx'], c.ref['S_dx']
        never = ref == 0
        assert bool(never.any()) == (name == 'stride2_1x1')
        assert float(dx[never].abs().max() if never.any() else 0.0) == 0.0
        if name == 'stride2_1x1':
            assert float(dx[:, 1::2].abs().max()) == 0.0 and float(dx[:, :, 1::2].abs().max()) == 0.0
    if name == 'ragged_3x3':            # y == 0 masks like a negative: those g are 0, and g_out says so exactly
        g = torch.full((c.c['B'], c.c['OH'], c.c['OW'], c.c['cout']), float('nan'), device=dev)
        c.run(m, want=('db',), g_out=g)
        assert torch.equal(g.cpu().double(), c.ref['g']) and bool((g.cpu()[c.c['y32'] == 0] == 0).all())


def test_repeatable(m, dev):
    for name in sorted(R3.CASES):
        c = _case(name, m, dev)
        again = c.run(m)
        for n in ('dx', 'dw', 'db'):
            assert _bits_equal(again[n], c.full[n]), (name, n)


@pytest.mark.parametrize('splits', [3, 1])
def test_forced_split(m, dev, splits):
    c = _case('forced_split', m, dev)
    a = c.run(m, want=('dw',), splits=splits)
    c.check(a, splits, 'forced_split splits=%d' % splits)
    b = c.run(m, want=('dw',), splits=splits)
    assert _bits_equal(a['dw'], b['dw'])


@pytest.mark.parametrize('tile', [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_tiles(m, dev, tile):
    c = _case('ragged_3x3', m, dev)
    c.check(c.run(m, want=('dx', 'dw'), tile=tile), 0, 'ragged_3x3 tile=%s' % (tile,))


def test_every_combination_of_null_outputs(m, dev):
    c = _case('ragged_3x3', m, dev)
    shape = (c.c['B'], c.c['OH'], c.c['OW'], c.c['cout'])
    g_full = torch.full(shape, float('nan'), device=dev)
    c.run(m, want=('db',), g_out=g_full)
    g32 = torch.full(shape, float('nan'), device=dev)
    fp32 = c.run(m, want=('db',), g_out=g32, precision='f32')
    assert _bits_equal(g_full, g32) and _bits_equal(c.full['db'], fp32['db'])
    names = ('dx', 'dw', 'db', 'g_out')
    for r in range(1, 5):
        for combo in itertools.combinations(names, r):
            g = torch.full(shape, float('nan'), device=dev) if 'g_out' in combo else None
            res = c.run(m, want=tuple(n for n in combo if n != 'g_out'), g_out=g)
            for n, got in res.items():
                assert _bits_equal(got, c.full[n]), (combo, n)
            if g is not None:
                assert _bits_equal(g, g_full), combo


@pytest.mark.parametrize('power', [-40, 30])
def test_range_exact(m, dev, power):
    """dy times 2^power: dx, dw and db are the unscaled results times that power, bit for bit -- the scale follows the tensor."""
    base = _case('ragged_3x3', m, dev)
    f = 2.0 ** power
    scaled = Case('ragged_3x3', m, dev, dy_full=base.c['dy_full'] * f)
    res = scaled.run(m)
    for n in ('dx', 'dw', 'db'):
        assert _bits_equal(res[n], base.full[n] * f), (power, n)


def test_range_within_a_tensor(m, dev):
    """One element of dy 2^12 larger than the rest: the derived bound alone judges it."""
    base = _case('ragged_3x3', m, dev)
    dy = base.c['dy_full'].clone()
    pos = (base.c['y32'] > 0).nonzero()[7]                       # an element the mask keeps
    dy[tuple(int(v) for v in pos)] = 2.0 ** 12 * float(dy.abs().max())
    c = Case('ragged_3x3', m, dev, dy_full=dy)
    assert c.amax >= 2.0 ** 11 * float(base.amax)
    c.check(c.run(m), 0, 'ragged_3x3 with one large element')


def test_all_zero_gradient(m, dev):
    base = _case('ragged_3x3', m, dev)
    c = Case('ragged_3x3', m, dev, dy_full=torch.zeros_like(base.c['dy_full']))
    res = c.run(m)
    for n in ('dx', 'dw', 'db'):
        assert bool(torch.isfinite(res[n]).all()) and float(res[n].abs().max()) == 0.0, n
