"""GPU: srcnn_conv2d_backward (dx, dw, db on the fp32 MFMA; stereo_rcnn_amd/csrc/conv_backward.hip) through
engine.conv2d_backward, against float64 torch autograd on the CPU (tests/conv_backward_ref.py).

The cases are the smallest at which each mechanism can go wrong (see CASES).  Per element the assertion is the DERIVED bound
|got - ref64| <= (K_terms + splits + 8) u S + tiny (conv_backward_ref.bound): for any summation order of a K-term float32 dot
product |err| <= gamma_K S, so a violation means terms are missing, duplicated or read from the wrong place.  K_terms: KH KW Cout
for dx, the B OH OW output pixels for dw and db; `splits` is the number of K slices asked for, or 64 -- the library's ceiling --
where it chooses.  The measured maxima (max |err| / max |ref| per case) are held by tests/conv_backward_tolerances.py.
Outputs are pre-filled with NaN inside 256 floats of sentinel on both sides: an element left unwritten shows as NaN, a write
outside the tensor changes a sentinel.
"""
import pytest
import torch

import conv_backward_ref as R
import conv_backward_tolerances as CT
from tolerances import observe

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARD = 256

# name: (B, H, W, Cin, Cout, k, stride, pad, relu, (y_cstride, y_coffset) or None)
CASES = {
    'single_k_tile': (1, 7, 9, 32, 32, 1, 1, 0, False, None),          # M = 63 is a ragged tail
    'ragged_3x3': (2, 23, 37, 96, 200, 3, 1, 1, True, None),           # ragged M, N, Cout tails; border taps; ReLU mask; residual
    'stride2_1x1': (2, 15, 21, 64, 64, 1, 2, 0, False, None),          # untouched dx pixels must be written as exact 0
    'stride2_3x3': (1, 15, 22, 64, 96, 3, 2, 1, True, None),           # the divisibility test of the gather
    'rcnn_top': (3, 7, 7, 64, 128, 7, 7, 0, False, None),              # wgrad K = 3 pixels (tail only), dgrad K = 49 * 128
    'cout24': (1, 19, 31, 1024, 24, 1, 1, 0, False, None),             # K-tile tail in dgrad, M tail in wgrad
    'channel_offset': (1, 10, 16, 256, 512, 3, 1, 1, False, (1024, 512)),
    'linear': (5, 1, 1, 2048, 10, 1, 1, 0, False, None),
}
SPLIT_CASES = ('ragged_3x3', 'rcnn_top')


@pytest.fixture(scope='module')
def m(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import engine
    return engine


class Case(object):
    """Inputs, the float64 reference (computed once) and the engine's weights of one case."""

    def __init__(self, name, engine, dev):
        B, H, W, cin, cout, k, s, p, relu, lay = CASES[name]
        gen = torch.Generator().manual_seed(sum(ord(c) for c in name))
        self.name, self.geom, self.relu = name, (B, H, W), relu
        self.OH, self.OW = engine.conv_out_hw(H, W, k, k, s, p)
        self.ycs, self.yco = lay if lay else (cout, 0)
        self.cin, self.cout, self.k, self.stride, self.pad = cin, cout, k, s, p
        x = torch.randn(B, H, W, cin, generator=gen)
        w = torch.randn(cout, k, k, cin, generator=gen) / float(k * k * cin) ** 0.5
        bias = torch.randn(cout, generator=gen)
        dy_full = torch.randn(B, self.OH, self.OW, self.ycs, generator=gen)
        self.x, self.dy_full = x.to(dev), dy_full.to(dev)
        self.cw = engine.ConvW(w.to(dev), bias.to(dev), k, k, s, p, relu)
        self.y = None
        y32 = None
        if relu:            # the saved output is the engine's own float32 forward
            self.y = torch.empty(B, self.OH, self.OW, cout, device=dev)
            engine.conv2d(self.cw, self.x, B, H, W, self.y, self.OH, self.OW, precision='f32', plan=(0, 0, 0, 0, 0))
            y32 = self.y.cpu()
            assert 0.2 < float((y32 > 0).float().mean()) < 0.8
        self.ref = R.conv_backward(x, w, dy_full[..., self.yco:self.yco + cout], s, p, y32=y32, relu=relu)
        self.M = B * self.OH * self.OW
        self.k_terms = {'dx': k * k * cout, 'dw': self.M, 'db': self.M}
        self.shapes = {'dx': (B, H, W, cin), 'dw': (cout, k, k, cin), 'db': (cout,)}

    def buffers(self, names):
        """NaN-filled outputs inside sentinel guards: {name: (whole buffer, view)}."""
        out = {}
        for n in names:
            numel = 1
            for v in self.shapes[n]:
                numel *= v
            buf = torch.full((numel + 2 * GUARD,), SENTINEL, device=self.x.device)
            buf[GUARD:GUARD + numel] = float('nan')
            out[n] = (buf, buf[GUARD:GUARD + numel].view(self.shapes[n]))
        return out

    def run(self, engine, want=('dx', 'dw', 'db'), splits=0, tile=None, g_out=None):
        B, H, W = self.geom
        bufs = self.buffers(want)
        # with relu the saved output shares dy's layout in the library: both dense here
        engine.conv2d_backward(self.cw, self.x, B, H, W, self.y, self.dy_full, self.OH, self.OW, want=want, splits=splits,
                               y_cstride=self.ycs, y_coffset=self.yco, g_out=g_out, out={n: v for n, (_, v) in bufs.items()}, tile=tile)
        torch.cuda.synchronize()
        res = {}
        for n, (buf, view) in bufs.items():
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), '%s: stray write' % n
            res[n] = view.cpu()
        return res

    def check(self, res, splits, label):
        """The derived per-element bound; returns the normalised errors."""
        norm = {}
        for n, got in res.items():
            ref, S = self.ref[n], self.ref['S_' + n]
            assert not bool(torch.isnan(got).any()), '%s %s: %d elements left unwritten' % (label, n, int(torch.isnan(got).sum()))
            err = (got.double() - ref).abs()
            lim = R.bound(self.k_terms[n], (splits or 64) if n == 'dw' else 0, S)
            worst = float((err / lim).max())
            norm[n] = float(err.max() / ref.abs().max())
            print('%s %s: max err / bound %.3f, normalised %.3e' % (label, n, worst, norm[n]))
            assert worst <= 1.0, (label, n, worst, int((err > lim).sum()))
        return norm


_cases = {}


def _case(name, engine, dev):
    if name not in _cases:
        _cases[name] = Case(name, engine, dev)
        _cases[name].full = _cases[name].run(engine)
    return _cases[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_gradients_meet_the_derived_bound(m, dev, name):
    c = _case(name, m, dev)
    norm = c.check(c.full, 0, name)
    for n, v in norm.items():
        observe('conv_bwd_%s_%s' % (name, n), v)
        lim = CT.LIMITS.get('conv_bwd_%s_%s' % (name, n))
        if lim is not None:
            assert v <= lim, (name, n, v, lim)
    if name == 'stride2_1x1':       # three input pixels in four receive no contribution: written, and exactly 0
        dx = c.full['dx']
        assert float(dx[:, 1::2].abs().max()) == 0.0 and float(dx[:, :, 1::2].abs().max()) == 0.0


@pytest.mark.parametrize('name', sorted(CASES))
def test_repeatable_and_partial_requests(m, dev, name):
    c = _case(name, m, dev)
    again = c.run(m)
    for n in ('dx', 'dw', 'db'):
        assert torch.equal(again[n], c.full[n]), n
    only_dx = c.run(m, want=('dx',))
    assert list(only_dx) == ['dx'] and torch.equal(only_dx['dx'], c.full['dx'])
    dw_db = c.run(m, want=('dw', 'db'))
    assert torch.equal(dw_db['dw'], c.full['dw']) and torch.equal(dw_db['db'], c.full['db'])
    only_dw = c.run(m, want=('dw',))          # without a ReLU and with Cout % 32 == 0 this reads dy in place
    assert torch.equal(only_dw['dw'], c.full['dw'])


@pytest.mark.parametrize('splits', [1, 3, 9])
@pytest.mark.parametrize('name', SPLIT_CASES)
def test_split_k(m, dev, name, splits):
    c = _case(name, m, dev)
    a = c.run(m, want=('dw',), splits=splits)
    c.check(a, splits, '%s splits=%d' % (name, splits))
    b = c.run(m, want=('dw',), splits=splits)
    assert torch.equal(a['dw'], b['dw'])


@pytest.mark.parametrize('tile', [(1, 1), (1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize('name', ['ragged_3x3', 'stride2_3x3', 'cout24'])
def test_every_tile(m, dev, name, tile):
    """The heuristic picks the 64 x 64 tile for most of these small shapes: every instantiated tile of both GEMMs is run."""
    c = _case(name, m, dev)
    c.check(c.run(m, want=('dx', 'dw'), tile=tile), 0, '%s tile=%s' % (name, tile))


def test_masked_gradient_output_is_exact(m, dev):
    """g_out = dy * [y > 0]: the residual branch's gradient, a product with 0 or 1 -- exact."""
    c = _case('ragged_3x3', m, dev)
    B, H, W = c.geom
    g = torch.full((B, c.OH, c.OW, c.cout), float('nan'), device=dev)
    res = c.run(m, want=('db',), g_out=g)
    assert torch.equal(g.cpu().double(), c.ref['g'])
    assert torch.equal(res['db'], c.full['db'])
    only_g = torch.full_like(g, float('nan'))
    m.conv2d_backward(c.cw, c.x, B, H, W, c.y, c.dy_full, c.OH, c.OW, want=(), g_out=only_g)
    assert torch.equal(only_g, g)


def test_refusals_raise(m, dev):
    c = _case('single_k_tile', m, dev)
    B, H, W = c.geom
    with pytest.raises(RuntimeError, match='shape'):
        m.conv2d_backward(c.cw, c.x, B, H, W, None, c.dy_full, c.OH + 1, c.OW)
    with pytest.raises(RuntimeError, match='null'):
        m.conv2d_backward(c.cw, c.x, B, H, W, None, c.dy_full, c.OH, c.OW, relu=True)
