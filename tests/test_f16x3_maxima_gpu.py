"""GPU: max |x| handed from layer to layer in the 3 x f16 training calls (srcnn_conv2d_forward_f16x3_maxima,
srcnn_conv2d_backward_f16x3_maxima, srcnn_absmax; include/srcnn_hip.h) and autograd's reuse_maxima on top of them.

A scale is a function of max |x| alone and a maximum does not depend on who computed it, so every comparison here is a bit-equality:
against the plain entries' results, and of a word against torch's own maximum of the same elements.  The cases are those of
tests/conv_forward_f16x3_ref.py and tests/conv_backward_f16x3_ref.py; y is pre-filled with NaN and the channels outside its view
with a sentinel, as in tests/test_conv_forward_f16x3_gpu.py."""
import pytest
import torch

import conv_backward_f16x3_ref as R3
import conv_forward_f16x3_ref as RF

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
FLT_MAX_BITS = 0x7f7fffff
TILES = ((1, 1), (1, 2), (2, 1), (2, 2))
_KEEP = object()


@pytest.fixture(scope='module')
def m(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import engine
    return engine


def _bits(t):
    return t.contiguous().view(torch.int32)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _float_bits(v):
    return int(torch.tensor([v], dtype=torch.float32).view(torch.int32).item())


def _word(dev, bits=FLT_MAX_BITS):
    return torch.tensor([bits], dtype=torch.int32, device=dev)


def _forward(engine, c, dev, x=None, bias=_KEEP, res=_KEEP, tile=None, **words):
    """One forward call of case c (inputs replaced by the keywords); returns the stored channels of y on the host."""
    x = (c['x'] if x is None else x).to(dev)
    bias = c['bias'] if bias is _KEEP else bias
    res = c['res'] if res is _KEEP else res
    full = torch.full((c['B'], c['OH'], c['OW'], c['ycs']), SENTINEL, device=dev)
    full[..., c['yco']:c['yco'] + c['cout']] = float('nan')
    cw = engine.ConvW(c['w'].to(dev), None if bias is None else bias.to(dev), c['k'], c['k'], c['stride'], c['pad'], c['relu'])
    engine.conv2d_train_f16x3(cw, x, c['B'], c['H'], c['W'], full, c['OH'], c['OW'], residual=None if res is None else res.to(dev),
                              x_cstride=c['xcs'], y_cstride=c['ycs'], y_coffset=c['yco'], tile=tile, **words)
    got = full.cpu()
    outside = torch.ones(c['ycs'], dtype=torch.bool)
    outside[c['yco']:c['yco'] + c['cout']] = False
    assert bool((got[..., outside] == SENTINEL).all()), 'channels of y outside the view were written'
    y = got[..., c['yco']:c['yco'] + c['cout']].contiguous()
    assert not bool(torch.isnan(y).any())
    return y


def _check_y_word(word, y, label):
    want = int(_bits(y.abs().max().reshape(1)).item())
    got = int(word.cpu().item())
    print('%s: y_amax 0x%08x, max |y| 0x%08x (%.6g)' % (label, got & 0xffffffff, want, float(y.abs().max())))
    assert got == want, (label, hex(got), hex(want))


@pytest.mark.parametrize('name', sorted(RF.CASES))
def test_y_amax_is_the_maximum_of_what_the_call_stores(m, dev, name):
    c = RF.make_case(name)
    plain = _forward(m, c, dev)
    word = _word(dev)                                    # pre-filled with FLT_MAX: overwritten, not merged
    y = _forward(m, c, dev, y_amax=word)
    assert _bits_equal(y, plain), name
    _check_y_word(word, y, name)
    # ... and with the input's word given as well
    word2 = _word(dev)
    y2 = _forward(m, c, dev, x_amax=m.absmax(c['x'].to(dev), c['cin'], c['xcs']), y_amax=word2)
    assert _bits_equal(y2, plain) and int(word2.cpu().item()) == int(word.cpu().item())


@pytest.mark.parametrize('name', ['ragged_3x3', 'two_k_tiles_wide'])
def test_y_amax_with_every_tile(m, dev, name):
    c = RF.make_case(name)
    plain = _forward(m, c, dev)
    for tile in TILES:
        word = _word(dev)
        y = _forward(m, c, dev, tile=tile, y_amax=word)
        assert _bits_equal(y, plain), (name, tile)
        _check_y_word(word, y, '%s %s' % (name, tile))


def test_y_amax_of_an_all_zero_output_is_zero(m, dev):
    c = RF.make_case('single_k_tile')
    x = torch.zeros_like(c['x'])
    word = _word(dev)
    y = _forward(m, c, dev, x=x, y_amax=word)
    assert float(y.abs().max()) == 0.0 and int(word.cpu().item()) == 0


def test_padding_rows_never_enter_the_maximum(m, dev):
    """single_k_tile has M = 20 rows in a 64-row tile.  With bias -1000 and residual +1000 on one channel the stored |y| stays of
    order 1, while a tile row beyond M -- zero accumulators, no residual row -- would evaluate to |bias| = 1000."""
    c = RF.make_case('single_k_tile')
    bias = torch.zeros(c['cout'])
    bias[3] = -1000.0
    res = torch.zeros(c['B'], c['OH'], c['OW'], c['cout'])
    res[..., 3] = 1000.0
    plain = _forward(m, c, dev, bias=bias, res=res)
    for tile in (None,) + TILES:
        word = _word(dev)
        y = _forward(m, c, dev, bias=bias, res=res, tile=tile, y_amax=word)
        assert _bits_equal(y, plain)
        assert 0 < float(y.abs().max()) < 100
        _check_y_word(word, y, 'single_k_tile -1000 + 1000 %s' % (tile,))


def _never_read_pixel_case(make_case):
    """stride2_1x1 (1x1, stride 2, no pad on 9 x 11): pixel (1, 1) is scanned by the max pass and never read by the GEMM.  Returns
    the case, x with that pixel at 2^20 max |x|, and that value."""
    c = make_case('stride2_1x1')
    assert (c['k'], c['stride'], c['pad']) == (1, 2, 0)
    big = float(c['x'][..., :c['cin']].abs().max()) * 2.0 ** 20
    xa = c['x'].clone()
    xa[0, 1, 1, 0] = big
    return c, xa, big


def test_absmax_is_the_maximum(m, dev):
    for name in ('stride2_1x1', 'channel_offset', 'two_k_tiles_wide'):       # channel_offset: NaNs behind Cin, unvectorised row length
        c = RF.make_case(name)
        word = m.absmax(c['x'].to(dev), c['cin'], c['xcs'])
        assert word.dtype == torch.int32 and word.numel() == 1
        assert int(word.cpu().item()) == int(_bits(c['x'][..., :c['cin']].abs().max().reshape(1)).item()), name
    z = torch.zeros(3, 5, 32, device=dev)
    assert int(m.absmax(z).cpu().item()) == 0
    odd = torch.randn(7, 5, 33, device=dev)                                   # a row length that is no multiple of 4
    assert int(m.absmax(odd).cpu().item()) == int(_bits(odd.abs().max().reshape(1)).cpu().item())


def test_x_amax_is_used_and_means_what_the_scan_means(m, dev):
    c, xa, big = _never_read_pixel_case(RF.make_case)
    plain = _forward(m, c, dev)
    # (a) the true word: the plain call's bits
    true = m.absmax(c['x'].to(dev), c['cin'], c['xcs'])
    assert _bits_equal(_forward(m, c, dev, x_amax=true), plain)
    # (b) the word is what sets the scale: the plain call on xa scans the planted pixel, which the GEMM never reads; the call on
    # the unmodified x with that maximum as its word must give those very bits -- and they are not the plain bits, since at
    # 2^-20 of the scale the low halves fall into float16's subnormals
    ya = _forward(m, c, dev, x=xa)
    y = _forward(m, c, dev, x_amax=_word(dev, _float_bits(big)))
    assert _bits_equal(y, ya)
    assert not _bits_equal(ya, plain)


def test_x_amax_with_floats_behind_cin(m, dev):
    c = RF.make_case('channel_offset')
    assert c['xcs'] > c['cin'] and bool(torch.isnan(c['x'][..., c['cin']:]).all())
    plain = _forward(m, c, dev)
    word = _word(dev)
    y = _forward(m, c, dev, x_amax=m.absmax(c['x'].to(dev), c['cin'], c['xcs']), y_amax=word)
    assert _bits_equal(y, plain)
    _check_y_word(word, y, 'channel_offset')


def _backward(engine, c, dev, x=None, x_amax=None):
    x = (c['x'] if x is None else x).to(dev)
    cw = engine.ConvW(c['w'].to(dev), None, c['k'], c['k'], c['stride'], c['pad'], c['relu'])
    g_out = torch.full((c['B'], c['OH'], c['OW'], c['cout']), float('nan'), device=dev)
    res = engine.conv2d_backward(cw, x, c['B'], c['H'], c['W'], None if c['y32'] is None else c['y32'].to(dev), c['dy_full'].to(dev),
                                 c['OH'], c['OW'], x_cstride=c['xcs'], y_cstride=c['ycs'], y_coffset=c['yco'], g_out=g_out,
                                 precision='f16x3', x_amax=x_amax)
    res = {k: v.cpu() for k, v in res.items()}
    res['g_out'] = g_out.cpu()
    for k, v in res.items():
        assert not bool(torch.isnan(v).any()), k
    return res


@pytest.mark.parametrize('name', ['ragged_3x3', 'stride2_1x1'])
def test_backward_with_the_word_keeps_its_bits(m, dev, name):
    c = R3.make_case(name)
    plain = _backward(m, c, dev)
    got = _backward(m, c, dev, x_amax=m.absmax(c['x'].to(dev), c['cin'], c['xcs']))
    assert set(got) == {'dx', 'dw', 'db', 'g_out'}
    for k in got:
        assert _bits_equal(got[k], plain[k]), (name, k)


def test_backward_takes_the_scale_of_x_from_the_word(m, dev):
    c, xa, big = _never_read_pixel_case(R3.make_case)
    plain = _backward(m, c, dev)
    want = _backward(m, c, dev, x=xa)
    got = _backward(m, c, dev, x_amax=_word(dev, _float_bits(big)))
    assert _bits_equal(got['dw'], want['dw'])
    assert not _bits_equal(want['dw'], plain['dw'])
    for k in ('dx', 'db', 'g_out'):                      # nothing but dw depends on x
        assert _bits_equal(got[k], plain[k]), k


class _Chain(object):
    """1x1 (32 -> 64, ReLU) -> 3x3 (64 -> 64, ReLU) -> 1x1 (64 -> 32) + residual, ReLU at 2 x 7 x 9, both precisions f16x3."""

    def __init__(self, dev):
        gen = torch.Generator().manual_seed(7)
        self.x = torch.randn(2, 7, 9, 32, generator=gen).to(dev)
        self.w = [(torch.randn(co, ci, k, k, generator=gen) / (ci * k * k) ** 0.5).to(dev) for co, ci, k in ((64, 32, 1), (64, 64, 3), (32, 64, 1))]
        self.b = [torch.randn(co, generator=gen).to(dev) for co in (64, 64, 32)]
        self.dy = torch.randn(2, 7, 9, 32, generator=gen).to(dev)

    def run(self, engine, reuse, tamper=None):
        """Returns (tensors, scans, reused): the output and, unless tamper is 'inplace' (which runs without a graph: the changed
        tensor is a saved one), every gradient."""
        from stereo_rcnn_amd import autograd
        leaves = [t.clone().requires_grad_(True) for t in [self.x] + self.w + self.b]
        x, w, b = leaves[0], leaves[1:4], leaves[4:7]
        kw = dict(backward_precision='f16x3', forward_precision='f16x3', reuse_maxima=reuse)
        engine.reset_f16x3_maxima()
        with (torch.no_grad() if tamper == 'inplace' else torch.enable_grad()):
            h = autograd.conv2d_nhwc(x, w[0], b[0], relu=True, **kw)
            if tamper == 'slice':
                h = h[:1]
            elif tamper == 'cat':
                h = torch.cat((h[:1], h[1:]), 0)
            elif tamper == 'inplace':
                h.add_(0)
            h = autograd.conv2d_nhwc(h, w[1], b[1], padding=1, relu=True, **kw)
            y = autograd.conv2d_nhwc(h, w[2], b[2], relu=True, residual=x[:int(h.shape[0])], **kw)
        out = [y.detach().cpu()]
        if tamper != 'inplace':
            y.backward(self.dy[:int(y.shape[0])])
            out += [t.grad.cpu() for t in leaves]
        torch.cuda.synchronize()
        return out, engine.F16X3_MAXIMA['scans'], engine.F16X3_MAXIMA['reused']


@pytest.fixture(scope='module')
def chain(dev):
    return _Chain(dev)


def _same(a, b):
    return len(a) == len(b) and all(_bits_equal(p, q) for p, q in zip(a, b))


def test_chain_of_three_scans_its_input_once(m, chain):
    off, scans_off, reused_off = chain.run(m, False)
    on, scans_on, reused_on = chain.run(m, True)
    assert len(on) == 8 and float(on[0].abs().max()) > 0 and _same(on, off)
    # without: three forward scans and three weight-gradient scans; with: the chain's input, once
    assert (scans_off, reused_off) == (6, 0)
    assert (scans_on, reused_on) == (1, 5)


@pytest.mark.parametrize('tamper', ['slice', 'cat', 'inplace'])
def test_chain_misses_on_another_tensor(m, chain, tamper):
    """A slice, a torch.cat result and a tensor changed in place are not the tensor the word was recorded for: scanned."""
    off, scans_off, _ = chain.run(m, False, tamper)
    on, scans_on, reused_on = chain.run(m, True, tamper)
    assert _same(on, off), tamper
    assert scans_on == 2, (tamper, scans_on)             # the chain's input and the tampered tensor
    assert scans_on + reused_on == scans_off


def test_only_the_backward_f16x3(m, chain):
    """forward 'f32', backward 'f16x3': the forward-time scan replaces the backward-time one, and a second consumer hits."""
    from stereo_rcnn_amd import autograd
    res = {}
    for reuse in (False, True):
        x = chain.x.clone().requires_grad_(True)
        w = [chain.w[0].clone().requires_grad_(True), chain.w[0].clone().requires_grad_(True)]
        m.reset_f16x3_maxima()
        y = sum(autograd.conv2d_nhwc(x, wi, None, backward_precision='f16x3', reuse_maxima=reuse) for wi in w)
        y.backward(torch.ones_like(y))
        res[reuse] = ([y.detach().cpu(), x.grad.cpu(), w[0].grad.cpu(), w[1].grad.cpu()], dict(m.F16X3_MAXIMA))
    assert _same(res[True][0], res[False][0])
    assert res[False][1] == {'scans': 2, 'reused': 0} and res[True][1] == {'scans': 1, 'reused': 1}
    # no weight gradient wanted, or no graph: nothing is scanned ahead of a backward that will not come
    m.reset_f16x3_maxima()
    autograd.conv2d_nhwc(chain.x.clone().requires_grad_(True), chain.w[0], None, backward_precision='f16x3')
    with torch.no_grad():
        autograd.conv2d_nhwc(chain.x.clone(), chain.w[0].clone().requires_grad_(True), None, backward_precision='f16x3')
    assert m.F16X3_MAXIMA == {'scans': 0, 'reused': 0}


def test_conv_transpose_hands_its_maximum_through_the_shuffle(m, dev):
    from stereo_rcnn_amd import autograd
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(3, 4, 5, 32, generator=gen).to(dev)
    wt = (torch.randn(32, 32, 2, 2, generator=gen) / 8).to(dev)
    w = (torch.randn(8, 32, 1, 1, generator=gen) / 6).to(dev)
    out = {}
    for reuse in (False, True):
        m.reset_f16x3_maxima()
        up = autograd.conv_transpose2x2(x, wt, None, relu=True, forward_precision='f16x3', reuse_maxima=reuse)
        out[reuse] = (autograd.conv2d_nhwc(up, w, forward_precision='f16x3', reuse_maxima=reuse).cpu(), dict(m.F16X3_MAXIMA))
    assert _bits_equal(out[True][0], out[False][0])
    assert out[False][1] == {'scans': 2, 'reused': 0} and out[True][1] == {'scans': 1, 'reused': 1}


def test_graph_capture(m, dev):
    """One stream, no parallel branches: the _maxima forward captured and replayed twice gives the eager call's bits and word."""
    c = RF.make_case('ragged_3x3')
    x, w, bias = c['x'].to(dev), c['w'].to(dev), c['bias'].to(dev)
    cw = m.ConvW(w, bias, c['k'], c['k'], c['stride'], c['pad'], c['relu'])
    xw = m.absmax(x, c['cin'], c['xcs'])
    torch.cuda.synchronize()

    def call(y, word):
        m.conv2d_train_f16x3(cw, x, c['B'], c['H'], c['W'], y, c['OH'], c['OW'], x_amax=xw, y_amax=word)

    shape = (c['B'], c['OH'], c['OW'], c['cout'])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y0, word0 = torch.empty(shape, device=dev), _word(dev)
        call(y0, word0)
        y1, word1 = torch.full(shape, float('nan'), device=dev), _word(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            call(y1, word1)
        for _ in range(2):
            y1.fill_(float('nan'))
            word1.fill_(FLT_MAX_BITS)
            graph.replay()
            s.synchronize()
            assert _bits_equal(y1.cpu(), y0.cpu()) and int(word1.cpu().item()) == int(word0.cpu().item())
    _check_y_word(word0, y0.cpu(), 'ragged_3x3 captured')
