"""GPU: the f16x3 weights of a whole list of layers from one call (srcnn_train_weights_prepare, csrc/train_weights.hip) and the two
entries that read them (srcnn_conv2d_forward_f16x3_prepared, srcnn_conv2d_backward_f16x3_prepared; include/srcnn_hip.h).

max |w| and the split are functions of the weights alone, so every comparison is a bit-equality: the words against engine.absmax,
the planes against a torch restatement of pow2_scale / split_f16 (s from the word, hi = f16(w s), lo = f16(w s - hi), the forward
layout padded to Cp rows, the backward layout its (Cin, taps, Cp) transpose), and the prepared calls against the *_maxima calls on
the same inputs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 0x5a5a5a5a          # int32 guard words; the planes' guard halves are 1234.0
SHAPES = [(24, 1, 1, 512), (40, 3, 3, 64), (64, 1, 1, 32), (32, 7, 7, 32), (32, 1, 1, 32), (32, 1, 1, 32), (256, 3, 3, 256)]
ZERO, NEGATIVE = 4, 5       # the all-zero layer; the layer whose largest magnitude is a negative element


@pytest.fixture(scope='module')
def m(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import engine
    return engine


@pytest.fixture(scope='module')
def weights(dev):
    g = torch.Generator().manual_seed(7)
    ws = [torch.randn(s, generator=g) * (0.02 * (i + 1)) for i, s in enumerate(SHAPES)]
    ws[ZERO] = torch.zeros(SHAPES[ZERO])
    ws[NEGATIVE][3, 0, 0, 5] = -9.5
    return [w.to(dev) for w in ws]


def _split(w, word):
    """(w_hi, w_lo, wt_hi, wt_lo) as conv_f16x3_scaled.h's pow2_scale and split_f16 give them, on the host."""
    cout, kh, kw, cin = w.shape
    cp = (cout + 31) // 32 * 32
    e = ((int(word) >> 23) & 0xff) - 127
    s = 2.0 ** min(max(14 - e, -126), 126)
    t = torch.zeros(cp, kh * kw, cin)
    t[:cout] = w.cpu().reshape(cout, kh * kw, cin) * s          # exact: a power of two
    hi = t.half()
    lo = (t - hi.float()).half()
    return hi, lo, hi.permute(2, 1, 0).contiguous(), lo.permute(2, 1, 0).contiguous()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _check(engine, ws, prepared):
    for i, (w, p) in enumerate(zip(ws, prepared)):
        word = int(p.word.cpu().item())
        assert word == int(engine.absmax(w).cpu().item()), i
        want = _split(w, word)
        cout, kh, kw, cin = w.shape
        cp = (cout + 31) // 32 * 32
        got = (p.w_hi.cpu().view(cp, kh * kw, cin), p.w_lo.cpu().view(cp, kh * kw, cin),
               p.wt_hi.cpu().view(cin, kh * kw, cp), p.wt_lo.cpu().view(cin, kh * kw, cp))
        for name, a, b in zip(('w_hi', 'w_lo', 'wt_hi', 'wt_lo'), got, want):
            assert _same(a, b), (i, tuple(w.shape), name)
        if cp > cout:
            assert not bool(got[0][cout:].any()) and not bool(got[1][cout:].any()) and not bool(got[2][..., cout:].any())


def test_mixed_list_of_seven(m, weights):
    prepared = m.prepare_train_weights(weights)
    _check(m, weights, prepared)
    z = prepared[ZERO]
    assert int(z.word.cpu().item()) == 0                              # s = 2^126 and exact-zero planes
    assert not bool(z.w_hi.any()) and not bool(z.w_lo.any()) and not bool(z.wt_hi.any()) and not bool(z.wt_lo.any())
    assert int(prepared[NEGATIVE].word.cpu().item()) == int(torch.tensor([9.5]).view(torch.int32).item())


@pytest.mark.parametrize('index', [0, 6])
def test_list_of_one(m, weights, index):
    _check(m, weights[index:index + 1], m.prepare_train_weights(weights[index:index + 1]))


def test_more_layers_than_one_argument_block(m, weights, dev):
    n = 48 + 3                  # include/srcnn_hip.h: 48 layers travel in one kernel-argument block
    g = torch.Generator().manual_seed(9)
    ws = [(torch.randn(8 + i, 1, 1, 32, generator=g) * (1 + i)).to(dev) for i in range(n)]
    _check(m, ws, m.prepare_train_weights(ws))


def test_repeatable_and_isolated(m, weights, dev):
    a = m.prepare_train_weights(weights)
    b = m.prepare_train_weights(weights)
    for p, q in zip(a, b):
        assert torch.equal(p.word, q.word)
        assert all(_same(getattr(p, k), getattr(q, k)) for k in ('w_hi', 'w_lo', 'wt_hi', 'wt_lo'))
    keep = [[getattr(p, k).clone() for k in ('w_hi', 'w_lo', 'wt_hi', 'wt_lo')] + [p.word.clone()] for p in a]
    other = [w * 3.0 for w in reversed(weights[:4])]
    ws2 = torch.empty(4096, dtype=torch.uint8, device=dev)
    _check(m, other, m.prepare_train_weights(other, workspace=ws2))
    for p, k in zip(a, keep):
        assert all(_same(getattr(p, n), t) for n, t in zip(('w_hi', 'w_lo', 'wt_hi', 'wt_lo'), k)) and torch.equal(p.word, k[4])


# ---- the prepared convolution calls: (B, H, W, Cin, Cout, k, stride, pad, relu, bias, residual)
CONVS = {
    '1x1_s1': (2, 6, 7, 64, 64, 1, 1, 0, False, True, False),
    '3x3_s2_res_relu': (1, 9, 11, 32, 40, 3, 2, 1, True, True, True),
    'cout24': (1, 5, 6, 512, 24, 1, 1, 0, False, True, False),
    'm35': (1, 5, 7, 32, 32, 3, 1, 1, True, False, False),            # B OH OW = 35: no multiple of any tile
}


def _conv_case(engine, name, dev):
    B, H, W, cin, cout, k, s, p, relu, bias, res = CONVS[name]
    g = torch.Generator().manual_seed(sorted(CONVS).index(name) + 21)
    OH, OW = engine.conv_out_hw(H, W, k, k, s, p)
    c = dict(B=B, H=H, W=W, OH=OH, OW=OW, relu=relu)
    c['x'] = (torch.randn(B, H, W, cin, generator=g) * 3.0).to(dev)
    w = (torch.randn(cout, k, k, cin, generator=g) * 0.05).to(dev)
    c['cw'] = engine.ConvW(w, torch.randn(cout, generator=g).to(dev) if bias else None, k, k, s, p, relu)
    c['res'] = torch.randn(B, OH, OW, cout, generator=g).to(dev) if res else None
    c['dy'] = (torch.randn(B, OH, OW, cout, generator=g) * 1e-3).to(dev)
    return c


@pytest.mark.parametrize('name', sorted(CONVS))
def test_prepared_forward_and_backward_keep_their_bits(m, dev, name):
    c = _conv_case(m, name, dev)
    cw, x = c['cw'], c['x']
    prepared, = m.prepare_train_weights([cw.weight])
    xw = m.absmax(x)
    outs = []
    for kw in ({}, {'prepared': prepared}):
        y = torch.full((c['B'], c['OH'], c['OW'], cw.cout), float('nan'), device=dev)
        yw = torch.full((1,), GUARD, dtype=torch.int32, device=dev)
        m.conv2d_train_f16x3(cw, x, c['B'], c['H'], c['W'], y, c['OH'], c['OW'], residual=c['res'], x_amax=xw, y_amax=yw, **kw)
        outs.append((y, yw))
    assert not bool(torch.isnan(outs[0][0]).any())
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1], outs[1][1])
    # the prepared call that scans x itself (x_amax absent)
    y = torch.full_like(outs[0][0], float('nan'))
    m.conv2d_train_f16x3(cw, x, c['B'], c['H'], c['W'], y, c['OH'], c['OW'], residual=c['res'], prepared=prepared)
    assert torch.equal(y.view(torch.int32), outs[0][0].view(torch.int32))

    y = outs[0][0]
    grads = []
    for kw in ({}, {'prepared': prepared}):
        g_out = torch.full_like(c['dy'], float('nan'))
        want = ('dx', 'dw', 'db')
        r = m.conv2d_backward(cw, x, c['B'], c['H'], c['W'], y, c['dy'], c['OH'], c['OW'], want=want, g_out=g_out, precision='f16x3',
                              x_amax=xw, **kw)
        grads.append([r[k] for k in want] + [g_out])
    for a, b in zip(*grads):
        assert not bool(torch.isnan(a).any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    # dw alone: no weights are read, the planes are not needed
    r = m.conv2d_backward(cw, x, c['B'], c['H'], c['W'], y, c['dy'], c['OH'], c['OW'], want=('dw',), precision='f16x3', x_amax=xw,
                          prepared=prepared)
    assert torch.equal(r['dw'].view(torch.int32), grads[0][1].view(torch.int32))


# ---- refusals: the error code, and nothing written (guard words around every buffer)
def _guarded_call(dev, break_it):
    from stereo_rcnn_amd import _lib
    L = _lib.lib()
    cout, cin = 40, 32
    w = torch.ones(cout, 1, 1, cin, device=dev)
    halves = 64 * cin
    planes = torch.full((4, halves + 16), 1234.0, dtype=torch.float16, device=dev)        # 8 guard halves on either side
    words = torch.full((3,), GUARD, dtype=torch.int32, device=dev)
    need = L.srcnn_train_weights_workspace_bytes(1)
    ws = torch.full((need + 64,), 0x5a, dtype=torch.uint8, device=dev)
    d = (_lib.TrainWeightDesc * 1)()
    d[0].w, d[0].w_amax = w.data_ptr(), words[1:2].data_ptr()
    d[0].w_hi, d[0].w_lo, d[0].wt_hi, d[0].wt_lo = (planes[j, 8:].data_ptr() for j in range(4))
    d[0].Cout, d[0].KH, d[0].KW, d[0].Cin = cout, 1, 1, cin
    n, nbytes = break_it(d, need)
    rc = L.srcnn_train_weights_prepare(d, n, ws.data_ptr(), nbytes, _lib.stream())
    torch.cuda.synchronize()
    return rc, L.srcnn_last_error().decode(), planes, words, ws


def _break_null_plane(d, need):
    d[0].wt_lo = None
    return 1, need


@pytest.mark.parametrize('how,code,text', [(_break_null_plane, 'ERR_ARG', 'null'), (lambda d, need: (1, need - 1), 'ERR_WORKSPACE', 'workspace'),
                                           (lambda d, need: (0, need), 'ERR_ARG', 'n_layers')],
                         ids=['null_plane', 'workspace_one_byte_short', 'no_layers'])
def test_refusals_write_nothing(m, dev, how, code, text):
    from stereo_rcnn_amd import _lib
    rc, msg, planes, words, ws = _guarded_call(dev, how)
    assert rc == getattr(_lib, code) and text in msg, (rc, msg)
    assert bool((planes == 1234.0).all()) and bool((words == GUARD).all()) and bool((ws == 0x5a).all())


def test_guards_survive_a_good_call(m, dev):
    rc, msg, planes, words, ws = _guarded_call(dev, lambda d, need: (1, need))
    assert rc == 0, msg
    assert bool((planes[:, :8] == 1234.0).all()) and bool((planes[:, -8:] == 1234.0).all())
    assert int(words[0]) == GUARD and int(words[2]) == GUARD and int(words[1]) == int(torch.tensor([1.0]).view(torch.int32))
    assert bool((planes[0, 8:8 + 40 * 32] == 16384.0).all()) and not bool(planes[0, 8 + 40 * 32:-8].any())


def test_prepared_entries_refuse_bad_planes(m, dev):
    c = _conv_case(m, '1x1_s1', dev)
    cw, x = c['cw'], c['x']
    p, = m.prepare_train_weights([cw.weight])
    y = torch.empty(c['B'], c['OH'], c['OW'], cw.cout, device=dev)
    small = m.PreparedW(p.weight, p.word, p.w_hi[:-8], p.w_lo[:-8], p.wt_hi[:-8], p.wt_lo[:-8])
    odd = m.PreparedW(p.weight, p.word, p.w_hi[1:], p.w_lo[1:], p.wt_hi[1:], p.wt_lo[1:])
    odd.plane_bytes = p.plane_bytes
    for bad, text in ((small, 'plane_bytes'), (odd, 'aligned')):
        with pytest.raises(RuntimeError, match=text):
            m.conv2d_train_f16x3(cw, x, c['B'], c['H'], c['W'], y, c['OH'], c['OW'], prepared=bad)
        with pytest.raises(RuntimeError, match=text):
            m.conv2d_backward(cw, x, c['B'], c['H'], c['W'], None, c['dy'], c['OH'], c['OW'], want=('dx',), precision='f16x3', prepared=bad)
    with pytest.raises(ValueError, match='prepared'):
        m.conv2d_train_f16x3(m.ConvW(cw.weight.clone(), cw.bias, 1, 1, 1, 0, False), x, c['B'], c['H'], c['W'], y, c['OH'], c['OW'], prepared=p)
