"""GPU: srcnn_prep_weights against the eager path (tests/prep_weights_ref.py), bit for bit: weight, bias, w_hi, w_lo, k /
inv_scale and the fused head's fragment layout, for every form and branch of csrc/prep_weights.hip at the smallest shapes that
reach them -- Cout / Cin that are no multiples of the vector width, several rows per unit and several units per row (a 3x3 over
512 channels and a 7x7 over 96 are cut along Cin), sources concatenated along Cout, destinations off the 16-byte grid -- with and
without a frozen BN where the eager form has both (the stem and the shortcut form always fold one; the deconvolution and the
stacked heads never do).  All cases go through ONE call (more layers than one launch carries), into NaN-filled destinations
between sentinel guards, and a second call over the first one's output must give the same bits."""
import pytest
import torch

import prep_weights_ref as R

pytestmark = pytest.mark.gpu


def _cases():
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g) * 0.05
    cases = []
    for bn in (False, True):
        for name, shape in (('1x1 cout 24', (24, 40, 1, 1)), ('1x1 cout 10', (10, 40, 1, 1)), ('3x3 cin 33', (64, 33, 3, 3)),
                            ('3x3 cin 512 (cut along cin)', (4, 512, 3, 3)), ('7x7 cin 96 (cut along cin)', (2, 96, 7, 7)),
                            ('1x1 cin 3', (5, 3, 1, 1))):
            c = dict(name=name + (' bn' if bn else ''), form='conv', ws=[rn(*shape)])
            if bn:
                c['bns'] = [R.bn_of(g, shape[0])]
            else:
                c['bs'] = [rn(shape[0])]
            cases.append(c)
    cases.append(dict(name='1x1 no bias', form='conv', ws=[rn(24, 40, 1, 1)]))
    cases.append(dict(name='stem', form='stem', ws=[rn(8, 3, 7, 7)], bns=[R.bn_of(g, 8)]))
    cases.append(dict(name='shortcut', form='shortcut', ws=[rn(24, 40, 1, 1), rn(24, 20, 1, 1)], bns=[R.bn_of(g, 24), R.bn_of(g, 24)]))
    cases.append(dict(name='shortcut odd', form='shortcut', ws=[rn(7, 10, 1, 1), rn(7, 5, 1, 1)], bns=[R.bn_of(g, 7), R.bn_of(g, 7)]))
    cases.append(dict(name='deconv', form='deconv', ws=[rn(16, 6, 2, 2)], bs=[rn(6)]))
    cases.append(dict(name='linear stack', form='linear', ws=[rn(4, 40), rn(5, 40), rn(2, 40)], bs=[rn(4), rn(5), rn(2)]))
    cases.append(dict(name='rpn head + fragments', form='conv', ws=[rn(6, 32, 1, 1), rn(18, 32, 1, 1)], bs=[rn(6), rn(18)], frag=True))
    cases.append(dict(name='narrow head + fragments', form='conv', ws=[rn(10, 48, 1, 1)], bs=[rn(10)], frag=True))
    # boundary inputs: the max decides k
    p2 = 2.0 ** -3
    one = torch.tensor(p2)
    below, above = float(torch.nextafter(one, torch.tensor(0.0))), float(torch.nextafter(one, torch.tensor(1.0)))

    def with_max(m, at=17):
        w = rn(10, 40, 1, 1).clamp(-0.1, 0.1)
        w.view(-1)[at] = m
        return w
    cases.append(dict(name='all zero', form='conv', ws=[torch.zeros(10, 40, 1, 1)], bs=[rn(10)]))
    cases.append(dict(name='max = 2^-3', form='conv', ws=[with_max(p2)], bs=[rn(10)]))
    cases.append(dict(name='max one ulp below 2^-3', form='conv', ws=[with_max(below)], bs=[rn(10)]))
    cases.append(dict(name='max one ulp above 2^-3', form='conv', ws=[with_max(above)], bs=[rn(10)]))
    cases.append(dict(name='max at a negative element', form='conv', ws=[with_max(-0.3, at=399)], bs=[rn(10)]))
    # max = 1 -> k = 14; elements whose lo lands on / around the smallest f16 subnormal (2^-24) and the smallest normal (2^-14)
    w = torch.zeros(2, 16, 1, 1)
    w.view(-1)[0] = 1.0
    lo_targets = [2.0 ** -24, 0.5 * 2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -15, -2.0 ** -24, 3 * 2.0 ** -25]
    for i, lo in enumerate(lo_targets):
        v = (2.0 ** -3 + lo) / 16384.0
        assert float(torch.tensor(v, dtype=torch.float32).double()) == v        # the element is a float32 as it stands
        w.view(-1)[1 + i] = v
    cases.append(dict(name='lo at the edge of the f16 subnormal range', form='conv', ws=[w], bs=[rn(2)]))
    return cases


@pytest.fixture(scope='module')
def ran(dev):
    """Every case through one srcnn_prep_weights call: [(case, reference, guarded buffers)], k_out buffer, the specs."""
    from stereo_rcnn_amd import engine
    cases = _cases()
    refs = [R.reference(c) for c in cases]
    built = [R.device_spec(c, r, dev) for c, r in zip(cases, refs)]
    specs = [b[0] for b in built]
    from stereo_rcnn_amd import _lib
    assert len(specs) > _lib.PREP_LAYERS_PER_LAUNCH              # more than one launch per pass
    kbuf, k = R.guarded(len(specs), torch.int32, dev)
    engine.prep_weights_into(specs, k)
    torch.cuda.synchronize()
    return [(c, r, b[1]) for c, r, b in zip(cases, refs, built)], (kbuf, k), specs


def _same_bits(got, want):
    want = want.to(got.device).reshape(-1)
    gi = got.view(torch.int32 if got.dtype == torch.float32 else torch.int16)
    wi = want.contiguous().view(torch.int32 if want.dtype == torch.float32 else torch.int16)
    return torch.equal(gi, wi)


def test_bit_equal_to_the_eager_path(ran):
    rows, (kbuf, k), _ = ran
    ks = k.cpu().tolist()
    for (case, ref, bufs), ki in zip(rows, ks):
        for name in ('weight', 'bias', 'w_hi', 'w_lo', 'frag'):
            if name in bufs:
                assert _same_bits(bufs[name][1], ref[name]), (case['name'], name)
        assert ki == ref['k'] and 2.0 ** -ki == ref['inv_scale'], (case['name'], ki, ref['k'])


def test_boundary_exponents(ran):
    rows, (_, k), _ = ran
    got = dict(zip((c['name'] for c, _, _ in rows), k.cpu().tolist()))
    assert got['all zero'] == 0 and got['max = 2^-3'] == 17 and got['max one ulp below 2^-3'] == 17 and got['max one ulp above 2^-3'] == 16
    assert got['lo at the edge of the f16 subnormal range'] == 14


def test_guards_survive_and_nothing_is_left_unwritten(ran):
    rows, (kbuf, k), _ = ran
    assert R.guards_intact(kbuf) and bool((k != -1).all())
    for case, ref, bufs in rows:
        for name, (buf, view) in bufs.items():
            assert R.guards_intact(buf), (case['name'], name)
            assert not bool(torch.isnan(view.float()).any()), (case['name'], name)


def test_second_call_over_the_first_gives_the_same_bits(ran):
    from stereo_rcnn_amd import engine
    rows, (kbuf, k), specs = ran
    before = [{n: b[0].clone() for n, b in bufs.items()} for _, _, bufs in rows]
    k0 = kbuf.clone()
    engine.prep_weights_into(specs, k)
    torch.cuda.synchronize()
    assert torch.equal(kbuf, k0)
    for (case, _, bufs), old in zip(rows, before):
        for n, (buf, _) in bufs.items():
            assert _same_bits(buf, old[n]), (case['name'], n)


def test_nan_wins_the_max_as_in_torch(dev):
    """torch.max returns NaN when one element is NaN; the eager path's `m > 0` is then false: k = 0."""
    from stereo_rcnn_amd import engine
    w = torch.randn(10, 40, 1, 1) * 0.05
    w.view(-1)[123] = float('nan')
    case = dict(name='nan', form='conv', ws=[w], bs=[torch.zeros(10)])
    ref = R.reference(case)
    assert ref['k'] == 0
    spec, bufs = R.device_spec(case, ref, dev)
    k = engine.prep_weights_into([spec]).cpu().tolist()
    assert k == [0]
    for name in ('weight', 'w_hi', 'w_lo'):
        assert _same_bits(bufs[name][1], ref[name]), name


def test_destinations_off_the_16_byte_grid_and_an_alias(dev):
    """Scalar paths: every destination and source one element off the vector grid; and a second layer that shares the first
    one's weight (alias_of: two ConvW over one tensor) writes only its own hi / lo."""
    from stereo_rcnn_amd import _lib, engine
    g = torch.Generator().manual_seed(3)
    w, b = torch.randn(8, 32, 3, 3, generator=g) * 0.05, torch.randn(8, generator=g)
    ref = R.reference(dict(form='conv', ws=[w], bs=[b]))
    n = w.numel()
    off = lambda t: t[1:]
    src = torch.zeros(n + 1, device=dev)
    src[1:] = w.reshape(-1).to(dev)
    dw, dh, dl = (torch.full((n + 2,), float('nan'), dtype=dt, device=dev) for dt in (torch.float32, torch.float16, torch.float16))
    db = torch.full((8,), float('nan'), device=dev)
    h2, l2 = torch.full((n,), float('nan'), dtype=torch.float16, device=dev), torch.full((n,), float('nan'), dtype=torch.float16, device=dev)
    first = engine.PrepSpec(_lib.PREP_CONV, [off(src).view(8, 32, 3, 3)], [b.to(dev)], (), dw[1:n + 1], db, dh[1:n + 1], dl[1:n + 1])
    alias = engine.PrepSpec(_lib.PREP_CONV, [off(src).view(8, 32, 3, 3)], [b.to(dev)], (), dw[1:n + 1], db, h2, l2, alias_of=0)
    k = engine.prep_weights_into([first, alias]).cpu().tolist()
    assert k == [ref['k'], ref['k']]
    assert _same_bits(dw[1:n + 1], ref['weight']) and _same_bits(db, ref['bias'])
    for hi, lo in ((dh[1:n + 1], dl[1:n + 1]), (h2, l2)):
        assert _same_bits(hi, ref['w_hi']) and _same_bits(lo, ref['w_lo'])
    assert bool(torch.isnan(dw[0])) and bool(torch.isnan(dw[n + 1])) and bool(torch.isnan(dh[0])) and bool(torch.isnan(dl[n + 1]))
