"""The SPLIT16 DMA-ring convolution kernel (csrc/conv_f16s.hip, conv_f16s_tile.h, conv_f16s_body.inc) against float64 torch on the
CPU: every case of tests/conv_f16s_cases.py on every one of the sixteen instantiations of launch_conv_f16s, unsplit and at the
case's split-K requests.  Per launch:

  * the plan that ran is the plan under test: srcnn_conv2d_plan (engine.resolved_plan) on the launch's own descriptor reports the
    requested tile, waves and stages and the slices plan_for forms.  The one exception is the documented fallback -- an
    instantiation without the scalar general epilogue (cases.vector_only) asked for a case that needs it -- which is computed from
    the case table, must resolve to exactly what the zero plan resolves to, and is still checked for its result;
  * nothing stray, nothing missing: the output lies between guard regions and, like the channels of its rows the launch does not
    own, is prefilled with a bit pattern that decodes to NaN in the output's own format; guards and foreign channels are compared
    as int32 bits, and no written element may decode to NaN;
  * the value: the project's bounds against float64, 2e-5 max(1, max |ref|) (1e-4 for the stem, whose input is scaled by 50);
  * the order classes: the unsplit launches whose resolved plans keep the split products in the same number of accumulator chains
    give identical bits -- a row computed by the wrong tile shows here whatever the tolerance;
  * the SPLIT16 range guard stays clear.

The references are computed once per case (module fixture); a launch takes milliseconds at these sizes."""
import collections

import pytest
import torch
import torch.nn.functional as F

import conv_f16s_cases as cases

pytestmark = pytest.mark.gpu

GUARD = 256                                    # int32 words on either side of the output
CANARY = {0: 0x7FC0BEEF, 1: 0x7E2A7E2A}        # F32: a quiet NaN; SPLIT16: two f16 NaNs per word, so hi and lo both decode to NaN

Prepared = collections.namedtuple('Prepared', 'case cw x res ref rows ycs geometry kwargs')


def _bn(cout, g):
    return {'weight': torch.rand(cout, generator=g) + 0.5, 'bias': torch.randn(cout, generator=g),
            'running_mean': torch.randn(cout, generator=g) * 0.1, 'running_var': torch.rand(cout, generator=g) + 0.5}


def _bn64(v, b):
    return F.batch_norm(v, b['running_mean'].double(), b['running_var'].double(), b['weight'].double(), b['bias'].double(),
                        False, 0.0, 1e-5)


def _prepare(dev, c, seed):
    """Engine weights, device inputs in SPLIT16 and the float64 reference (output pixels x cq) of one case."""
    from stereo_rcnn_amd import engine
    g = torch.Generator().manual_seed(seed)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    res = None
    if c.kind == 'stem':
        x = torch.randn(c.B, 3, c.H, c.W, generator=g) * 50
        w = torch.randn(c.cout, 3, 7, 7, generator=g) * 0.01
        bnp = _bn(c.cout, g)
        ref = F.relu(_bn64(F.conv2d(x.double(), w.double(), None, 2, 3), bnp))
        cw = engine.prep_stem(w, bnp, device=dev)
        xs = torch.empty((c.B, c.H + 6, c.W + 8, 4), device=dev)
        engine.stem_pack(x.to(dev), xs, out_fmt=1)
        geometry = (c.B, c.H + 6, c.W + 8) + tuple(ref.shape[2:])
        kwargs = dict(x_cstride=4)
    elif c.kind == 'deconv':
        x = torch.randn(c.B, c.cin, c.H, c.W, generator=g)
        w = torch.randn(c.cin, c.cout, 2, 2, generator=g) / c.cin ** 0.5
        b = torch.randn(c.cout, generator=g)
        ref = F.conv_transpose2d(x.double(), w.double(), b.double(), 2)
        ref = F.relu(ref) if c.relu else ref
        cw = engine.prep_deconv2x2(w, b, relu=c.relu, device=dev)
        xs = engine.act_convert(nhwc(x).to(dev), 0, 1)
        geometry = (c.B, c.H, c.W, c.H, c.W)
        kwargs = {}
    else:
        x = torch.randn(c.B, c.cin, c.H, c.W, generator=g)
        w = torch.randn(c.cout, c.cin, c.k, c.k, generator=g) / (c.cin * c.k * c.k) ** 0.5
        b = torch.randn(c.cout, generator=g) if c.bias else None
        bnp = _bn(c.cout, g) if c.bn else None
        ref = F.conv2d(x.double(), w.double(), None if b is None else b.double(), c.stride, c.pad)
        if c.bn:
            ref = _bn64(ref, bnp)
        OH, OW = ref.shape[2:]
        kwargs = {}
        if c.res is not None:
            rcs = cases.strides(c)[3]
            r = torch.randn(c.B, OH, OW, rcs, generator=g)          # rows of rcs channels: the launch reads the first cout of each
            ref = ref + r[..., :c.cout].permute(0, 3, 1, 2).double()
            res = r.to(dev)
            if c.res == 'split16':
                res = engine.act_convert(res, 0, 1)
            kwargs = dict(residual=res, res_cstride=rcs, res_fmt=1 if c.res == 'split16' else 0)
        if c.relu:
            ref = F.relu(ref)
        cw = engine.prep_conv(w, b, c.stride, c.pad, c.relu, bn=bnp, device=dev)
        xs = engine.act_convert(nhwc(x).to(dev), 0, 1)
        geometry = (c.B, c.H, c.W, OH, OW)
    assert tuple(geometry[3:]) == cases.out_hw(c)
    ref = nhwc(ref).reshape(-1, c.cout)
    cq, ycs, yco, _ = cases.strides(c)
    kwargs.update(y_cstride=ycs, y_coffset=yco, precision='f16x3', x_fmt=1, y_fmt=c.y_fmt)
    torch.cuda.synchronize()
    return Prepared(c, cw, xs, res, ref, ref.shape[0], ycs, geometry, kwargs)


@pytest.fixture(scope='module')
def prepared(dev):
    """Every case's operands and float64 reference, computed once for the module and left unchanged."""
    return {c.id: _prepare(dev, c, 100 + i) for i, c in enumerate(cases.CASES)}


def _conv(p, y, plan, desc_only=False):
    from stereo_rcnn_amd import engine
    B, H, W, OH, OW = p.geometry
    return engine.conv2d(p.cw, p.x, B, H, W, y, OH, OW, plan=plan, desc_only=desc_only, **p.kwargs)


def _canary_out(p, dev):
    """(whole buffer as int32, the output as the float32-typed tensor conv2d takes): guards and output alike hold the canary."""
    n = p.rows * p.ycs
    buf = torch.full((n + 2 * GUARD,), CANARY[p.case.y_fmt], dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def _decode(p, buf, label):
    """Checks guards and foreign channels bit for bit, decodes the launch's own channels -> (float32 (rows, cq), their int32 bits)."""
    c = p.case
    cq, ycs, yco, _ = cases.strides(c)
    host = buf.cpu()
    canary = CANARY[c.y_fmt]
    assert bool((host[:GUARD] == canary).all()) and bool((host[-GUARD:] == canary).all()), '%s: stray write outside the tensor' % (label,)
    body = host[GUARD:-GUARD].view(p.rows, ycs)
    own = torch.zeros(ycs, dtype=torch.bool)
    own[yco:yco + cq] = True
    if c.y_fmt == 1:
        # SPLIT16: per pixel, every group of 8 channels is 8 int32 words = [8 x f16 hi][8 x f16 lo]
        assert yco % 8 == 0 and cq % 8 == 0 and ycs % 8 == 0
        halves = body.contiguous().view(torch.float16).view(p.rows, ycs // 8, 2, 8)
        value = (halves[:, :, 0, :].float() + halves[:, :, 1, :].float()).reshape(p.rows, ycs)
    else:
        value = body.contiguous().view(torch.float32)
    assert bool((body[:, ~own] == canary).all()), '%s: stray write into channels outside [%d, %d)' % (label, yco, yco + cq)
    got = value[:, own]
    assert not bool(torch.isnan(got).any()), '%s: %d elements left unwritten' % (label, int(torch.isnan(got).sum()))
    return got, body[:, own].contiguous()


MATRIX = [(c.id, s) for c in cases.CASES for s in (1,) + c.splits]


@pytest.mark.parametrize('cid,splits', MATRIX, ids=['%s-splits%d' % cs for cs in MATRIX])
def test_conv_f16s_every_instantiation_vs_float64(dev, prepared, cid, splits):
    """One case at one splits request on all sixteen instantiations; see the module docstring for what each launch must satisfy.
    The mode-1 cases never split (plan_for), the K = 2 case `narrow` at splits 2 runs one K tile per slice and the reduction
    kernel's scalar branch."""
    from stereo_rcnn_amd import engine
    p = prepared[cid]
    c = p.case
    M, N, nkt = cases.gemm(c)
    mode1 = c.kind == 'deconv'
    bound = 1e-4 if c.kind == 'stem' else 2e-5 * max(1.0, float(p.ref.abs().max()))
    engine.range_flag(reset=True)
    heuristic = engine.resolved_plan(_conv(p, _canary_out(p, dev)[1], (0, 0, 0, 0, 0), desc_only=True))
    assert not cases.vector_only(heuristic) and heuristic[2:4] == (4, 2), heuristic
    bits, worst, ran = {}, (-1.0, None), []
    for tile in cases.PLANS:
        plan = tile + (splits,)
        label = (cid, plan)
        buf, y = _canary_out(p, dev)
        resolved = engine.resolved_plan(_conv(p, y, plan, desc_only=True))
        if cases.falls_back(c, plan):
            assert resolved == heuristic, (label, resolved, heuristic)
        else:
            assert resolved == cases.expected_plan(plan, nkt, mode1), (label, resolved)
        ran.append(resolved)
        assert _conv(p, y, plan) == plan, label                      # conv2d returns the request, unchanged
        got, raw = _decode(p, buf, label)
        err = float((got.double() - p.ref).abs().max())
        worst = (err, plan) if err > worst[0] else worst
        assert err < bound, (label, err, bound)
        if resolved[4] == 1:
            bits.setdefault(cases.chains(resolved), []).append((plan, raw))
    print('%s splits %d: largest |got - float64| = %.3e on plan %s (bound %.3e, max |ref| %.3e)'
          % (cid, splits, worst[0], worst[1], bound, float(p.ref.abs().max())))
    # every instantiation the case can carry ran as itself
    assert sorted(set(r[:4] for r in ran)) == sorted(set([t for t in cases.PLANS if not cases.falls_back(c, t)] +
                                                         ([heuristic[:4]] if not c.expect['vector'] else [])))
    for n, members in bits.items():
        for plan, raw in members[1:]:
            assert torch.equal(raw, members[0][1]), '%s: plans %s and %s (%d accumulator chains) differ in bits' % (cid, members[0][0], plan, n)
    flag, name = engine.range_flag(reset=True)
    assert flag == 0, (cid, splits, flag, name)
