"""The specification of srcnn_prep_weights, restated on CPU tensors: the eager path itself (engine.prep_* +
ConvW.split_f16x3 + engine.head_fragments), which is IEEE arithmetic on the host.  A case is (form, sources); `reference`
returns what the kernel must produce bit for bit, `device_spec` the same case as an engine.PrepSpec into guarded buffers."""
import math

import torch

GUARD = 64                  # sentinel elements on either side of every destination
SENTINEL = {torch.float32: 12345.5, torch.float16: 1234.0, torch.int32: 1234567}


def bn_of(gen, c):
    return {'weight': torch.rand(c, generator=gen) + 0.5, 'bias': torch.randn(c, generator=gen) * 0.1,
            'running_mean': torch.randn(c, generator=gen) * 0.1, 'running_var': torch.rand(c, generator=gen) + 0.25}


def reference(case):
    """{'weight', 'bias', 'w_hi', 'w_lo', 'k', 'inv_scale', 'frag' (None unless case['frag'])} from the eager path on the CPU."""
    from stereo_rcnn_amd import engine
    f, ws, bs, bns = case['form'], case['ws'], case.get('bs'), case.get('bns') or []
    if f == 'conv':
        w, b = (ws[0], bs[0] if bs else None) if len(ws) == 1 else (torch.cat(ws, 0), torch.cat(bs, 0) if bs else None)
        cw = engine.prep_conv(w, b, 1, 0, False, bns[0] if bns else None, 'cpu')
    elif f == 'linear':
        cw = engine.prep_linear_stack(ws, bs, 'cpu')
    elif f == 'shortcut':
        cw = engine.prep_conv_shortcut(ws[0], bns[0], ws[1], bns[1], 2, 'cpu')
    elif f == 'stem':
        cw = engine.prep_stem(ws[0], bns[0], 'cpu')
    else:
        cw = engine.prep_deconv2x2(ws[0], bs[0], True, 'cpu')
    cw.split_f16x3()
    k = int(round(-math.log2(cw.inv_scale)))
    assert 2.0 ** -k == cw.inv_scale
    frag = engine.head_fragments(cw) if case.get('frag') else (None, 0)
    return {'weight': cw.weight, 'bias': cw.bias, 'w_hi': cw.w_hi, 'w_lo': cw.w_lo, 'k': k, 'inv_scale': cw.inv_scale,
            'frag': frag[0], 'frag_rows': frag[1]}


def guarded(numel, dtype, dev):
    """A NaN-filled (int: -1) destination of `numel` elements between two sentinel guards: (whole buffer, destination view)."""
    buf = torch.full((numel + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=dev)
    buf[GUARD:GUARD + numel] = float('nan') if dtype.is_floating_point else -1
    return buf, buf[GUARD:GUARD + numel]


def guards_intact(buf):
    s = torch.tensor(SENTINEL[buf.dtype], dtype=buf.dtype, device=buf.device)
    return bool((buf[:GUARD] == s).all()) and bool((buf[-GUARD:] == s).all())


def device_spec(case, ref, dev):
    """(engine.PrepSpec, {name: (guarded buffer, destination view)}) of a case; the destinations have the reference's sizes."""
    from stereo_rcnn_amd import _lib, engine
    form = {'conv': _lib.PREP_CONV, 'linear': _lib.PREP_CONV, 'shortcut': _lib.PREP_SHORTCUT, 'stem': _lib.PREP_STEM,
            'deconv': _lib.PREP_DECONV2X2}[case['form']]
    to = lambda t: None if t is None else t.to(dev).contiguous()
    bufs = {'weight': guarded(ref['weight'].numel(), torch.float32, dev), 'w_hi': guarded(ref['weight'].numel(), torch.float16, dev),
            'w_lo': guarded(ref['weight'].numel(), torch.float16, dev)}
    if ref['bias'] is not None:
        bufs['bias'] = guarded(ref['bias'].numel(), torch.float32, dev)
    if ref['frag'] is not None:
        bufs['frag'] = guarded(ref['frag'].numel(), torch.float16, dev)
    view = lambda n: bufs[n][1] if n in bufs else None
    bns = [{k: to(v) for k, v in bn.items()} for bn in (case.get('bns') or [])]
    spec = engine.PrepSpec(form, [to(w) for w in case['ws']], [to(b) for b in case['bs']] if case.get('bs') else None, bns,
                           view('weight'), view('bias'), view('w_hi'), view('w_lo'), view('frag'), ref['frag_rows'])
    return spec, bufs
