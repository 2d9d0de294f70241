"""CPU: characterisation of the conv engine's host side (stereo_rcnn_amd/engine.py: conv2d, conv_chain, conv_group, _tune).

No kernel runs: the library is a stub that records every descriptor it is handed (pointers replaced by the label of the tensor they
point into), the stream is 0 and CPU tensors serve as buffers.  Each case records what the engine did -- descriptors, the returned
plan, the launches issued, the FlopCounter totals and rows, KEY_HITS, and the candidate plans handed to the tuner -- and the test
asserts EXACT equality (dicts, floats) with tests/golden/engine_host_characterisation.json.

The golden file is not written by hand: `python tests/test_engine_host_cpu.py --record` writes it from the engine it runs on.  It was
recorded at commit 3c49a39 (before engine.py's launch path was restructured), so it pins that commit's behaviour."""
import contextlib
import ctypes
import json
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(HERE))

from stereo_rcnn_amd import _lib, engine  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden', 'engine_host_characterisation.json')
F32, S16 = _lib.FMT_F32, _lib.FMT_SPLIT16
POINTER_FIELDS = [n for n, t in _lib.ConvDesc._fields_ if t is ctypes.c_void_p]


def weights(*shape):
    """Deterministic non-zero values without a random generator: max |w| = 0.08."""
    n = 1
    for s in shape:
        n *= s
    return (((torch.arange(n) % 17) - 8).float() * 0.01).view(*shape)


def bn(c):
    return {'weight': weights(c) + 1.0, 'bias': weights(c), 'running_mean': weights(c) * 0.5, 'running_var': weights(c) + 1.0}


class DeviceWord(object):
    """Stand-in for the device int32 tensor of a row limit: conv2d needs is_cuda, dtype and data_ptr."""
    is_cuda, dtype = True, torch.int32

    def __init__(self, backing):
        self.backing = backing

    def data_ptr(self):
        return self.backing.data_ptr()


class StubLib(object):
    def __init__(self, h):
        self.h = h

    def srcnn_conv2d_workspace_bytes(self, dref):
        return 0

    def srcnn_program_recording(self):
        return self.h.recording

    def srcnn_range_flag_device_word(self):
        return 0

    def srcnn_range_flag_bind(self, p):
        return 0

    def srcnn_conv2d(self, dref, ws, ws_bytes, st):
        self.h.calls.append(['srcnn_conv2d', [self.h.desc(dref._obj)], st])
        return 0

    def srcnn_conv2d_chain(self, descs, n, st):
        self.h.calls.append(['srcnn_conv2d_chain', [self.h.desc(descs[i]) for i in range(n)], st])
        return 0

    def srcnn_conv2d_group(self, descs, n, st):
        self.h.calls.append(['srcnn_conv2d_group', [self.h.desc(descs[i]) for i in range(n)], st])
        return 0


class Harness(object):
    """One per case: the labelled buffers, the stub's switches, and the log of what the engine did."""

    def __init__(self):
        self.labels = {}
        self.recording = 0
        self.capturing = False
        self.calls = []
        self.tunes = []

    def buf(self, label, numel=64):
        t = self.labels[label] = torch.zeros(int(numel))
        return t

    def cw(self, label, cw):
        self.labels[label] = cw
        return cw

    def _regions(self):
        for label, v in self.labels.items():
            if isinstance(v, engine.ConvW):
                parts = [('.weight', v.weight), ('.bias', v.bias), ('.w_hi', v.w_hi), ('.w_lo', v.w_lo),
                         ('._frag', (getattr(v, '_frag', None) or (None,))[0])]
                parts += [('._bias_shifted[%d]' % k, t) for k, t in sorted(getattr(v, '_bias_shifted', {}).items())]
                for suffix, t in parts:
                    if t is not None:
                        yield label + suffix, t
            else:
                yield label, v

    def label_of(self, p):
        if not p:
            return None
        for label, t in self._regions():
            off = p - t.data_ptr()
            if 0 <= off < max(1, t.numel() * t.element_size()):
                return label if off == 0 else '%s+%d' % (label, off)
        return '<unlabelled>'

    def desc(self, d):
        out = {}
        for name, _ in _lib.ConvDesc._fields_:
            v = getattr(d, name)
            out[name] = self.label_of(v) if name in POINTER_FIELDS else v
        out['layer_tag'] = engine.TAG_NAMES.get(d.layer_tag + 1) if d.layer_tag else None
        return out

    def tune_candidates_stub(self, d, key, device, cands, log, L, st):
        self.tunes.append({'key': list(key), 'cands': [list(c) for c in cands], 'desc': self.desc(d), 'log': list(log), 'stream': st})
        engine._TUNED[key] = cands[0]
        return cands[0]

    def observe(self, fn, *args, **kw):
        """Run one engine entry point; returns the record of what it did."""
        count = kw.pop('_count', True)
        rows = kw.pop('_rows', True)
        FC = engine.FlopCounter
        FC.enabled, FC.flops, FC.launches, FC.bytes, FC.rows = count, 0.0, 0, 0.0, ([] if rows else None)
        engine.KEY_HITS = {}
        self.calls, self.tunes = [], []
        out = fn(*args, **kw)
        return {'returned': self.desc(out) if isinstance(out, _lib.ConvDesc) else out,
                'calls': self.calls, 'n_calls': len(self.calls), 'tunes': self.tunes,
                'flops': FC.flops, 'bytes': FC.bytes, 'launches': FC.launches, 'rows': FC.rows,
                'key_hits': [[list(k), n] for k, n in engine.KEY_HITS.items()],
                'tuned': [[list(k), list(v)] for k, v in engine._TUNED.items()]}


@contextlib.contextmanager
def patched(h):
    """The engine on a stub library, with every module switch at its documented default and empty plan tables."""
    FC = engine.FlopCounter
    saved = [(_lib, 'lib', _lib.lib), (_lib, 'stream', _lib.stream),
             (torch.cuda, 'is_current_stream_capturing', torch.cuda.is_current_stream_capturing),
             (engine, '_tune_candidates', engine._tune_candidates)]
    saved += [(engine, n, getattr(engine, n)) for n in ('_TUNED', '_TUNE_LOG', 'KEY_HITS', 'REPEAT', 'AUTOTUNE', 'PRECISION', 'TUNE_MODE',
                                                        'TUNE_STREAMS', 'MAX_LDS_KB', 'CHAIN_MIN_WGS', 'LIMIT_TUNE_ROIS')]
    saved += [(FC, n, getattr(FC, n)) for n in ('enabled', 'flops', 'launches', 'bytes', 'rows')]
    stub = StubLib(h)
    try:
        _lib.lib = lambda: stub
        _lib.stream = lambda: 0
        torch.cuda.is_current_stream_capturing = lambda: h.capturing
        engine._tune_candidates = h.tune_candidates_stub
        engine._TUNED, engine._TUNE_LOG, engine.KEY_HITS, engine.REPEAT = {}, {}, None, []
        engine.AUTOTUNE, engine.PRECISION, engine.TUNE_MODE, engine.TUNE_STREAMS = True, 'f32', 'isolated', 3
        engine.MAX_LDS_KB, engine.CHAIN_MIN_WGS, engine.LIMIT_TUNE_ROIS = 160, 32, 64
        yield
    finally:
        for obj, name, value in saved:
            setattr(obj, name, value)


# ---- the cases: each takes a fresh Harness and returns {step name: record}

def conv3x3(h, label, cin, cout, relu=True, stride=1):
    return h.cw(label, engine.prep_conv(weights(cout, cin, 3, 3), weights(cout), stride, 1, relu, device='cpu'))


def conv1x1(h, label, cin, cout, relu=False, stride=1, bias=True):
    return h.cw(label, engine.prep_conv(weights(cout, cin, 1, 1), weights(cout) if bias else None, stride, 0, relu, device='cpu'))


def shortcut(h, label, cin, cin2, cout, stride2):
    return h.cw(label, engine.prep_conv_shortcut(weights(cout, cin, 1, 1), bn(cout), weights(cout, cin2, 1, 1), bn(cout), stride2, device='cpu'))


def deconv(h, label, cin, cout):
    return h.cw(label, engine.prep_deconv2x2(weights(cin, cout, 2, 2), weights(cout), device='cpu'))


def case_f32_explicit_plan(h):
    cw = conv3x3(h, 'cw', 32, 64)
    x, y = h.buf('x'), h.buf('y')
    return {'counted': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, plan=(2, 1, 4, 2, 1), name='l1.conv'),
            'unnamed': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, plan=[1, 1, 4, 2, 3]),
            'totals_only': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, plan=(2, 1, 4, 2, 1), _rows=False),
            'not_counted': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, plan=(2, 1, 4, 2, 1), _count=False),
            'no_autotune_no_plan': _without_autotune(h, engine.conv2d, cw, x, 2, 20, 30, y, 20, 30)}


def _without_autotune(h, fn, *args, **kw):
    engine.AUTOTUNE = False
    try:
        return h.observe(fn, *args, **kw)
    finally:
        engine.AUTOTUNE = True


def case_f16x3_tuned_hit(h):
    cw = conv3x3(h, 'cw', 64, 128)
    x, y = h.buf('x'), h.buf('y')
    engine._TUNED[('f16x3', 2, 20, 30, 20, 30, 64, 128, 3, 3, 1, 1, 0, 64, 1, 1, 0)] = (2, 2, 8, 4, 1)
    engine._TUNED[('f16x3', 2, 20, 30, 20, 30, 64, 128, 3, 3, 1, 1, 0, 64, 1, 0, 0, 'conc', 3)] = (1, 2, 4, 3, 2)
    engine._TUNED[('f32', 2, 20, 30, 20, 30, 64, 128, 3, 3, 1, 1, 0, 96, 0, 0, 0)] = (1, 1, 4, 2, 6)
    out = {'split16': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, precision='f16x3', x_fmt=S16, y_fmt=S16, name='l2.conv')}
    engine.set_tune_mode('concurrent')
    out['concurrent_key'] = h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, precision='f16x3', x_fmt=S16)
    engine.set_tune_mode('isolated')
    out['f32_default_precision_x_cstride'] = h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, x_cstride=96)
    return out


def case_out_shift_bias_cache(h):
    cw = conv1x1(h, 'cw', 64, 128, relu=True)
    nb = conv1x1(h, 'nobias', 64, 128, bias=False)
    x, y = h.buf('x'), h.buf('y')
    kw = dict(precision='f16x3', x_fmt=S16, y_fmt=S16, plan=(2, 2, 4, 2, 1))
    out = {'first': h.observe(engine.conv2d, cw, x, 1, 16, 16, y, 16, 16, in_shift=1, out_shift=2, **kw)}
    first = cw._bias_shifted[2]
    out['second'] = h.observe(engine.conv2d, cw, x, 1, 16, 16, y, 16, 16, in_shift=0, out_shift=2, **kw)
    out['cache_reused'] = cw._bias_shifted[2] is first
    out['other_shift'] = h.observe(engine.conv2d, cw, x, 1, 16, 16, y, 16, 16, in_shift=3, out_shift=-1, **kw)
    out['cache_keys'] = sorted(cw._bias_shifted)
    out['cache_scales'] = [float(cw._bias_shifted[k].abs().sum() / cw.bias.abs().sum()) for k in sorted(cw._bias_shifted)]
    out['in_shift_only'] = h.observe(engine.conv2d, cw, x, 1, 16, 16, y, 16, 16, in_shift=2, **kw)
    out['no_bias'] = h.observe(engine.conv2d, nb, x, 1, 16, 16, y, 16, 16, out_shift=2, **kw)
    return out


def case_residual(h):
    cw = conv1x1(h, 'cw', 64, 256, relu=True)
    x, y, r = h.buf('x', 4096), h.buf('y'), h.buf('res')
    return {'f32': h.observe(engine.conv2d, cw, x, 2, 12, 18, y, 12, 18, residual=r, plan=(2, 2, 4, 2, 1), name='l1.b1.conv3'),
            'strides_offsets': h.observe(engine.conv2d, cw, x, 2, 12, 18, y, 12, 18, x_cstride=128, y_cstride=1024, y_coffset=512, residual=r,
                                         res_cstride=512, x_offset_elems=100, relu=False, precision='f16x3', x_fmt=S16, y_fmt=S16,
                                         res_fmt=S16, plan=(2, 2, 8, 2, 1))}


def case_strided_1x1(h):
    cw = conv1x1(h, 'cw', 64, 128, stride=2)
    x, y = h.buf('x'), h.buf('y')
    return {'explicit': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 10, 15, plan=(1, 2, 4, 2, 1), name='l2.downsample')}


def case_shortcut_x2(h):
    cw = shortcut(h, 'cw', 64, 128, 256, 2)
    x, y, x2 = h.buf('x'), h.buf('y'), h.buf('x2')
    kw = dict(precision='f16x3', x_fmt=S16, y_fmt=S16, x2=x2, H2=20, W2=30, name='l2.b0.conv3+shortcut')
    out = {'tuned_now': h.observe(engine.conv2d, cw, x, 2, 10, 15, y, 10, 15, **kw),
           'hit': h.observe(engine.conv2d, cw, x, 2, 10, 15, y, 10, 15, **kw),
           'explicit_x2_cstride': h.observe(engine.conv2d, cw, x, 2, 10, 15, y, 10, 15, x2_cstride=192, plan=(2, 2, 8, 2, 1), **kw)}
    with pytest.raises(AssertionError):
        engine.conv2d(cw, x, 2, 10, 15, y, 10, 15, precision='f16x3', x_fmt=S16, plan=(2, 2, 8, 2, 1))
    return out


def case_m_limit(h):
    cw = conv3x3(h, 'cw', 256, 256)
    x, y = h.buf('x'), h.buf('y')
    lim = DeviceWord(h.buf('m_limit', 1))
    kw = dict(precision='f16x3', x_fmt=S16, y_fmt=S16, m_limit=lim, m_limit_mul=196, name='kpts.conv1')
    out = {'tuned_with_typical_limit': h.observe(engine.conv2d, cw, x, 300, 14, 14, y, 14, 14, **kw),
           'hit': h.observe(engine.conv2d, cw, x, 300, 14, 14, y, 14, 14, **kw),
           'explicit': h.observe(engine.conv2d, cw, x, 300, 14, 14, y, 14, 14, plan=(2, 2, 8, 4, 1), **kw)}
    h.recording = 1
    kw['m_limit_mul'] = 49
    out['recording'] = h.observe(engine.conv2d, cw, x, 300, 14, 14, y, 14, 14, **kw)
    return out


def case_untuned_while_recording(h):
    cw = conv3x3(h, 'cw', 64, 128)
    x, y = h.buf('x'), h.buf('y')
    h.recording = 1
    out = {'recording': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, precision='f16x3', x_fmt=S16, y_fmt=S16)}
    h.recording, h.capturing = 0, True
    out['capturing'] = h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30)
    h.capturing = False
    out['then_tuned'] = h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30)
    return out


def case_head_on_deconv(h):
    cw = deconv(h, 'deconv', 256, 256)
    hcw = conv1x1(h, 'head', 256, 6)
    x, hy = h.buf('x'), h.buf('head_y', 8 * 14 * 14 * 4 * 6)
    lim = DeviceWord(h.buf('m_limit', 1))
    kw = dict(precision='f16x3', x_fmt=S16, y_fmt=S16, head=(hcw, hy), name='kpts.deconv+class')
    out = {'no_plan': h.observe(engine.conv2d, cw, x, 8, 14, 14, None, 14, 14, out_shift=1, **kw),
           'explicit_plan_is_overridden': h.observe(engine.conv2d, cw, x, 8, 14, 14, None, 14, 14, plan=(2, 2, 8, 2, 1), m_limit=lim,
                                                    m_limit_mul=196, **kw),
           'no_autotune': _without_autotune(h, engine.conv2d, cw, x, 8, 14, 14, None, 14, 14, **kw)}
    cw0 = conv3x3(h, 'conv', 256, 256)
    out['mode0'] = h.observe(engine.conv2d, cw0, x, 8, 14, 14, h.buf('y'), 14, 14, **kw)
    return out


def case_head2(h):
    dc = deconv(h, 'deconv', 256, 256)
    k6 = conv1x1(h, 'head6', 256, 6)
    rpn = conv3x3(h, 'rpn', 256, 1024)
    k24 = conv1x1(h, 'head24', 1024, 24)
    nb24 = conv1x1(h, 'head24nb', 1024, 24, bias=False)
    x = h.buf('x')
    hy6 = h.buf('hy6', 8 * 14 * 14 * 4 * 6)
    lim = DeviceWord(h.buf('m_limit', 1))
    kw = dict(precision='f16x3', x_fmt=S16, y_fmt=S16)
    out = {'final_deconv': h.observe(engine.conv2d, dc, x, 8, 14, 14, None, 14, 14, head2=(k6, hy6, 0), out_shift=-1, m_limit=lim, m_limit_mul=196,
                                     name='kpts.deconv+class', **kw),
           'final_explicit': h.observe(engine.conv2d, dc, x, 8, 14, 14, None, 14, 14, head2=(k6, hy6, 0), plan=(2, 2, 8, 2, 1), **kw),
           'final_no_autotune': _without_autotune(h, engine.conv2d, dc, x, 8, 14, 14, None, 14, 14, head2=(k6, hy6, 0), **kw)}

    def parts(label, M, n=8):
        return h.buf(label, n * M * 24)

    engine._TUNED[('f16x3', 2, 38, 125, 38, 125, 256, 1024, 3, 3, 1, 1, 0, 256, 1, 0, 0, 'head2', 24)] = (2, 2, 8, 2, 1)
    out['partial_tuned'] = h.observe(engine.conv2d, rpn, x, 2, 38, 125, None, 38, 125, head2=(k24, parts('p3', 9500), 8), name='rpn_conv+head.P3', **kw)
    out['partial_no_head_bias'] = h.observe(engine.conv2d, rpn, x, 2, 38, 125, None, 38, 125, head2=(nb24, parts('p3b', 9500), 8), **kw)
    out['final_24'] = h.observe(engine.conv2d, conv3x3(h, 'rpn256', 256, 256), x, 2, 38, 125, None, 38, 125, head2=(conv1x1(h, 'h24x256', 256, 24),
                                                                                                               parts('f24', 9500, 1), 0), **kw)
    h.recording = 1
    out['partial_recording_M2048'] = h.observe(engine.conv2d, rpn, x, 2, 32, 32, None, 32, 32, head2=(k24, parts('m2048', 2048), 8), **kw)
    out['partial_recording_M2046'] = h.observe(engine.conv2d, rpn, x, 2, 31, 33, None, 31, 33, head2=(k24, parts('m2046', 2046), 8), **kw)
    h.recording = 0
    out['partial_tuned_now_M1024'] = h.observe(engine.conv2d, rpn, x, 2, 16, 32, None, 16, 32, head2=(k24, parts('m1024', 1024), 8), **kw)
    out['partial_tuned_now_M1022'] = h.observe(engine.conv2d, rpn, x, 2, 7, 73, None, 7, 73, head2=(k24, parts('m1022', 1022), 8), m_limit=lim,
                                               m_limit_mul=7, **kw)
    engine.set_tune_mode('concurrent', 4)
    h.capturing = True
    out['partial_capturing_concurrent_key'] = h.observe(engine.conv2d, rpn, x, 2, 10, 32, None, 10, 32, head2=(k24, parts('m640', 640), 8), **kw)
    return out


def case_up(h):
    cw = conv1x1(h, 'lateral', 512, 256)
    x, y, top = h.buf('x'), h.buf('y'), h.buf('top')
    kw = dict(precision='f16x3', x_fmt=S16, y_fmt=S16, up=(top, 19, 63, S16), name='fpn.lateral2')
    return {'explicit_256x256': h.observe(engine.conv2d, cw, x, 2, 38, 125, y, 38, 125, plan=(4, 4, 8, 2, 1), **kw),
            'explicit_128x128_split': h.observe(engine.conv2d, cw, x, 2, 38, 125, y, 38, 125, plan=(2, 2, 8, 4, 3), **kw),
            'explicit_zeros': h.observe(engine.conv2d, cw, x, 2, 38, 125, y, 38, 125, plan=(0, 0, 0, 0, 0), **kw),
            'tuned_now': h.observe(engine.conv2d, cw, x, 2, 38, 125, y, 38, 125, **kw),
            'hit': h.observe(engine.conv2d, cw, x, 2, 38, 125, y, 38, 125, **kw),
            'desc_only_256x256': h.observe(engine.conv2d, cw, x, 2, 38, 125, y, 38, 125, plan=(4, 4, 8, 2, 1), desc_only=True, **kw)}


def case_desc_only(h):
    cw = conv3x3(h, 'cw', 64, 128)
    x, y = h.buf('x'), h.buf('y')
    engine.REPEAT = [(re.compile('l2'), 2)]
    out = {'desc_only': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, precision='f16x3', x_fmt=S16, y_fmt=S16, plan=(2, 2, 8, 2, 1),
                                  desc_only=True, name='l2.conv')}
    with pytest.raises(AssertionError):
        engine.conv2d(cw, x, 2, 20, 30, y, 20, 30, desc_only=True)
    return out


def _chain_phases(h):
    c2 = conv3x3(h, 'conv2', 128, 128, stride=2)
    c3 = shortcut(h, 'conv3+shortcut', 128, 256, 512, 2)
    c1 = conv1x1(h, 'conv1', 512, 128, relu=True)
    t0, t1, t2, t3, xin, res = [h.buf(n) for n in ('t0', 't1', 't2', 't3', 'block_in', 'res')]
    kw = dict(precision='f16x3', x_fmt=S16, y_fmt=S16)
    return [((c2, t0, 2, 76, 250, t1, 38, 125), dict(kw, name='l2.b0.conv2')),
            ((c3, t1, 2, 38, 125, t2, 38, 125), dict(kw, name='l2.b0.conv3', x2=xin, H2=76, W2=250)),
            ((c1, t2, 2, 38, 125, t3, 38, 125), dict(kw, name='l2.b1.conv1', residual=res, res_fmt=S16, in_shift=1, out_shift=1))]


def case_conv_chain(h):
    phases = _chain_phases(h)
    out = {'three_phases': h.observe(engine.conv_chain, phases, (4, 8, 3, 1, 2), name='l2.b0.chain'),
           'unnamed_two_phases_one_width': h.observe(engine.conv_chain, phases[1:], (2, 4, 2, 1, 1)),
           'phases_without_names': h.observe(engine.conv_chain, [(a, {k: v for k, v in kw.items() if k != 'name'}) for a, kw in phases[:2]],
                                             (4, 8, 3, 2, 2)),
           'totals_only': h.observe(engine.conv_chain, phases, (4, 8, 3, 1, 2), name='l2.b0.chain', _rows=False),
           'not_counted': h.observe(engine.conv_chain, phases, (4, 8, 3, 1, 2), name='l2.b0.chain', _count=False)}
    out['chain_tile'] = [[p, M, engine.chain_tile(p, M)] for p, M in [(64, 128 * 32), (64, 128 * 31 + 1), (64, 128 * 31), (128, 256 * 32),
                                                                     (128, 256 * 31), (256, 10 ** 6), (512, 10 ** 6), (96, 10 ** 6)]]
    engine.CHAIN_MIN_WGS = 1
    out['chain_tile_min_wgs_1'] = [[p, M, engine.chain_tile(p, M)] for p, M in [(64, 1), (512, 10 ** 6)]]
    return out


def _group_problems(h, head):
    rpn = conv3x3(h, 'rpn', 256, 1024)
    k24 = conv1x1(h, 'head24', 1024, 24)
    probs = []
    for l, (hh, ww) in enumerate([(38, 125), (19, 63), (10, 32)]):
        kw = dict(precision='f16x3', x_fmt=S16, in_shift=1, out_shift=2, name='rpn_conv+head.P%d' % (l + 3))
        if head:
            kw['head2'] = (k24, h.buf('part%d' % l, 8 * 2 * hh * ww * 24), 8)
        else:
            kw['y_fmt'] = S16
        probs.append(((rpn, h.buf('p%d' % (l + 3)), 2, hh, ww, None if head else h.buf('y%d' % l), hh, ww), kw))
    return probs


def case_conv_group(h):
    with_head, plain = _group_problems(h, True), _group_problems(h, False)
    res = h.buf('res')
    plain[1][1]['residual'] = res
    return {'three_levels_head2': h.observe(engine.conv_group, with_head, (4, 4, 8, 2), name='rpn_conv+head.P3+4+5'),
            'final_head2': h.observe(engine.conv_group, [(a, dict(kw, head2=(kw['head2'][0], kw['head2'][1], 0))) for a, kw in with_head[:2]],
                                     [2, 2, 8, 2]),
            'plain_unnamed': h.observe(engine.conv_group, plain, (4, 2, 8, 3)),
            'totals_only': h.observe(engine.conv_group, with_head, (4, 4, 8, 2), name='rpn_conv+head.P3+4+5', _rows=False),
            'not_counted': h.observe(engine.conv_group, with_head, (4, 4, 8, 2), name='rpn_conv+head.P3+4+5', _count=False)}


def case_repeat(h):
    cw = conv3x3(h, 'cw', 64, 128)
    x, y = h.buf('x'), h.buf('y')
    engine.REPEAT = [(re.compile(r'l2\.'), 2), (re.compile(r'rpn'), 3), (re.compile(r'.*conv3$'), 1)]
    kw = dict(precision='f16x3', x_fmt=S16, y_fmt=S16, plan=(2, 2, 8, 2, 1))
    chain, group = _chain_phases(h), _group_problems(h, True)
    return {'conv2d_match': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, name='l2.b0.conv1', **kw),
            'conv2d_two_matches': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, name='l2.b0.conv3', **kw),
            'conv2d_no_match': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, name='l3.b0.conv1', **kw),
            'conv2d_no_name': h.observe(engine.conv2d, cw, x, 2, 20, 30, y, 20, 30, **kw),
            'chain_match': h.observe(engine.conv_chain, chain, (4, 8, 3, 1, 2), name='l2.b0.chain'),
            'chain_no_match': h.observe(engine.conv_chain, chain, (4, 8, 3, 1, 2), name='l4.b0.chain'),
            'chain_no_name': h.observe(engine.conv_chain, chain, (4, 8, 3, 1, 2)),
            'group_match': h.observe(engine.conv_group, group, (4, 4, 8, 2), name='rpn_conv+head.P3+4+5'),
            'group_no_match': h.observe(engine.conv_group, group, (4, 4, 8, 2), name='other'),
            'group_no_name': h.observe(engine.conv_group, group, (4, 4, 8, 2))}


def case_tune_candidates(h):
    """The candidate plans engine._tune hands to the timing loop (engine._tune_candidates, stubbed)."""
    x, y = h.buf('x'), h.buf('y')
    s16 = dict(precision='f16x3', x_fmt=S16, y_fmt=S16)
    dev = torch.device('cpu')

    def cands(key, cw, B, H, W, OH, OW, only=None, **kw):
        d = engine.conv2d(cw, x, B, H, W, y, OH, OW, plan=(0, 0, 0, 0, 0), desc_only=True, **kw)
        h.tunes = []
        best = engine._tune(d, (key,), dev, only=only)
        assert engine._TUNE_LOG[(key,)] == []
        return {'best': best, 'cands': h.tunes[0]['cands'], 'n_tune_calls': len(h.tunes)}

    wide, narrow = conv3x3(h, 'wide', 256, 256), conv3x3(h, 'narrow', 64, 64)
    mid = conv3x3(h, 'mid', 128, 128)
    big1x1 = conv1x1(h, 'big1x1', 2048, 512)
    out = {'f32_cout_64': cands('a', narrow, 2, 40, 60, 40, 60),
           'split16_cout_64': cands('b', narrow, 2, 40, 60, 40, 60, **s16),
           'split16_cout_128': cands('c', mid, 2, 40, 60, 40, 60, **s16),
           'f16x3_f32_input': cands('d', wide, 2, 40, 60, 40, 60, precision='f16x3'),
           'small_M_64': cands('e', wide, 1, 8, 8, 8, 8, **s16),
           'small_M_65': cands('f', wide, 1, 5, 13, 5, 13, **s16),
           'small_M_128': cands('g', wide, 2, 8, 8, 8, 8, **s16),
           'eligible_256x256': cands('h', wide, 2, 32, 32, 32, 32, **s16),
           'not_eligible_256x256_M2047': cands('i', wide, 1, 23, 89, 23, 89, **s16),
           'many_blocks': cands('j', wide, 2, 150, 500, 150, 500, **s16),
           'deep_K_few_blocks': cands('k', big1x1, 1, 19, 63, 19, 63, **s16),
           'x2': cands('l', shortcut(h, 'sc', 256, 512, 1024, 2), 2, 32, 32, 32, 32, x2=h.buf('x2'), H2=64, W2=64, **s16),
           'up': cands('m', conv1x1(h, 'lateral', 512, 256), 2, 38, 125, 38, 125, up=(h.buf('top'), 19, 63, S16), **s16),
           'mode1': cands('n', deconv(h, 'deconv', 256, 256), 16, 14, 14, 14, 14, **s16),
           'only_M1024': cands('o', wide, 2, 16, 32, 16, 32, only=[(4, 4, 8, 2), (2, 2, 8, 2)], **s16),
           'only_M1023': cands('p', wide, 1, 11, 93, 11, 93, only=[(4, 4, 8, 2), (2, 2, 8, 2)], **s16),
           'only_all_fat_small_M': cands('q', wide, 1, 8, 8, 8, 8, only=[(4, 4, 8, 2), (4, 2, 8, 3)], **s16),
           'only_narrow_cout': cands('r', narrow, 1, 8, 8, 8, 8, only=[(2, 2, 8, 2)], **s16)}
    engine.MAX_LDS_KB = 64
    out['lds_64_eligible_256x256'] = cands('s', wide, 2, 32, 32, 32, 32, **s16)
    out['lds_64_only'] = cands('t', wide, 2, 16, 32, 16, 32, only=[(4, 4, 8, 2), (2, 2, 8, 2)], **s16)
    out['lds_64_f32'] = cands('u', wide, 2, 32, 32, 32, 32)
    engine.MAX_LDS_KB = 32
    out['lds_32'] = cands('v', wide, 2, 32, 32, 32, 32, **s16)
    return out


CASES = {name[5:]: fn for name, fn in sorted(globals().items()) if name.startswith('case_') and callable(fn)}


def run_case(name):
    h = Harness()
    with patched(h):
        return json.loads(json.dumps(CASES[name](h)))            # tuples -> lists, as the golden file holds them


@pytest.mark.parametrize('name', sorted(CASES))
def test_engine_host_characterisation(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(CASES)
    got, want = run_case(name), golden[name]
    assert sorted(got) == sorted(want)
    for step in sorted(want):
        assert got[step] == want[step], '%s / %s' % (name, step)


def test_patches_are_undone():
    before = (_lib.lib, _lib.stream, engine._tune_candidates, engine._TUNED, engine.REPEAT, engine.FlopCounter.enabled)
    run_case('f32_explicit_plan')
    assert before == (_lib.lib, _lib.stream, engine._tune_candidates, engine._TUNED, engine.REPEAT, engine.FlopCounter.enabled)


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit('usage: python tests/test_engine_host_cpu.py --record   (writes %s from the engine it runs on)' % GOLDEN)
    with open(GOLDEN, 'w') as f:
        json.dump({name: run_case(name) for name in sorted(CASES)}, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', GOLDEN)
