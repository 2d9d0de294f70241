"""CPU: characterisation of the forward's launch plan (stereo_rcnn_amd/model/stereo_rcnn/plan.py: Plan).

No kernel runs: every engine function plan.py calls and the library itself are recorders, torch.cuda's streams and events are
labelled fakes, CPU tensors serve as buffers.  Each case is the ordered log of what a Plan issued -- every launch with its
operands (pointers replaced by the name of the Plan / Weights tensor they point into, plus byte offset), the stream it was issued
on, every event record and wait (eager and program-recording form) -- plus the plan's state afterwards, and the test asserts EXACT
equality with tests/golden/plan_host_characterisation.json.gz.  Two launch orders with equal results are different logs.

The golden file is not written by hand: `python tests/test_plan_host_cpu.py --record` writes it from the plan.py it runs on (its
header names the commit it was recorded at: the one before plan.py's rules were restated once each, so it pins that commit's
behaviour).  Identical events are stored once (`events`) and the cases list indices; the JSON text (0.4 MB: a ResNet-101 trunk is a
hundred launches per forward) is committed gzip-compressed, `--dump` prints it for reading or for a diff of two recordings.
`python tests/test_plan_host_cpu.py --time` prints the host time of one eager launch_all() walk under the stubs."""
import contextlib
import ctypes
import gc
import gzip
import io
import json
import os
import subprocess
import sys
import time

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(HERE))

from stereo_rcnn_amd import _lib, engine, fixture, streams  # noqa: E402
from stereo_rcnn_amd.model.stereo_rcnn import plan as plan_mod  # noqa: E402
from stereo_rcnn_amd.model.stereo_rcnn.plan import Plan, Weights  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden', 'plan_host_characterisation.json.gz')
F32, S16 = _lib.FMT_F32, _lib.FMT_SPLIT16
H_IN, W_IN = 64, 96            # pyramid levels 16x24 down to 1x2, A = 1536
SKIP_NAMES = ('maxpool', 'upsample_add', 'subsample', 'rpn_scores', 'proposals', 'roi_align', 'roi_align7', 'roi_align14', 'box_tail',
              'kpts_tail')
SWITCH_DEFAULTS = dict(PRECISION='f32', RPN_PAIR_LAUNCH=True, RPN_HEAD_FUSION=True, RPN_GROUP='small', RPN_GROUP_TILE=(4, 4, 8, 2),
                       UPSAMPLE_FUSION=False, KPTS_HEAD_FUSION='valu', SHORTCUT_FUSION=True, ACT_SCALES=True, DEBUG_SKIP=frozenset(),
                       PLAN_EPOCH=0, TUNE_MODE='isolated', TUNE_STREAMS=3)

_WEIGHTS = []


def the_weights():
    """Built once per module (about 3 s); every case resets what a Plan may change on them."""
    if not _WEIGHTS:
        _WEIGHTS.append(Weights(fixture.make_state_dict(3), torch.device('cpu')))
    w = _WEIGHTS[0]
    w.shifts, w.calibrated, w.calibration_max, w.calib_epoch, w.fuse_shortcut = {}, False, {}, 0, [True, True, True, True]
    if hasattr(w, 'calibration_frames'):
        del w.calibration_frames
    return w


def fixed_shifts(w):
    """Calibrated weights without a calibration run: every group a shift, conv2's output of a layer's first block at its input's."""
    s = {'stem': 3, 'L1': 2, 'L2': 1, 'L3': 0, 'L4': -1, 'P': 2, 'rpn': 1, 'h1': 4, 'h2': 5, 'kup': -3}
    s.update(('k%d' % i, i - 2) for i in range(6))
    for li, blocks in enumerate(w.layers):
        for bi in range(len(blocks)):
            s['L%d.%d.m1' % (li + 1, bi)] = 1
            s['L%d.%d.m2' % (li + 1, bi)] = (s['stem' if li == 0 else 'L%d' % li] if bi == 0 else 0)
    w.shifts, w.calibrated = s, True


class OnDevice(torch.Tensor):
    """A CPU tensor that says it is a device tensor (Plan's entry points assert is_cuda on what callers hand them)."""
    is_cuda = property(lambda self: True)


def on_device(t):
    return t.as_subclass(OnDevice)


class FakeStream(object):
    def __init__(self, h, label):
        self.h, self.label, self.cuda_stream = h, label, label

    def wait_event(self, ev):
        self.h.log('wait_event', stream=self.label, event=ev.n)


class FakeEvent(object):
    def __init__(self, h):
        self.h = h
        self.n = h.n_events = h.n_events + 1

    def record(self, stream):
        self.h.log('event_record', event=self.n, stream=stream.label)


def _walk(name, v):
    if isinstance(v, torch.Tensor):
        yield name, v
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            for r in _walk('%s[%d]' % (name, i), x):
                yield r
    elif isinstance(v, dict):
        for k in sorted(v, key=str):
            for r in _walk('%s.%s' % (name, k), v[k]):
                yield r
    elif isinstance(v, engine.ConvW):
        for k in ('weight', 'bias'):
            if getattr(v, k) is not None:
                yield '%s.%s' % (name, k), getattr(v, k)


def _convws(name, v):
    if isinstance(v, engine.ConvW):
        yield name, v
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            for r in _convws('%s[%d]' % (name, i), x):
                yield r
    elif isinstance(v, dict):
        for k in sorted(v):
            for r in _convws('%s.%s' % (name, k), v[k]):
                yield r


class StubLib(object):
    """Every srcnn_* call is logged with its arguments; a few return what plan.py goes on with."""

    def __init__(self, h):
        self._h = h

    def __getattr__(self, name):
        h = self._h

        def call(*args):
            if name == 'srcnn_range_flag_device_word':
                return 0
            ret = 0
            if name == 'srcnn_program_create':
                h.n_programs += 1
                ret = 'program#%d' % h.n_programs
            elif name == 'srcnn_program_record_event':
                ret = h.n_tokens = h.n_tokens + 1
            elif name == 'srcnn_proposal_workspace_bytes':
                ret = 4096
            h.log(name, args=[h.enc(a) for a in args], **({'returned': ret} if ret else {}))
            return ret
        return call


class Harness(object):
    """One per case: the plan under test, the stubs' switches and the log."""

    def __init__(self, B=1, build=True):
        self.events = []
        self.main = FakeStream(self, 'main')
        self.stack = [self.main]
        self.n_events = self.n_tokens = self.n_programs = self.n_launches = 0
        self.used = (4, 4, 8, 2, 1)        # the plan engine.conv2d says it ran
        self.fill = False                  # conv2d / upsample_add write a constant into their output (cases that read values)
        self.fill_by_name = {}
        self.chain = False
        self.chain_tiles = {}
        self.overlap_default = True        # streams.branch_overlap()
        self.side_kind = 'auto'
        self.extra = {}
        self._regions = None
        self.w = the_weights()
        self.cw_names = {id(cw): n for n, cw in _convws('w', vars(self.w))}
        self.plan = Plan(self.w, B, H_IN, W_IN) if build else None

    # ---- labels
    def regions(self):
        if self._regions is None:
            named = list(self.extra.items())
            for k in sorted(vars(self.plan)):
                if k not in ('c', '_src', 'w', 'programs', 'graphs'):
                    named += list(_walk(k, vars(self.plan)[k]))
            named += list(_walk('w', {k: v for k, v in vars(self.w).items() if k not in ('shifts', 'calibration_max')}))
            self._regions = [(n, t.data_ptr(), max(1, t.numel() * t.element_size())) for n, t in named]
            self._exact = {}
            for n, p, _ in self._regions:
                self._exact.setdefault(p, n)
        return self._regions

    def invalidate(self):
        self._regions = None

    def label_of(self, p):
        if not p:
            return None
        self.regions()
        if p in self._exact:
            return self._exact[p]
        for n, start, size in self._regions:
            if 0 <= p - start < size:
                return '%s+%d' % (n, p - start)
        return '<unlabelled>'

    def enc(self, v):
        if v is None or isinstance(v, (bool, float, str)):
            return v
        if isinstance(v, int):
            return self.label_of(v) if v >= (1 << 24) else v
        if isinstance(v, torch.Tensor):
            return self.label_of(v.data_ptr())
        if isinstance(v, engine.ConvW):
            return self.cw_names[id(v)]
        if isinstance(v, FakeStream):
            return v.label
        if isinstance(v, ctypes.Array):
            return [self.enc(x) for x in v]
        if isinstance(v, (list, tuple)):
            return [self.enc(x) for x in v]
        if isinstance(v, dict):
            return {k: self.enc(x) for k, x in v.items()}
        raise TypeError('cannot label %r' % (v,))

    def log(self, op, **kw):
        kw['op'], kw['on'] = op, self.stack[-1].label
        self.events.append(kw)

    def step(self, name, **kw):
        self.events.append(dict(kw, op='== ' + name))

    # ---- engine stubs
    def conv2d(self, cw, x, B, H, W, y, OH, OW, **kw):
        self.n_launches += 1
        if self.fill and y is not None:
            y.fill_(self.fill_by_name.get(kw.get('name'), 1.0 + self.n_launches % 13))
        self.log('conv2d', cw=self.enc(cw), x=self.enc(x), y=self.enc(y), dims=[B, H, W, OH, OW], kw=self.enc(kw))
        return self.used

    def conv_chain(self, phases, tile, name=None):
        self.n_launches += 1
        self.log('conv_chain', phases=[[self.enc(a), self.enc(kw)] for a, kw in phases], tile=self.enc(tile), name=name)

    def conv_group(self, problems, tile, name=None):
        self.n_launches += 1
        self.log('conv_group', problems=[[self.enc(a), self.enc(kw)] for a, kw in problems], tile=self.enc(tile), name=name)

    def upsample_add(self, top, TH, TW, lateral, B, H, W, C, y, **kw):
        self.n_launches += 1
        if self.fill:
            y.fill_(2.0 + self.n_launches % 7)
        self.log('upsample_add', args=self.enc([top, TH, TW, lateral, B, H, W, C, y]), kw=self.enc(kw))

    def plain(self, op):
        def call(*args, **kw):
            self.log(op, args=self.enc(list(args)), kw=self.enc(kw))
            if op == 'act_convert':
                return args[0].clone()
        return call

    def workspace(self, nbytes, device, key='default'):
        buf = self.extra.setdefault('workspace.' + key, torch.zeros(max(int(nbytes), 256), dtype=torch.uint8))
        self.invalidate()
        if _lib._recording_refs is not None:
            _lib._recording_refs.append(buf)
        return buf

    @contextlib.contextmanager
    def stream(self, s):
        self.stack.append(s)
        try:
            yield
        finally:
            self.stack.pop()

    # ---- what a case leaves behind
    def state(self):
        p = self.plan
        self.invalidate()
        return {'buf_shift': sorted([self.label_of(ptr), k] for ptr, k in p._buf_shift.items()), 'rpn_nparts': list(p.rpn_nparts),
                'packed_fmt': p.packed_fmt, 'fmt': p.fmt, 'programs': sorted(repr(k) for k in p.programs),
                'program_refs': sorted([repr(k), len(v[1])] for k, v in p.programs.items()),
                'PRECISION': engine.PRECISION, 'overlap': p.overlap, 'epoch': repr(p._epoch),
                'src': 'own planes' if p._src[0] is p.im_left and p._src[1] is p.im_right else 'caller tensors',
                'shifts': dict(self.w.shifts), 'fuse_shortcut': list(self.w.fuse_shortcut), 'calibrated': self.w.calibrated,
                'calib_epoch': self.w.calib_epoch, 'calibration_frames': getattr(self.w, 'calibration_frames', None),
                'calibration_max': dict(self.w.calibration_max)}


@contextlib.contextmanager
def patched(h):
    """plan.py on recorders, every engine switch at its documented default."""
    stub = StubLib(h)
    patches = [(_lib, 'lib', lambda: stub), (_lib, 'stream', lambda: h.stack[-1].label), (_lib, 'workspace', h.workspace),
               (engine, 'conv2d', h.conv2d), (engine, 'conv_chain', h.conv_chain), (engine, 'conv_group', h.conv_group),
               (engine, 'upsample_add', h.upsample_add), (engine, 'chain_enabled', lambda: h.chain),
               (engine, 'chain_tile', lambda planes, M: h.chain_tiles.get(planes)),
               (torch.cuda, 'current_stream', lambda *a: h.stack[-1]), (torch.cuda, 'stream', h.stream),
               (torch.cuda, 'Event', lambda *a, **kw: FakeEvent(h)), (torch.cuda, 'synchronize', lambda *a: h.log('synchronize')),
               (streams, 'side_streams', lambda n, device=None, kind=None: None if h.side_kind == 'none' else
                [FakeStream(h, 'side%d' % i) for i in range(n)]),
               (streams, 'branch_overlap', lambda: h.overlap_default)]
    patches += [(engine, op, h.plain(op)) for op in ('stem_pack_pair', 'maxpool3x3s2_ceil', 'subsample2', 'act_convert')]
    patches += [(engine, k, v) for k, v in SWITCH_DEFAULTS.items()]
    saved = [(obj, name, getattr(obj, name)) for obj, name, _ in patches]
    try:
        for obj, name, value in patches:
            setattr(obj, name, value)
        yield
    finally:
        h.plan = None
        gc.collect()                      # Plan.__del__ asks the library for its range word: while the stub is still in place
        for obj, name, value in saved:
            setattr(obj, name, value)


# ---- the cases: each takes a fresh Harness (plan built, stubs in place) and drives it; h.events is the record

def _f16x3(h):
    fixed_shifts(h.w)
    h.plan.fmt, engine.PRECISION = S16, 'f16x3'


def _launch(h, kpts=True, **switches):
    """launch_all on the SPLIT16 engine with fixed shifts under the given engine switches / plan.overlap / harness settings."""
    _f16x3(h)
    for k, v in switches.items():
        if k == 'overlap':
            h.plan.overlap = v
        elif hasattr(engine, k):
            setattr(engine, k, v)
        else:
            assert hasattr(h, k), k
            setattr(h, k, v)
    h.plan.launch_all(kpts)


def case_launch_all_f32(h):
    h.plan.launch_all()


def case_launch_all_f32_no_kpts_no_overlap(h):
    h.plan.overlap = False
    h.plan.launch_all(False)


LAUNCH_CASES = {
    'default': {},
    'no_kpts': dict(kpts=False),
    'overlap_false': dict(overlap=False),
    'overlap_true': dict(overlap=True),
    'overlap_true_but_no_side_streams': dict(overlap=True, side_kind='none'),
    'overlap_follows_streams_false': dict(overlap_default=False),
    'pair_launch_0': dict(RPN_PAIR_LAUNCH=False),
    'head_fusion_0': dict(RPN_HEAD_FUSION=False),
    'group_0': dict(RPN_GROUP='0'),
    'group_all': dict(RPN_GROUP='all'),
    'group_tile_2282': dict(RPN_GROUP_TILE=(2, 2, 8, 2)),
    'upsample_fusion_1': dict(UPSAMPLE_FUSION=True),
    'kpts_head_fusion_0': dict(KPTS_HEAD_FUSION=False),
    'kpts_head_fusion_mfma': dict(KPTS_HEAD_FUSION='mfma'),
    'shortcut_fusion_0': dict(SHORTCUT_FUSION=False),
    'used_2_2_group_0': dict(RPN_GROUP='0', used=(2, 2, 8, 2, 1)),
    'used_zero_small_M_group_0': dict(RPN_GROUP='0', used=(0, 0, 0, 0, 0)),
    'used_4_4_group_0': dict(RPN_GROUP='0', used=(4, 4, 8, 2, 1)),
    'used_2_2_group_small': dict(used=(2, 2, 8, 2, 1)),
    'chains': dict(chain=True, chain_tiles={64: (2, 4, 2, 1, 1), 128: (4, 8, 3, 2, 2), 256: None, 512: (4, 8, 3, 2, 2)}),
    'chains_shortcut_fusion_0': dict(chain=True, chain_tiles={64: (2, 4, 2, 1, 1), 128: (4, 8, 3, 2, 2)}, SHORTCUT_FUSION=False),
}
# pairs of switches that share a branch of fpn_rpn()
for _ov in (False, True):
    for _g in ('0', 'small', 'all'):
        LAUNCH_CASES['overlap_%s_group_%s' % (_ov, _g)] = dict(overlap=_ov, RPN_GROUP=_g)
    for _u in (False, True):
        LAUNCH_CASES['overlap_%s_upsample_fusion_%s' % (_ov, _u)] = dict(overlap=_ov, UPSAMPLE_FUSION=_u)
for _g in ('0', 'small', 'all'):
    for _hf in (False, True):
        for _pl in (False, True):
            LAUNCH_CASES['group_%s_head_fusion_%s_pair_%s' % (_g, _hf, _pl)] = dict(RPN_GROUP=_g, RPN_HEAD_FUSION=_hf, RPN_PAIR_LAUNCH=_pl)
for _n in SKIP_NAMES:
    LAUNCH_CASES['skip_' + _n] = dict(DEBUG_SKIP=frozenset([_n]))
LAUNCH_CASES['skip_upsample_add_no_overlap'] = dict(DEBUG_SKIP=frozenset(['upsample_add']), overlap=False)


def _launch_case(kw):
    def case(h):
        _launch(h, **kw)
    return case


def case_launch_default_B2(h):
    _launch(h)


def case_launch_one_layer_not_fusable(h):
    _f16x3(h)
    h.w.fuse_shortcut = [True, False, True, True]
    h.plan.launch_all()


def case_launch_m2_shift_differs(h):
    _f16x3(h)
    h.w.shifts['L3.0.m2'] = 7
    h.plan.launch_all()


def case_stage_entry_points(h):
    for precision in ('f16x3', 'f32'):
        if precision == 'f16x3':
            _f16x3(h)
        else:
            h.plan.fmt, engine.PRECISION = F32, 'f32'
        for name in ('trunk', 'fpn', 'rpn', 'proposals', 'heads', 'box_head', 'kpts_head', 'fpn_rpn'):
            h.step('%s %s' % (precision, name))
            getattr(h.plan, name)()
        h.step('%s heads(kpts=False)' % precision)
        h.plan.heads(False)
        h.step('%s heads, overlap False' % precision)
        h.plan.overlap = False
        h.plan.heads()
        h.plan.overlap = None
        h.step('%s as_f32' % precision)
        h.plan.as_f32(h.plan.p2)
        h.plan.as_f32(h.plan.sem)
    h.step('fpn leaves overlap as it was', overlap=h.plan.overlap)


def case_rpn_entry_point_switches(h):
    _f16x3(h)
    for g in ('0', 'small', 'all'):
        for hf in (False, True):
            engine.RPN_GROUP, engine.RPN_HEAD_FUSION = g, hf
            h.step('rpn group %s head fusion %s' % (g, hf))
            h.plan.rpn()
            h.step('nparts', rpn_nparts=list(h.plan.rpn_nparts))
    engine.RPN_GROUP, engine.RPN_HEAD_FUSION, h.used = '0', True, (2, 2, 8, 2, 1)
    h.plan.rpn()


def _kept_args(h):
    p = h.plan
    a = {'rois_left_b': on_device(torch.zeros(p.post, 5)), 'keep_idx': on_device(torch.zeros(p.post, dtype=torch.int32)),
         'num': on_device(torch.zeros(1, dtype=torch.int32)), 'im_info': torch.tensor([[float(H_IN), float(W_IN), 1.0]]),
         'det_kpts': on_device(torch.zeros(p.post, 5))}
    h.extra.update(('arg.' + k, v) for k, v in a.items())
    h.invalidate()
    return a


def case_kpts_for_kept(h):
    fixed_shifts(h.w)
    a = _kept_args(h)
    for precision, before in (('f16x3', 'f32'), ('f32', 'f16x3')):
        engine.PRECISION = before
        h.step('kpts_for_kept ' + precision)
        h.plan.kpts_for_kept(a['rois_left_b'], a['keep_idx'], a['num'], a['im_info'], a['det_kpts'], precision)
        h.step('after', PRECISION=engine.PRECISION, fmt=h.plan.fmt)
    engine.KPTS_HEAD_FUSION = 'mfma'
    h.step('kpts_for_kept f16x3 mfma head')
    h.plan.kpts_for_kept(a['rois_left_b'], a['keep_idx'], a['num'], a['im_info'], a['det_kpts'], 'f16x3')


def _calibration(h):
    return {'shifts': dict(h.w.shifts), 'fuse_shortcut': list(h.w.fuse_shortcut), 'calib_epoch': h.w.calib_epoch,
            'calibration_frames': getattr(h.w, 'calibration_frames', None), 'calibrated': h.w.calibrated,
            'calibration_max': dict(h.w.calibration_max), 'packed_fmt': h.plan.packed_fmt, 'PRECISION': engine.PRECISION,
            'fmt': h.plan.fmt, 'overlap': h.plan.overlap}


def case_calibrate_plain_then_merge(h):
    h.fill = True
    engine.PRECISION, h.plan.fmt, h.plan.overlap, h.plan.packed_fmt = 'f16x3', S16, True, S16
    h.plan.calibrate()
    h.step('after calibrate()', **_calibration(h))
    h.n_launches = 5                          # other constants: the second frame's maxima differ from the first's
    h.plan.calibrate(merge=True)
    h.step('after calibrate(merge=True)', **_calibration(h))
    h.n_launches = 0
    h.plan.calibrate()                        # the first frame again: same shifts as the first time, another epoch only if they differ
    h.step('after calibrate() again', **_calibration(h))
    h.n_launches = 0
    h.plan.calibrate()
    h.step('same frame, same shifts: the epoch stays', **_calibration(h))


def case_calibrate_blank_frame(h):
    h.fill = True
    h.fill_by_name = {'stem': 0.0}
    h.plan.packed_fmt = S16
    h.plan.calibrate()
    h.step('blank frame refused', **_calibration(h))
    h.fill_by_name = {'stem': float('inf')}
    h.plan.calibrate()
    h.step('non-finite frame refused', **_calibration(h))
    h.w.calibration_max = {'stem': 4.0}
    h.fill_by_name = {'stem': 0.0}
    h.plan.calibrate(merge=True)
    h.step('blank frame merged with an earlier one', **_calibration(h))


def case_calibrate_shortcut_window(h):
    h.fill = True
    for diff in (-7, -6, 4, 5):
        # shift = round(log2(2048 / max)): the block input's minus conv2's output's = diff
        h.fill_by_name = {'stem': 2048.0 / 2 ** 8, 'layer1.0.conv2': 2048.0 / 2 ** (8 - diff)}
        h.n_launches = 0
        h.plan.calibrate()
        h.step('shifts[stem] - shifts[L1.0.m2] = %d' % diff, stem=h.w.shifts['stem'], m2=h.w.shifts['L1.0.m2'],
               fuse_shortcut=list(h.w.fuse_shortcut), calib_epoch=h.w.calib_epoch)


def _inputs(h, B=1):
    a = {'left': on_device(torch.zeros(B, 3, H_IN, W_IN)), 'right': on_device(torch.zeros(B, 3, H_IN, W_IN)),
         'info': torch.tensor([[float(H_IN), float(W_IN), 1.0]] * B)}
    h.extra.update(('arg.' + k, v) for k, v in a.items())
    h.invalidate()
    return a


def _src(h):
    p = h.plan
    return {'src': [h.label_of(t.data_ptr()) for t in p._src], 'packed_fmt': p.packed_fmt}


def case_driver_set_inputs(h):
    fixed_shifts(h.w)
    a = _inputs(h)
    p = h.plan
    p.set_inputs(a['left'], a['right'], a['info'])
    h.step('set_inputs by reference', same_objects=p._src[0] is a['left'] and p._src[1] is a['right'], **_src(h))
    p.run(precision='f16x3')
    h.step('after run', **_src(h))
    p.run(precision='f16x3')
    h.step('after second run without new inputs', **_src(h))
    p.set_inputs(a['left'], a['right'], a['info'], copy=True)
    h.step('set_inputs copy=True', **_src(h))
    p.run(precision='f32')
    wide = torch.zeros(1, 3, H_IN, W_IN + 5)
    h.extra['arg.wide'] = wide
    h.invalidate()
    p.set_inputs(a['left'], on_device(wide[..., :W_IN]), a['info'])
    h.step('set_inputs non-contiguous', **_src(h))
    p.set_inputs(a['left'].double(), a['right'], a['info'])
    h.step('set_inputs float64', **_src(h))
    p.set_inputs(torch.zeros(1, 3, H_IN, W_IN), a['right'], a['info'])
    h.step('set_inputs host tensor', **_src(h))
    p.run(precision='f16x3', kpts=False)
    h.step('after run(kpts=False)', PRECISION=engine.PRECISION, **_src(h))


def case_driver_set_images_and_pack_inputs(h):
    fixed_shifts(h.w)
    a = _inputs(h)
    p = h.plan
    imgs = {'img_left': on_device(torch.zeros(32, 48, 3, dtype=torch.uint8)), 'img_right': on_device(torch.zeros(32, 48, 3, dtype=torch.uint8))}
    h.extra.update(('arg.' + k, v) for k, v in imgs.items())
    h.invalidate()
    p.set_inputs(a['left'], a['right'], a['info'])
    scale = p.set_images(imgs['img_left'], imgs['img_right'], 'f16x3', 64)
    h.step('set_images f16x3', scale=scale, **_src(h))
    p.run(precision='f16x3')
    h.step('after run', **_src(h))
    p.run(precision='f16x3')
    h.step('after second run', **_src(h))
    p.set_images(imgs['img_left'], imgs['img_right'], target_short=64)
    h.step('set_images f32', **_src(h))
    p.run(precision='f16x3')                       # packed in the other format: packs again
    h.step('after f16x3 run on f32-packed images', **_src(h))
    p.set_inputs(a['left'], a['right'], a['info'])
    p.pack_inputs(S16)
    h.step('pack_inputs', **_src(h))
    p.run(precision='f16x3')
    h.step('after run', **_src(h))
    p.pack_inputs(F32)
    p.run(precision='f16x3')
    h.step('after f16x3 run on f32-packed inputs', **_src(h))


def case_driver_programs(h):
    fixed_shifts(h.w)
    a = _inputs(h)
    p = h.plan
    imgs = on_device(torch.zeros(32, 48, 3, dtype=torch.uint8))
    h.extra['arg.img'] = imgs
    p.set_inputs(a['left'], a['right'], a['info'])
    h.step('first run: records')
    p.run(precision='f16x3', use_program=True)
    h.step('after', programs=sorted(repr(k) for k in p.programs), **_src(h))
    h.step('second run: replays')
    p.run(precision='f16x3', use_program=True)
    h.step('after', **_src(h))
    p.set_images(imgs, imgs, 'f16x3', 64)
    h.step('replay on set_images input')
    p.run(precision='f16x3', use_program=True)
    h.step('other key: kpts=False')
    p.run(precision='f16x3', use_program=True, kpts=False)
    h.step('other key: overlap False')
    p.overlap = False
    p.run(precision='f16x3', use_program=True)
    p.overlap = None
    h.step('other key: f32')
    p.run(precision='f32', use_program=True)
    h.step('after', programs=sorted(repr(k) for k in p.programs), PRECISION=engine.PRECISION)
    h.w.calib_epoch += 1
    h.step('calib_epoch bumped')
    p.run(precision='f16x3', use_program=True)
    h.step('after', programs=sorted(repr(k) for k in p.programs), epoch=repr(p._epoch))
    engine.PLAN_EPOCH += 1
    h.step('PLAN_EPOCH bumped')
    p.run(precision='f16x3', use_program=True)
    h.step('after', programs=sorted(repr(k) for k in p.programs), epoch=repr(p._epoch))
    engine.set_tune_mode('concurrent', 4)
    h.step('tune mode changed, eager run')
    p.run(precision='f16x3')
    h.step('after', programs=sorted(repr(k) for k in p.programs), epoch=repr(p._epoch), keys=[repr(p.program_key('f16x3', True)),
           repr(p.program_key('f32', False, par=0))])


def case_run_uncalibrated(h):
    h.fill = True
    a = _inputs(h)
    h.plan.set_inputs(a['left'], a['right'], a['info'])
    h.plan.run(precision='f16x3')
    h.step('calibrated by the first f16x3 run', **_calibration(h))
    h.w.calibrated, h.w.shifts = False, {}
    engine.ACT_SCALES = False
    h.plan.run(precision='f16x3')
    h.step('ACT_SCALES off: no calibration', **_calibration(h))


RESULTS = ('rois_left', 'rois_right', 'cls_prob', 'bbox_pred', 'dim_orien', 'kpts_prob', 'left_prob', 'right_prob')


def _outputs(h, name, **kw):
    p = h.plan
    before = {n: getattr(p, n).data_ptr() for n in RESULTS}
    res = p.outputs(**kw)
    after = {n: getattr(p, n).data_ptr() for n in RESULTS}
    attr = {'dim_orien_pred': 'dim_orien', 'left_border_prob': 'left_prob', 'right_border_prob': 'right_prob'}
    what = {}
    for k in sorted(res):
        n = attr.get(k, k)
        if res[k] is None:
            what[k] = None
        else:
            ptr = res[k].data_ptr()
            what[k] = ['the plan\'s buffer, still its own' if ptr == after[n] else 'the plan\'s buffer, handed over' if ptr == before[n]
                       else 'fresh', list(res[k].shape)]
    h.step(name, results=what, replaced=[n for n in RESULTS if before[n] != after[n]])
    h.invalidate()
    return res               # kept alive by the caller: a freed result's address could be handed out again


def case_outputs(h):
    keep = []
    for kpts in (True, False):
        keep.append(_outputs(h, 'eager, kpts=%s' % kpts, kpts=kpts))
        keep.append(_outputs(h, 'alias, kpts=%s' % kpts, kpts=kpts, alias=True))
    h.plan.programs[('f16x3', True, True, False)] = ('program#0', [])
    for kpts in (True, False):
        keep.append(_outputs(h, 'a program exists, kpts=%s' % kpts, kpts=kpts))
        keep.append(_outputs(h, 'a program exists, alias, kpts=%s' % kpts, kpts=kpts, alias=True))
    h.plan.programs, h.plan.graphs = {}, {'f16x3': object()}
    keep.append(_outputs(h, 'a graph exists', kpts=True))


CASES = {name[5:]: fn for name, fn in sorted(globals().items()) if name.startswith('case_') and callable(fn)}
CASES.update(('launch_' + k, _launch_case(v)) for k, v in LAUNCH_CASES.items())
BATCH = {'launch_default_B2': 2}


def run_case(name):
    h = Harness(build=False)
    with patched(h):
        h.plan = Plan(h.w, BATCH.get(name, 1), H_IN, W_IN)
        CASES[name](h)
        out = {'log': h.events, 'state': h.state()}
    return json.loads(json.dumps(out))            # tuples -> lists, as the golden file holds them


def load_golden():
    with gzip.open(GOLDEN, 'rt') as f:
        g = json.load(f)
    return g, {name: {'log': [g['events'][i] for i in c['log']], 'state': c['state']} for name, c in g['cases'].items()}


@pytest.fixture(scope='module')
def golden():
    return load_golden()[1]


@pytest.mark.parametrize('name', sorted(CASES))
def test_plan_host_characterisation(golden, name):
    assert sorted(golden) == sorted(CASES)
    got, want = run_case(name), golden[name]
    assert len(got['log']) == len(want['log']), name
    for i, (g, w) in enumerate(zip(got['log'], want['log'])):
        assert g == w, '%s: event %d' % (name, i)
    assert got['state'] == want['state'], name


def test_no_raw_address_in_the_golden_file():
    g, cases = load_golden()
    assert len(g['header']['recorded_at_commit']) >= 7

    def numbers(v):
        if isinstance(v, dict):
            for x in v.values():
                for r in numbers(x):
                    yield r
        elif isinstance(v, list):
            for x in v:
                for r in numbers(x):
                    yield r
        elif isinstance(v, int):
            yield v
    assert max(numbers(g['events'])) < (1 << 24)
    assert '<unlabelled>' not in json.dumps(g)


def test_patches_are_undone():
    before = (_lib.lib, _lib.stream, _lib.workspace, engine.conv2d, engine.PRECISION, engine.DEBUG_SKIP, torch.cuda.current_stream,
              torch.cuda.Event, streams.side_streams, engine.TUNE_MODE, engine.TUNE_STREAMS)
    run_case('driver_programs')
    assert before == (_lib.lib, _lib.stream, _lib.workspace, engine.conv2d, engine.PRECISION, engine.DEBUG_SKIP, torch.cuda.current_stream,
                      torch.cuda.Event, streams.side_streams, engine.TUNE_MODE, engine.TUNE_STREAMS)


def _record():
    commit = subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=HERE).decode().strip()
    dirty = subprocess.check_output(['git', 'status', '--porcelain', '--', os.path.relpath(plan_mod.__file__, HERE)], cwd=HERE).decode().strip()
    events, index, cases = [], {}, {}
    for name in sorted(CASES):
        c = run_case(name)
        log = []
        for e in c['log']:
            key = json.dumps(e, sort_keys=True)
            if key not in index:
                index[key] = len(events)
                events.append(key)
            log.append(index[key])
        cases[name] = {'log': log, 'state': c['state']}
    with open(GOLDEN, 'wb') as raw, gzip.GzipFile(filename='', mode='wb', fileobj=raw, mtime=0) as gz, io.TextIOWrapper(gz) as f:
        f.write('{"header": %s,\n"events": [\n' % json.dumps({
            'recorded_at_commit': commit, 'plan_py_modified_since': bool(dirty),
            'what': 'stereo_rcnn_amd/model/stereo_rcnn/plan.py as of that commit, driven by tests/test_plan_host_cpu.py --record'},
            sort_keys=True))
        f.write(',\n'.join(events))
        f.write('\n],\n"cases": {\n')
        f.write(',\n'.join('%s: %s' % (json.dumps(n), json.dumps(cases[n], sort_keys=True, separators=(',', ':'))) for n in sorted(cases)))
        f.write('\n}}\n')
    print('wrote %s: %d cases, %d distinct events, %d bytes' % (GOLDEN, len(cases), len(events), os.path.getsize(GOLDEN)))


def _time():
    """Host time of one eager launch_all() walk under the stubs: five medians of 20 walks each (ms)."""
    h = Harness(build=False)
    with patched(h):
        h.plan = Plan(h.w, 1, H_IN, W_IN)
        _f16x3(h)
        medians = []
        for _ in range(6):
            ts = []
            for _ in range(20):
                h.events = []
                t0 = time.perf_counter()
                h.plan.launch_all()
                ts.append((time.perf_counter() - t0) * 1e3)
            medians.append(sorted(ts)[len(ts) // 2])
    medians = medians[1:]                              # the first block warms the interpreter up
    print('launch_all() under the stubs, median of 20 walks, five times (ms):', ' '.join('%.3f' % m for m in medians),
          '| median %.3f, spread %.3f' % (sorted(medians)[2], max(medians) - min(medians)))


if __name__ == '__main__':
    if sys.argv[1:] == ['--record']:
        _record()
    elif sys.argv[1:] == ['--time']:
        _time()
    elif sys.argv[1:] == ['--dump']:
        with gzip.open(GOLDEN, 'rt') as f:
            sys.stdout.write(f.read())
    else:
        sys.exit('usage: python tests/test_plan_host_cpu.py --record | --dump | --time   (--record writes %s from the plan.py it runs on)' % GOLDEN)
