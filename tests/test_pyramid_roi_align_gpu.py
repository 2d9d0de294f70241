"""GPU: the fused pyramid ROIAlign forward, srcnn_pyramid_roi_align, called through the C ABI in every configuration the forward
ships and in every kernel form the dispatch can reach (tests/pyramid_roi_align_ref.py: TABLE, BOX_HEAD, FORM0).

Every comparison with the exact reference is bit-equality; the only numeric bound is the derived gamma_7 x S against the
independent float64 reference (derivation in the reference module).  Output buffers start as a canary of a fixed bit pattern --
a NaN for float32 buffers, non-zero bytes for SPLIT16 ones -- and "untouched" means bit-identical to it.  A planted level tie
must equal the reference at a level a correct float32 evaluation can return (device_level_set), a decided roi at its level."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':                                   # the child process of test_row_pair_form_in_a_child_process
    sys.path.insert(0, ROOT)

import pyramid_roi_align_ref as R

pytestmark = pytest.mark.gpu

CANARY = {R.F32: 0x7FC0BEEF, R.SPLIT16: 0x5A5A5A5A}          # a quiet NaN with a payload; two float16 of 0x5A5A each


def _m():
    from stereo_rcnn_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _device_maps(mfmt, C, c0=0):
    """channels c0 .. c0 + C of the case's maps (the references are read at the same channels)"""
    return [torch.from_numpy(np.array(m[..., c0:c0 + C])).cuda() for m in R.map_bytes(mfmt)]


@functools.lru_cache(maxsize=None)
def _device_rois():
    return torch.from_numpy(np.array(R.build_case()['rois'])).cuda()


def canary(n, A, cstride, ofmt):
    return torch.full((n, A, A, cstride), CANARY[ofmt], dtype=torch.int32, device='cuda')


def call(cfg, out, coffset=None, limit=None, n=None, C=None, A=None, mfmt=None, ofmt=None, c0=0):
    """one srcnn_pyramid_roi_align call of a table entry into `out` (int32-typed); returns the status"""
    m = _m()
    C = cfg['C'] if C is None else C
    maps = _device_maps(cfg['mfmt'], 64 if C % 64 or C > R.CMAX else C, c0)        # (a refused channel count never reads the maps)
    rois = _device_rois()
    lim = None if limit is None else torch.tensor([limit], dtype=torch.int32, device='cuda')
    rc = m.lib().srcnn_pyramid_roi_align(m.ptr_array(maps), m.int_array(h for h, _ in R.MAP_HW), m.int_array(w for _, w in R.MAP_HW), C,
                                         float(R.IM_H), rois.data_ptr(), int(rois.shape[0]) if n is None else n,
                                         cfg['A'] if A is None else A, out.data_ptr(), cfg['cstride'],
                                         cfg['coffset'] if coffset is None else coffset, cfg['mfmt'] if mfmt is None else mfmt,
                                         cfg['ofmt'] if ofmt is None else ofmt, None if lim is None else lim.data_ptr(), m.stream())
    torch.cuda.synchronize()
    return rc


def run(cfg, **kw):
    """-> the whole output buffer as int32 numpy (n, A, A, cstride)"""
    m = _m()
    out = canary(len(R.build_case()['rois']), cfg['A'], cfg['cstride'], cfg['ofmt'])
    m.check(call(cfg, out, **kw))
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def table_output(i):
    out = run(R.TABLE[i])
    out.setflags(write=False)
    return out


def check_exact(got, cfg, counts=None, c0=0):
    """got (n, A, A, C) int32, the written channel slice: decided rois bit-equal to the reference at their level, a tie bit-equal to
    the reference at an admissible level"""
    c = R.build_case()
    C, A = cfg['C'], cfg['A']
    want = R.as_bits(R.expected(cfg['mfmt'], A)[..., c0:c0 + C], cfg['ofmt'])
    tie = c['kind'] == 'tie'
    same = (got == want).reshape(len(want), -1).all(1)
    bad = np.nonzero(~same & ~tie)[0]
    assert bad.size == 0, [(int(i), str(c['name'][i]), int((got[i] != want[i]).sum())) for i in bad[:8]]
    alt = R.as_bits(R.expected(cfg['mfmt'], A, alt=True)[..., c0:c0 + C], cfg['ofmt'])
    for j, i in enumerate(np.nonzero(tie)[0]):
        at = {int(c['level'][i]): bool(same[i]), int(c['alt'][i]): bool((got[i] == alt[j]).all())}
        went = [l for l in sorted(at) if at[l]]
        assert len(went) == 1, (str(c['name'][i]), at)                    # one of the two neighbouring levels, bit for bit
        assert went[0] in R.device_level_set(c['rois'][i]), (str(c['name'][i]), went, R.device_level_set(c['rois'][i]))
        if counts is not None:
            k = int(c['tie_k'][i])
            counts[(k, 'up' if went[0] == k - 1 else 'down')] = counts.get((k, 'up' if went[0] == k - 1 else 'down'), 0) + 1


def check_float64(got, cfg, c0=0):
    """every element within the derived bound of the float64 reference (a tie: of the reference at one of its two levels)"""
    c = R.build_case()
    C, A = cfg['C'], cfg['A']
    ref, bound = R.expected64(cfg['mfmt'], A)
    ok, err, allowed = R.within_bound(got, cfg['ofmt'], ref[..., c0:c0 + C], bound[..., c0:c0 + C])
    tie = np.nonzero(c['kind'] == 'tie')[0]
    ref2, bound2 = R.expected64(cfg['mfmt'], A, alt=True)
    ok2, _, _ = R.within_bound(got[tie], cfg['ofmt'], ref2[..., c0:c0 + C], bound2[..., c0:c0 + C])
    per_roi = ok.reshape(len(ok), -1).all(1)
    per_roi[tie] |= ok2.reshape(len(tie), -1).all(1)
    dec = np.ones(len(ok), bool)
    dec[tie] = False
    print('%s: uses %.3f of the derived bound' % (cfg['id'], float((err[dec] / np.maximum(allowed[dec], 1e-300)).max())))
    assert per_roi.all(), [(int(i), str(c['name'][i]), float(err[i].max())) for i in np.nonzero(~per_roi)[0][:8]]


def sliced(out, cfg, coffset=None):
    o = cfg['coffset'] if coffset is None else coffset
    return np.ascontiguousarray(out[..., o:o + cfg['C']])


def untouched(out, cfg, lo, hi):
    return bool((out[..., lo:hi] == CANARY[cfg['ofmt']]).all())


def test_roi_form_is_the_default(dev):
    assert os.environ.get('SRCNN_ROI_ALIGN_FORM') in (None, '1'), "the suite tests the shipped dispatch"


@pytest.mark.parametrize('i', range(len(R.TABLE)), ids=[c['id'] for c in R.TABLE])
def test_table_bit_exact(dev, i):
    cfg = R.TABLE[i]
    out = table_output(i)
    counts = {}
    check_exact(sliced(out, cfg), cfg, counts)
    print('%s: level ties went %s' % (cfg['id'], sorted(counts.items())))
    o, C = cfg['coffset'], cfg['C']
    assert untouched(out, cfg, 0, o) and untouched(out, cfg, o + C, cfg['cstride'])      # the rest of a pixel's channels


@pytest.mark.parametrize('i', range(len(R.TABLE)), ids=[c['id'] for c in R.TABLE])
def test_table_within_float64_bound(dev, i):
    cfg = R.TABLE[i]
    check_float64(sliced(table_output(i), cfg), cfg)


def test_box_head_two_calls_one_buffer(dev):
    """the shipped box head: C = 256, A = 7, SPLIT16 -> SPLIT16, channel stride 512, the left eye at offset 0 and the right eye at
    256 of ONE buffer.  The right eye reads other maps (channels 256..511 of the case), so that a half written to the wrong
    place cannot pass for the other."""
    cfg = R.BOX_HEAD
    n = len(R.build_case()['rois'])

    def both_eyes(out):
        _m().check(call(cfg, out, coffset=0))
        first = out.cpu().numpy()
        _m().check(call(cfg, out, coffset=256, c0=256))
        return first, out.cpu().numpy()

    first, both = both_eyes(canary(n, 7, 512, R.SPLIT16))
    counts = {}
    check_exact(sliced(first, cfg, 0), cfg, counts)
    assert untouched(first, cfg, 256, 512)                                   # the other half is still canary
    assert np.array_equal(both[..., :256], first[..., :256])                 # the second call leaves the first half alone
    check_exact(sliced(both, cfg, 256), cfg, c0=256)                         # whole buffer == the concatenated reference
    assert not np.array_equal(both[..., 256:], both[..., :256])
    check_float64(sliced(both, cfg, 0), dict(cfg, id='box-head-left'))
    check_float64(sliced(both, cfg, 256), dict(cfg, id='box-head-right'), c0=256)
    print('box head: level ties went %s' % sorted(counts.items()))
    # repeatability: the LDS hand-off sits behind a hand-written barrier -- three runs into fresh canaried buffers, bit-identical
    for _ in range(2):
        assert np.array_equal(both_eyes(canary(n, 7, 512, R.SPLIT16))[1], both)


CHILD_TIMEOUT = 240


def _child_main(outdir):
    """SRCNN_ROI_ALIGN_FORM=0 is read once per process: this process runs the FORM0 cases and leaves the raw output buffers."""
    assert os.environ.get('SRCNN_ROI_ALIGN_FORM') == '0'
    for cfg in R.FORM0:
        np.save(os.path.join(outdir, cfg['id'] + '.npy'), run(cfg))
    print('form0 done %d' % len(R.FORM0))


def test_row_pair_form_in_a_child_process(dev, tmp_path):
    """the row-pair form at C <= 256: blocks of 64 / (C / 8) output rows, the partial last block at A = 14 (C = 128: rows 12..15, of
    which two must return).  One fresh child process with the A/B switch; bit-equal to the exact reference and to this process's
    roi-form output of the same call."""
    env = dict(os.environ, SRCNN_ROI_ALIGN_FORM='0')
    res = subprocess.run([sys.executable, os.path.abspath(__file__), '--form0-child', str(tmp_path)], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'form0 done %d' % len(R.FORM0) in res.stdout
    for cfg in R.FORM0:
        got = np.load(str(tmp_path / (cfg['id'] + '.npy')))
        check_exact(got, cfg)
        assert np.array_equal(got, run(cfg)), cfg['id']                     # the roi form, in this process


@pytest.mark.parametrize('cfg', [R.TABLE[0]] + [c for c in R.TABLE if c['C'] == 320 and c['mfmt'] == c['ofmt']],
                         ids=lambda c: c['id'])
def test_roi_limit(dev, cfg):
    """a device-side roi count: rows below it as in the unlimited call, rows at or past it never written"""
    full = table_output(R.TABLE.index(cfg))
    n = full.shape[0]
    for limit in (0, 1, n - 1, n, n + 5):
        out = run(cfg, limit=limit)
        k = min(limit, n)
        assert np.array_equal(out[:k], full[:k]), limit
        assert (out[k:] == CANARY[cfg['ofmt']]).all(), limit


REFUSALS = [('channels not a multiple of 64', dict(C=96)), ('channels above 1024', dict(C=1088)), ('A = 9', dict(A=9)),
            ('map format 2', dict(mfmt=2)), ('output format 2', dict(ofmt=2)),
            ('SPLIT16 output at channel offset 4', dict(ofmt=R.SPLIT16, coffset=4))]


@pytest.mark.parametrize('what,kw', REFUSALS, ids=[w.replace(' ', '-') for w, _ in REFUSALS])
def test_refusals(dev, what, kw):
    cfg = dict(form='-', C=64, A=7, mfmt=R.F32, ofmt=R.F32, cstride=2048, coffset=0)
    n = len(R.build_case()['rois'])
    out = canary(n, 14, 2048, R.F32)                      # large enough for what any of the refused calls would have written
    rc = call(cfg, out, **kw)
    assert rc != 0, what
    msg = _m().lib().srcnn_last_error()
    assert msg and b'srcnn_pyramid_roi_align' in msg, msg
    assert (out.cpu().numpy() == CANARY[R.F32]).all()


def test_no_rois_is_ok_and_writes_nothing(dev):
    cfg = R.TABLE[0]
    out = canary(4, cfg['A'], cfg['cstride'], cfg['ofmt'])
    assert call(cfg, out, n=0) == 0
    assert (out.cpu().numpy() == CANARY[cfg['ofmt']]).all()


if __name__ == '__main__':
    assert sys.argv[1] == '--form0-child'
    _child_main(sys.argv[2])
