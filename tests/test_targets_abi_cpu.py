"""CPU: the target-layer entry points of the C ABI validate their arguments before any launch (include/srcnn_hip.h, "training
target layers") -- the pattern of tests/test_losses_abi_cpu.py.  No call here reaches a launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096            # a non-null "device pointer" (never dereferenced: every call below is refused first)
BIG = 1 << 20


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import _lib
    return _lib.lib()


def _refused(L, rc, text=None):
    assert rc in (-1, -3), rc
    if text is not None:
        assert text in L.srcnn_last_error(), L.srcnn_last_error()


def _anchor_params(**kw):
    from stereo_rcnn_amd import _lib
    v = dict(negative_overlap=0.3, positive_overlap=0.7, clobber_positives=0, batch_size=256, num_fg=128, inside_weight=1.0)
    v.update(kw)
    return _lib.AnchorTargetParams(**v)


def _proposal_params(**kw):
    from stereo_rcnn_amd import _lib
    c4, c5 = ctypes.c_float * 4, ctypes.c_float * 5
    v = dict(fg_thresh=0.5, bg_thresh_hi=0.5, bg_thresh_lo=0.0, rois_per_image=128, fg_rois_per_image=32, kpts_grid=28,
             bbox_means=c4(0, 0, 0, 0), bbox_stds=c4(.1, .1, .2, .2), dim_means=c5(1.6, 1.5, 4, 0, 0), dim_stds=c5(.5, .5, .5, .5, .5),
             inside_weights=c4(1, 1, 1, 1))
    v.update(kw)
    return _lib.ProposalTargetParams(**v)


def test_constants_and_structs_agree_with_the_header(L):
    from stereo_rcnn_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'srcnn_hip.h')).read()
    macro = lambda name: int(re.search(r'#define\s+%s\s+(\d+)' % name, hdr).group(1))
    assert macro('SRCNN_TARGETS_MAX_GT') == _lib.TARGETS_MAX_GT >= 30
    assert macro('SRCNN_TARGETS_MAX_ROIS') == _lib.TARGETS_MAX_ROIS >= 2030
    assert macro('SRCNN_TARGETS_MAX_BATCH_ROIS') == _lib.TARGETS_MAX_BATCH_ROIS >= 512
    assert ctypes.sizeof(_lib.AnchorTargetParams) == 24 and ctypes.sizeof(_lib.ProposalTargetParams) == 24 + 22 * 4
    assert L.srcnn_version() >= 270


def test_workspace_queries(L):
    a, p = L.srcnn_anchor_targets_workspace_bytes, L.srcnn_proposal_targets_workspace_bytes
    assert a(1, 30) >= (30 + 2) * 4 and a(4, 64) >= 4 * (64 + 2) * 4 and a(4, 64) % 256 == 0
    assert a(0, 30) == 0 and a(-1, 30) == 0 and a(1, 0) == 0 and a(1, 65) == 0
    assert p(1, 2000, 30) > 0 and p(0, 2000, 30) == 0 and p(1, 2000, 65) == 0 and p(1, 4096, 1) == 0 and p(1, -5, 3) == 0


def test_anchor_targets_argument_errors(L):
    def call(anchors=P, N=1000, gl=P, gr=P, gm=P, B=2, K=30, im=P, fk=P, bk=P, params='default', labels=P, tl=P, tr=P, iw=P, ow=P,
             mo=None, ws=P, ws_bytes=BIG):
        prm = _anchor_params() if params == 'default' else params
        return L.srcnn_anchor_targets(anchors, N, gl, gr, gm, B, K, im, fk, bk, ctypes.byref(prm) if prm is not None else None,
                                      labels, tl, tr, iw, ow, mo, ws, ws_bytes, None)
    for name in ('anchors', 'gl', 'gr', 'gm', 'im', 'fk', 'bk', 'labels', 'tl', 'tr', 'iw', 'ow'):
        _refused(L, call(**{name: None}), b'null')
    _refused(L, call(params=None), b'null params')
    _refused(L, call(K=65), b'SRCNN_TARGETS_MAX_GT')
    _refused(L, call(K=0), b'K must')
    _refused(L, call(N=-1), b'sizes')
    _refused(L, call(N=0), b'sizes')
    _refused(L, call(B=-2), b'sizes')
    _refused(L, call(B=4, N=1 << 30), b'2^31')
    _refused(L, call(params=_anchor_params(num_fg=257)), b'quota')
    _refused(L, call(params=_anchor_params(num_fg=-1)), b'quota')
    _refused(L, call(params=_anchor_params(batch_size=-1, num_fg=0)), b'batch_size')
    _refused(L, call(anchors=P + 4), b'aligned')
    assert call(ws_bytes=8) == -3 and b'workspace' in L.srcnn_last_error()
    assert call(ws=None) == -3


def test_proposal_targets_argument_errors(L):
    def call(rl=P, rr=P, B=2, R=2000, gl=P, gr=P, gd=P, gk=P, K=30, fk=P, u=P, params='default', outs=(P,) * 11, keep=None, ws=P,
             ws_bytes=BIG):
        prm = _proposal_params() if params == 'default' else params
        return L.srcnn_proposal_targets(rl, rr, B, R, gl, gr, gd, gk, K, fk, u, ctypes.byref(prm) if prm is not None else None,
                                        *outs, keep, ws, ws_bytes, None)
    for name in ('rl', 'rr', 'gl', 'gr', 'gd', 'gk', 'fk', 'u'):
        _refused(L, call(**{name: None}), b'null input')
    for i in range(11):                                    # the ten outputs and the status word
        _refused(L, call(outs=(P,) * i + (None,) + (P,) * (10 - i)), b'null output')
    _refused(L, call(params=None), b'null params')
    _refused(L, call(K=65), b'SRCNN_TARGETS_MAX_GT')
    _refused(L, call(R=-1), b'sizes')
    _refused(L, call(B=0), b'sizes')
    _refused(L, call(R=4090, K=30), b'SRCNN_TARGETS_MAX_ROIS')
    _refused(L, call(params=_proposal_params(rois_per_image=2000, fg_rois_per_image=10)), b'rois_per_image')
    _refused(L, call(params=_proposal_params(rois_per_image=0, fg_rois_per_image=0)), b'rois_per_image')
    _refused(L, call(params=_proposal_params(fg_rois_per_image=129)), b'quota')
    _refused(L, call(params=_proposal_params(fg_rois_per_image=-1)), b'quota')
    _refused(L, call(params=_proposal_params(kpts_grid=0)), b'kpts_grid')
    _refused(L, call(params=_proposal_params(bbox_stds=(ctypes.c_float * 4)(.1, 0, .2, .2))), b'std')
    assert call(ws_bytes=8) == -3 and b'workspace' in L.srcnn_last_error()
    assert call(ws=None) == -3


def test_python_entry_points_refuse_cpu_tensors():
    import torch
    from stereo_rcnn_amd.model.rpn.anchor_target_layer import _AnchorTargetLayer, as_key_bits
    from stereo_rcnn_amd.model.rpn.proposal_target_layer import _ProposalTargetLayer
    from stereo_rcnn_amd.model.utils.config import cfg
    gt = torch.zeros(1, 30, 5)
    with pytest.raises(NotImplementedError):
        _AnchorTargetLayer(cfg.FEAT_STRIDE, cfg.ANCHOR_RATIOS)((torch.zeros(1), gt, gt, gt, torch.tensor([[192., 320., 1.]]), None,
                                                                [(48, 80), (24, 40), (12, 20), (6, 10), (3, 5)]))
    with pytest.raises(NotImplementedError):
        _ProposalTargetLayer(2)(torch.zeros(1, 8, 5), torch.zeros(1, 8, 5), gt, gt, torch.zeros(1, 30, 5), torch.zeros(1, 30, 6), None)
    assert (cfg.TRAIN.RPN_BATCHSIZE, cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.FG_FRACTION, cfg.MAX_NUM_GT_BOXES) == (512, 512, 0.25, 30)
    bits = as_key_bits(torch.tensor([0, 1, 2 ** 31, 2 ** 32 - 1]))
    assert bits.dtype == torch.int32 and bits.tolist() == [0, 1, -2 ** 31, -1]
