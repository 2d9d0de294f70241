"""CPU: srcnn_prep_weights (csrc/prep_weights.hip) is declared in include/srcnn_hip.h ("weight preparation"), bound in _lib.py
with a matching argument list and descriptor, and validates every argument before its first launch, so each refusal is checkable
on a host without a GPU -- the pattern of tests/test_loader_abi_cpu.py.  No call here reaches a launch.  Also: the validation
flags of the training driver parse and default to off, and the driver's refusal of a pre-NMS top N the proposal kernel cannot
rank is what it was, with or without them."""
import ctypes
import os
import re

import pytest

P = 4096            # a non-null, 16-byte aligned "device pointer" (never dereferenced: every call below is refused first)


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import _lib
    return _lib.lib()


def _refused(L, rc, text, code=-1):
    assert rc == code, rc
    assert text in L.srcnn_last_error(), L.srcnn_last_error()


def _layer(**kw):
    """A valid 3x3 layer (8, 32, 3, 3) with a bias, then the overrides."""
    from stereo_rcnn_amd import _lib
    d = _lib.PrepLayer()
    d.form, d.n_src, d.kh, d.kw, d.cin, d.alias_of = _lib.PREP_CONV, 1, 3, 3, 32, -1
    d.cout[0] = 8
    d.w[0], d.b[0], d.dst_w, d.dst_b = P, P, P, P
    for k, v in kw.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(d, k)[i] = x
        else:
            setattr(d, k, v)
    return d


def _call(L, layers, k_out=P, ws=P, ws_bytes=1 << 12):
    from stereo_rcnn_amd import _lib
    arr = (_lib.PrepLayer * max(1, len(layers)))(*layers)
    return L.srcnn_prep_weights(arr, len(layers), k_out, ws, ws_bytes, None)


def test_header_constants_and_bindings(L):
    from stereo_rcnn_amd import _lib
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'srcnn_hip.h')).read()
    assert 'weight preparation' in header
    assert '#define SRCNN_PREP_LAYERS_PER_LAUNCH %d\n' % _lib.PREP_LAYERS_PER_LAUNCH in header
    for name, v in (('CONV', _lib.PREP_CONV), ('SHORTCUT', _lib.PREP_SHORTCUT), ('STEM', _lib.PREP_STEM), ('DECONV2X2', _lib.PREP_DECONV2X2)):
        assert '#define SRCNN_PREP_%s %d\n' % (name, v) in header
    # the descriptors travel in the kernels' arguments: within HIP's 4096 bytes
    assert ctypes.sizeof(_lib.PrepLayer) == 200 and _lib.PREP_LAYERS_PER_LAUNCH * (200 + 4 + 2 + 2 + 1) + 32 <= 4096
    m = re.search(r'SRCNN_API int srcnn_prep_weights\((.*?)\);', header, re.S)
    assert m and len([a for a in m.group(1).split(',') if a.strip()]) == len(_lib._SIGNATURES['srcnn_prep_weights'][1])
    assert L.srcnn_prep_weights_workspace_bytes(0) == 0 and L.srcnn_prep_weights_workspace_bytes(200) >= 800


def test_refusals(L):
    from stereo_rcnn_amd import _lib
    _refused(L, L.srcnn_prep_weights(None, 1, P, P, 4096, None), b'null layers_host')
    _refused(L, _call(L, []), b'n_layers must be')
    _refused(L, _call(L, [_layer()], k_out=None), b'null k_out')
    _refused(L, _call(L, [_layer()], ws=None), b'null k_out / workspace')
    _refused(L, _call(L, [_layer()], k_out=P + 2), b'aligned')
    _refused(L, _call(L, [_layer()], ws_bytes=2), b'workspace too small', code=-3)
    _refused(L, _call(L, [_layer(form=7)]), b'unknown form')
    _refused(L, _call(L, [_layer(dst_w=None)]), b'null dst_w')
    _refused(L, _call(L, [_layer(w=(None,))]), b'null source weight')
    _refused(L, _call(L, [_layer(dst_hi=P)]), b'dst_hi and dst_lo')
    _refused(L, _call(L, [_layer(dst_frag=P)]), b'dst_frag needs')
    _refused(L, _call(L, [_layer(dst_w=P + 2)]), b'misaligned destination')
    _refused(L, _call(L, [_layer(w=(P + 2,))]), b'misaligned source')
    _refused(L, _call(L, [_layer(n_src=4)]), b'n_src')
    _refused(L, _call(L, [_layer(cin=0)]), b'cin must be')
    _refused(L, _call(L, [_layer(cout=(0,))]), b'cout must be')
    _refused(L, _call(L, [_layer(kh=0)]), b'kernel size')
    _refused(L, _call(L, [_layer(cin2=4)]), b'cin2 belongs')
    _refused(L, _call(L, [_layer(bn_g=(P,))]), b'frozen BN needs all')
    _refused(L, _call(L, [_layer(dst_b=None)]), b'dst_b goes with')
    _refused(L, _call(L, [_layer(n_src=2, cout=(8, 8), w=(P, P), b=(P, None))]), b'size mismatch')
    _refused(L, _call(L, [_layer(cout=(1 << 20,), cin=1 << 12)]), b'2^31')
    # the second layer is checked as the first is, and named
    _refused(L, _call(L, [_layer(), _layer(dst_w=None)]), b'layer 1: null dst_w')
    # the special forms
    bn = dict(bn_g=(P, P), bn_b=(P, P), bn_m=(P, P), bn_v=(P, P))
    short = dict(form=_lib.PREP_SHORTCUT, n_src=2, kh=1, kw=1, cin2=16, cout=(8, 8), w=(P, P), b=(None, None), **bn)
    assert _layer(**short).cin2 == 16
    _refused(L, _call(L, [_layer(**dict(short, cin2=0))]), b'needs cin2')
    _refused(L, _call(L, [_layer(**dict(short, cout=(8, 9)))]), b'size mismatch')
    _refused(L, _call(L, [_layer(**dict(short, kh=3))]), b'shortcut form is 1x1')
    _refused(L, _call(L, [_layer(**dict(short, bn_g=(P, None), bn_b=(P, None), bn_m=(P, None), bn_v=(P, None)))]), b'two frozen BNs')
    _refused(L, _call(L, [_layer(form=_lib.PREP_STEM, kh=7, kw=7, cin=4, bn_g=(P,), bn_b=(P,), bn_m=(P,), bn_v=(P,))]), b'stem form is 7x7')
    _refused(L, _call(L, [_layer(form=_lib.PREP_STEM, kh=7, kw=7, cin=3)]), b'stem form folds')
    _refused(L, _call(L, [_layer(form=_lib.PREP_DECONV2X2, kh=3, kw=3)]), b'deconvolution form is 2x2')
    _refused(L, _call(L, [_layer(form=_lib.PREP_DECONV2X2, kh=2, kw=2, b=(None,))]), b'carries a bias')
    # fragments and aliases
    _refused(L, _call(L, [_layer(dst_hi=P, dst_lo=P, dst_frag=P, frag_rows=8)]), b'fragments: a 1x1')
    _refused(L, _call(L, [_layer(kh=1, kw=1, dst_hi=P, dst_lo=P, dst_frag=P, frag_rows=4)]), b'frag_rows')
    _refused(L, _call(L, [_layer(alias_of=0)]), b'earlier layer')
    _refused(L, _call(L, [_layer(), _layer(alias_of=0, dst_w=P + 64)]), b'alias shares dst_w')


def test_python_wrapper_refuses_host_tensors():
    import torch
    from stereo_rcnn_amd import _lib, engine
    w = torch.zeros(8, 32, 3, 3)
    with pytest.raises(AssertionError):
        engine.PrepSpec(_lib.PREP_CONV, [w], None, (), torch.zeros(8 * 288)).fill(_lib.PrepLayer())


def test_weight_table_is_the_list_both_paths_walk():
    """Weights.__init__ and Weights.refresh share plan.weight_table: every prepared layer once, the fused forms named."""
    from stereo_rcnn_amd import fixture
    from stereo_rcnn_amd.model.stereo_rcnn import plan
    t = plan.weight_table(fixture.make_state_dict(3))
    names = [e['name'] for e in t]
    assert len(names) == len(set(names)) and names[0] == 'stem' and 'layer1.0.conv3_down' in names and 'rpn_conv_pair' in names
    assert {e['kind'] for e in t} == {'stem', 'conv', 'shortcut', 'pair', 'cat', 'top0', 'stack', 'deconv'}
    assert names.index('rpn_conv') < names.index('rpn_conv_pair')          # an alias names an earlier layer


def test_validation_flags_parse_and_default_to_off():
    from stereo_rcnn_amd import trainval_net
    a = trainval_net.parse_args(['--kitti-path', 'k', '--split', 's'])
    assert a.val_split is None and a.val_label_dir is None and a.val_every == 1 and a.val_precision == 'f16x3'
    a = trainval_net.parse_args(['--kitti-path', 'k', '--split', 's', '--val-split', 'v.txt', '--val-label-dir', 'l', '--val-every', '2',
                                 '--val-precision', 'f32'])
    assert (a.val_split, a.val_label_dir, a.val_every, a.val_precision) == ('v.txt', 'l', 2, 'f32')


@pytest.mark.parametrize('val', [False, True])
def test_driver_still_refuses_a_pre_nms_top_n_the_proposal_kernel_cannot_rank(val, monkeypatch, capsys, tmp_path):
    import sys
    from stereo_rcnn_amd import trainval_net
    from stereo_rcnn_amd.model.utils.config import cfg
    monkeypatch.setattr(cfg.TRAIN, 'RPN_PRE_NMS_TOP_N', 12000)
    argv = ['--kitti-path', str(tmp_path), '--split', str(tmp_path / 'train.txt')]
    if val:
        argv += ['--val-split', str(tmp_path / 'val.txt'), '--val-label-dir', str(tmp_path)]
    assert trainval_net.main(argv) == []
    out = capsys.readouterr().out
    assert out.strip() == trainval_net.PRE_NMS_ADVICE % (12000, 8192, 8192, 8192)
    assert '12000' in out and '8192' in out and '--pre_nms_top_n' in out
