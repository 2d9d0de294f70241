"""CPU: the batch assembly entry points of csrc/loader.hip (srcnn_gt_batch, srcnn_preprocess_train) are declared in
include/srcnn_hip.h ("training: batch assembly"), bound in _lib.py with matching argument lists, and validate every argument
before their launch, so each refusal is checkable on a host without a GPU -- the pattern of tests/test_optim_abi_cpu.py.  No call
here reaches a launch."""
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


def _header():
    from stereo_rcnn_amd import _lib
    return open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'srcnn_hip.h')).read()


def test_header_constants_and_bindings(L):
    from stereo_rcnn_amd import _lib
    header = _header()
    assert 'training: batch assembly' in header
    assert '#define SRCNN_LOADER_MAX_BATCH %d\n' % _lib.LOADER_MAX_BATCH in header
    assert '#define SRCNN_GT_COLS %d\n' % _lib.GT_COLS in header
    assert '#define SRCNN_GT_MAX_ROWS %d\n' % _lib.GT_MAX_ROWS in header
    # the slots travel in the kernels' arguments: within HIP's 4096 bytes
    assert _lib.LOADER_MAX_BATCH * 48 + 64 <= 4096 and ctypes.sizeof(_lib.GtSlot) == 16 and ctypes.sizeof(_lib.TrainImage) == 40
    for name in ('srcnn_gt_batch', 'srcnn_preprocess_train'):
        m = re.search(r'SRCNN_API int %s\((.*?)\);' % name, header, re.S)
        assert m, name
        n_args = len([a for a in m.group(1).split(',') if a.strip()])
        assert n_args == len(_lib._SIGNATURES[name][1]), name
        assert getattr(L, name)


def _slots(*v):
    from stereo_rcnn_amd import _lib
    return (_lib.GtSlot * len(v))(*[_lib.GtSlot(*s) for s in v])


def test_gt_batch_refusals(L):
    f = L.srcnn_gt_batch    # (table, table_rows, slots, B, keys, key_stride, K, left, right, merge, dim_orien, kpts, num_boxes, stream)
    ok = _slots((0, 4, 1.6, 100.0))
    outs = [P] * 6
    _refused(L, f(P, 8, None, 1, P, 8, 30, *outs, None), b'null slots')
    _refused(L, f(P, 8, ok, 0, P, 8, 30, *outs, None), b'B must be')
    _refused(L, f(P, 8, ok, 17, P, 8, 30, *outs, None), b'B must be')
    _refused(L, f(P, 8, ok, 1, P, 8, 0, *outs, None), b'K must be')
    _refused(L, f(P, -1, ok, 1, P, 8, 30, *outs, None), b'negative')
    for i in range(6):
        bad = list(outs)
        bad[i] = None
        _refused(L, f(P, 8, ok, 1, P, 8, 30, *bad, None), b'null output')
    _refused(L, f(P, 8, _slots((0, -1, 1.6, 100.0)), 1, P, 8, 30, *outs, None), b'negative row range')
    _refused(L, f(P, 8, _slots((-2, 1, 1.6, 100.0)), 1, P, 8, 30, *outs, None), b'negative row range')
    _refused(L, f(P, 8, _slots((6, 4, 1.6, 100.0)), 1, P, 8, 30, *outs, None), b'beyond the table')
    _refused(L, f(P, 1 << 20, _slots((0, 513, 1.6, 100.0)), 1, P, 1024, 30, *outs, None), b'SRCNN_GT_MAX_ROWS')
    _refused(L, f(P, 8, ok, 1, P, 3, 30, *outs, None), b'key_stride')
    _refused(L, f(P, 8, _slots((0, 4, 0.0, 100.0)), 1, P, 8, 30, *outs, None), b'im_scale')
    _refused(L, f(P, 8, _slots((0, 4, float('nan'), 100.0)), 1, P, 8, 30, *outs, None), b'im_scale')
    _refused(L, f(None, 8, ok, 1, P, 8, 30, *outs, None), b'null table')
    _refused(L, f(P, 8, ok, 1, None, 8, 30, *outs, None), b'null table')
    # the second slot is checked as the first is
    _refused(L, f(P, 8, _slots((0, 4, 1.6, 100.0), (4, 5, 1.6, 100.0)), 2, P, 8, 30, *outs, None), b'beyond the table')


def _images(*v):
    from stereo_rcnn_amd import _lib
    return (_lib.TrainImage * len(v))(*[_lib.TrainImage(*s) for s in v])


def test_preprocess_train_refusals(L):
    f = L.srcnn_preprocess_train          # (slots, B, Hmax, Wmax, max_size, out_left, out_right, stream)
    ok = _images((P, P, 375, 1242, 0, 1.6))
    _refused(L, f(None, 1, 600, 1987, 2484, P, P, None), b'null slots')
    _refused(L, f(ok, 0, 600, 1987, 2484, P, P, None), b'B must be')
    _refused(L, f(ok, 17, 600, 1987, 2484, P, P, None), b'B must be')
    _refused(L, f(ok, 1, 0, 1987, 2484, P, P, None), b'positive')
    _refused(L, f(ok, 1, 600, 1987, 0, P, P, None), b'positive')
    _refused(L, f(ok, 1, 600, 1987, 2484, None, P, None), b'null output')
    _refused(L, f(ok, 1, 600, 1987, 2484, P, P + 4, None), b'aligned')
    _refused(L, f(_images((None, P, 375, 1242, 0, 1.6)), 1, 600, 1987, 2484, P, P, None), b'null image')
    _refused(L, f(_images((P, P, 0, 1242, 0, 1.6)), 1, 600, 1987, 2484, P, P, None), b'image size')
    _refused(L, f(_images((P, P, 375, 1242, 0, -1.0)), 1, 600, 1987, 2484, P, P, None), b'bad scale')
    _refused(L, f(_images((P, P, 375, 1242, 0, float('inf'))), 1, 600, 1987, 2484, P, P, None), b'bad scale')
    _refused(L, f(ok, 1, 599, 1987, 2484, P, P, None), b'exceeds')             # OH = 600
    _refused(L, f(ok, 1, 600, 1986, 2484, P, P, None), b'exceeds')             # OW = 1987
    _refused(L, f(_images((P, P, 375, 1242, 0, 1.6), (P, P, 376, 1241, 1, 1.6)), 2, 600, 1987, 2484, P, P, None), b'exceeds')


def test_python_wrappers_refuse_what_the_kernels_do_not_take():
    import torch
    from stereo_rcnn_amd import engine
    img = torch.zeros((8, 13, 3), dtype=torch.uint8)          # pageable host memory
    with pytest.raises(AssertionError):
        engine.preprocess_train([(img, img)], [False], [1.6])
    with pytest.raises(AssertionError):
        engine.gt_batch(torch.zeros((4, 24)), [(0, 4, 1.6, 100.0)], torch.zeros((1, 4), dtype=torch.int32), 30)


def test_driver_refuses_a_pre_nms_top_n_the_proposal_kernel_cannot_rank(monkeypatch, capsys, tmp_path):
    from stereo_rcnn_amd import trainval_net
    from stereo_rcnn_amd.model.utils.config import cfg
    monkeypatch.setattr(cfg.TRAIN, 'RPN_PRE_NMS_TOP_N', 12000)
    assert trainval_net.main(['--kitti-path', str(tmp_path), '--split', str(tmp_path / 'train.txt')]) == []
    out = capsys.readouterr().out
    assert '12000' in out and '8192' in out and '--pre_nms_top_n' in out
