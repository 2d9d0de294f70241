"""CPU: the result visualisation entry points of csrc/overlay.hip (srcnn_render_overlay, srcnn_bev_lidar) are declared in
include/srcnn_hip.h ("result visualisation"), bound in _lib.py with matching argument lists, and validate every argument before any
HIP call, so each refusal is checkable on a host without a GPU -- the pattern of tests/test_loader_abi_cpu.py.  No call here
reaches a launch."""
import ctypes
import os
import re

import pytest

P = 4096            # a non-null, 16-byte aligned "device pointer" (never dereferenced: every call below is refused first)
FAR = 1 << 30       # another one, far from P: a panel there overlaps nothing at P


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
    from stereo_rcnn_amd import _lib, distributed
    header = _header()
    assert 'result visualisation' in header and 'RASTERISATION RULE' in header and 'NOT claimed' in header
    assert '#define SRCNN_OVERLAY_SLOTS_PER_ROW %d\n' % _lib.OVERLAY_SLOTS_PER_ROW in header
    assert '#define SRCNN_OVERLAY_MAX_OFFSET %d\n' % (1 << 20) in header
    for name, value in (('BOXES', _lib.OVERLAY_BOXES), ('WIREFRAMES', _lib.OVERLAY_WIREFRAMES), ('BEV_BOXES', _lib.OVERLAY_BEV_BOXES)):
        assert '#define SRCNN_OVERLAY_%s %d\n' % (name, value) in header
    assert distributed.REC_COLS == _lib.REC_COLS == 32
    assert L.srcnn_version() >= 310
    for name in ('srcnn_render_overlay', 'srcnn_bev_lidar', 'srcnn_overlay_workspace_bytes'):
        m = re.search(r'SRCNN_API (?:int|size_t) %s\((.*?)\);' % name, header, re.S)
        assert m, name
        n_args = len([a for a in m.group(1).split(',') if a.strip()])
        assert n_args == len(_lib._SIGNATURES[name][1]), name
        assert getattr(L, name)
    # 26 slots of 36 bytes per record row, each array rounded up to 256 bytes
    assert L.srcnn_overlay_workspace_bytes(300) >= 300 * 26 * 36
    assert L.srcnn_overlay_workspace_bytes(0) > 0 and L.srcnn_overlay_workspace_bytes(-5) == L.srcnn_overlay_workspace_bytes(0)


def _p2():
    return (ctypes.c_double * 12)(*([721.5, 0, 609.5, 44.8, 0, 721.5, 172.8, 0.2, 0, 0, 1, 0.003]))


def _render(L, **kw):
    """srcnn_render_overlay with good arguments for a 20 x 37 pair (x_max 22, y_max 40), one of them replaced."""
    a = dict(left=P, right=P + 4096, H=20, W=37, rec=P + 8192, max_det=7, rec_cols=32, p2=_p2(), vis_thresh=0.7, plane=None,
             res=70.0 / 40, x_max=22, y_max=40, x_off=-12, y_off=39, layers=7, rpt=0, panel=FAR, ws=FAR * 2, ws_bytes=1 << 20,
             stream=None)
    a.update(kw)
    return L.srcnn_render_overlay(a['left'], a['right'], a['H'], a['W'], a['rec'], a['max_det'], a['rec_cols'], a['p2'], a['vis_thresh'],
                                  a['plane'], a['res'], a['x_max'], a['y_max'], a['x_off'], a['y_off'], a['layers'], a['rpt'],
                                  a['panel'], a['ws'], a['ws_bytes'], a['stream'])


def test_render_overlay_refusals(L):
    _refused(L, _render(L, left=None), b'null image')
    _refused(L, _render(L, right=None), b'null image')
    _refused(L, _render(L, rec=None), b'null record')
    _refused(L, _render(L, p2=None), b'null p2_host')
    _refused(L, _render(L, panel=None), b'null panel')
    _refused(L, _render(L, ws=None), b'null workspace')
    _refused(L, _render(L, H=0), b'H and W')
    _refused(L, _render(L, H=-3), b'H and W')
    _refused(L, _render(L, W=0), b'H and W')
    _refused(L, _render(L, W=40000), b'H and W')
    _refused(L, _render(L, max_det=-1), b'max_det')
    _refused(L, _render(L, max_det=5000), b'max_det')
    _refused(L, _render(L, rec_cols=20), b'SRCNN_REC_COLS')
    _refused(L, _render(L, rec_cols=33), b'SRCNN_REC_COLS')
    _refused(L, _render(L, x_max=-1), b'x_max')
    _refused(L, _render(L, y_max=39), b'y_max must equal 2 H')
    _refused(L, _render(L, res=0.0), b'res')
    _refused(L, _render(L, res=float('nan')), b'res')
    _refused(L, _render(L, x_off=-(1 << 20) - 1), b'x_off and y_off')
    _refused(L, _render(L, y_off=(1 << 20) + 1), b'x_off and y_off')
    _refused(L, _render(L, vis_thresh=float('inf')), b'vis_thresh')
    _refused(L, _render(L, layers=8), b'layers')
    _refused(L, _render(L, rpt=3), b'rows_per_thread')
    panel_bytes = 40 * (37 + 22) * 3
    _refused(L, _render(L, panel=P), b'overlaps an input image')                         # panel == left
    _refused(L, _render(L, right=FAR - 20 * 37 * 3 + 1), b'overlaps an input image')     # right's last byte is the panel's first
    _refused(L, _render(L, left=FAR + panel_bytes - 1), b'overlaps an input image')
    _refused(L, _render(L, rec=FAR + 16), b'overlaps the record')
    _refused(L, _render(L, plane=FAR + 100), b'overlaps the bev plane')
    _refused(L, _render(L, ws=FAR + 64), b'overlaps the workspace')
    _refused(L, _render(L, ws_bytes=64), b'workspace too small', code=-3)
    # x_max == 0: no bird's-eye columns, y_max is not looked at; refused only further on (here: the workspace)
    _refused(L, _render(L, x_max=0, y_max=0, ws_bytes=0), b'workspace too small', code=-3)


def _lidar(L, **kw):
    a = dict(points=P, n=100, m=_p2(), res=70.0 / 40, x_max=22, y_max=40, x_off=-12, y_off=39, plane=FAR, stream=None)
    a.update(kw)
    return L.srcnn_bev_lidar(a['points'], a['n'], a['m'], a['res'], a['x_max'], a['y_max'], a['x_off'], a['y_off'], a['plane'], a['stream'])


def test_bev_lidar_refusals(L):
    _refused(L, _lidar(L, plane=None), b'null plane')
    _refused(L, _lidar(L, m=None), b'null velo_to_cam2_host')
    _refused(L, _lidar(L, n=-1), b'negative n_points')
    _refused(L, _lidar(L, points=None), b'null points')
    _refused(L, _lidar(L, points=P + 4), b'aligned')
    _refused(L, _lidar(L, x_max=0), b'x_max and y_max')
    _refused(L, _lidar(L, y_max=-2), b'x_max and y_max')
    _refused(L, _lidar(L, res=-1.0), b'res')
    _refused(L, _lidar(L, res=float('inf')), b'res')
    _refused(L, _lidar(L, x_off=1 << 21), b'x_off and y_off')
    _refused(L, _lidar(L, y_off=-(1 << 21)), b'x_off and y_off')
    _refused(L, _lidar(L, plane=P + 160), b'overlaps the points')


def test_python_wrappers_refuse_cpu_tensors():
    import numpy as np
    import torch
    from stereo_rcnn_amd import engine, visualize
    img = torch.zeros((20, 37, 3), dtype=torch.uint8)
    rec = torch.zeros((8, 32), dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        engine.render_overlay(img, img, rec, np.eye(3, 4))
    with pytest.raises(NotImplementedError):
        engine.bev_lidar(torch.zeros((5, 4)), np.eye(4), 20)
    with pytest.raises(NotImplementedError):
        visualize.vis_detections(img, 'Car', np.zeros((2, 5), np.float32))

    class Calib(object):
        p2 = np.eye(3, 4)
        r0_rect = np.eye(3)
        tr_velodyne_to_cam0 = np.eye(3, 4)
        t_cam2_cam0 = np.zeros(3)
    with pytest.raises(NotImplementedError):
        visualize.render_result(img, img, rec, Calib())
    with pytest.raises(NotImplementedError):
        visualize.vis_single_box_in_img(img, Calib(), (0, 1, 10), (1.6, 1.5, 4.0), 0.3)


def test_read_lidar_and_velo_to_cam2(tmp_path):
    import numpy as np
    import torch
    from stereo_rcnn_amd import visualize
    from stereo_rcnn_amd.model.utils import kitti_utils
    pts = np.arange(24, dtype=np.float32).reshape(6, 4)
    pts.tofile(str(tmp_path / 'lidar.bin'))
    got = visualize.read_lidar(str(tmp_path / 'lidar.bin'))
    assert got.dtype == torch.float32 and tuple(got.shape) == (6, 4) and (got.numpy() == pts).all()

    class Calib(object):
        r0_rect = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])
        tr_velodyne_to_cam0 = np.array([[1.0, 0, 0, 0.5], [0, 1, 0, -0.25], [0, 0, 1, 2]])
        t_cam2_cam0 = np.array([0.06, 0, 0])
    m = kitti_utils.velo_to_cam2(Calib())
    # (x, y, z) -> velodyne shift -> axes permuted by the rectification -> camera-2 shift
    p = m.dot([1.0, 2.0, 3.0, 1.0])
    assert np.allclose(p, [-(2 - 0.25) + 0.06, -(3 + 2), 1 + 0.5, 1.0], atol=1e-15)
