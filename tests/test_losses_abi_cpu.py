"""CPU: the loss entry points of the C ABI validate their arguments before any launch (include/srcnn_hip.h, "training
losses"), so every refusal is checkable on a host without a GPU -- the pattern of
tests/test_abi.py::test_workspace_query_and_argument_errors_without_gpu.  No call here reaches a launch."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096            # a non-null "device pointer" (never dereferenced: every call below is refused first)
BIG = 1 << 20       # workspace bytes that would do


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


def test_constants_agree_with_the_header(L):
    from stereo_rcnn_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'srcnn_hip.h')).read()
    macro = lambda name: int(re.search(r'#define\s+%s\s+(\d+)' % name, hdr).group(1))
    assert macro('SRCNN_LOSS_ROWS_PER_WG') == _lib.LOSS_ROWS_PER_WG
    assert macro('SRCNN_CE_MAX_COLS') == _lib.CE_MAX_COLS >= 112
    assert (macro('SRCNN_CE_MEAN_KEPT'), macro('SRCNN_CE_WEIGHTED')) == (_lib.CE_MEAN_KEPT, _lib.CE_WEIGHTED)
    assert L.srcnn_version() >= 260


def test_workspace_query(L):
    from stereo_rcnn_amd import _lib
    rpw = _lib.LOSS_ROWS_PER_WG
    w = L.srcnn_loss_workspace_bytes
    assert w(0) > 0 and w(1) == w(rpw)                      # one partial {sum, normaliser sum} per workgroup of rpw rows
    assert w(100 * rpw + 1) >= 101 * 8 > w(100 * rpw) - 256 and w(100 * rpw + 1) >= w(100 * rpw)
    assert w(1 << 31) >= ((1 << 31) // rpw) * 8             # 64-bit row counts
    assert w(-1) == 0


def test_cross_entropy_argument_errors(L):
    ce = lambda logits=P, rows=10, cols=28, stride=28, labels=P, weights=None, mode=0, loss=P, norm=P, ws=P, ws_bytes=BIG: \
        L.srcnn_cross_entropy(logits, rows, cols, stride, labels, weights, mode, loss, norm, ws, ws_bytes, None)
    _refused(L, ce(logits=None), b'null')
    _refused(L, ce(labels=None), b'null')
    _refused(L, ce(loss=None), b'null')
    _refused(L, ce(norm=None), b'null')
    _refused(L, ce(ws=None), b'null')
    _refused(L, ce(rows=-1), b'rows')
    _refused(L, ce(cols=0), b'cols')
    _refused(L, ce(cols=257, stride=257), b'cols')
    _refused(L, ce(cols=28, stride=27), b'stride')
    _refused(L, ce(mode=2), b'mode')
    assert ce(rows=5000, ws_bytes=8) == -3 and b'workspace' in L.srcnn_last_error()
    assert ce(ws_bytes=0) == -3


def test_cross_entropy_backward_argument_errors(L):
    bw = lambda logits=P, rows=10, cols=2, stride=2, labels=P, weights=None, mode=1, norm=P, g=P, grad=P, gstride=2: \
        L.srcnn_cross_entropy_backward(logits, rows, cols, stride, labels, weights, mode, norm, g, grad, gstride, None)
    _refused(L, bw(logits=None), b'null')
    _refused(L, bw(labels=None), b'null')
    _refused(L, bw(norm=None), b'null')
    _refused(L, bw(g=None), b'null')
    _refused(L, bw(grad=None), b'null')
    _refused(L, bw(rows=-3), b'rows')
    _refused(L, bw(cols=0), b'cols')
    _refused(L, bw(cols=300, stride=300, gstride=300), b'cols')
    _refused(L, bw(cols=4, stride=3, gstride=4), b'stride')
    _refused(L, bw(cols=4, stride=4, gstride=3), b'stride')
    _refused(L, bw(mode=-1), b'mode')


def test_smooth_l1_argument_errors(L):
    sl = lambda pred=P, sel=None, n_sel=1, target=P, w_in=None, in_row=0, w_out=None, out_row=0, rows=10, D=6, sigma=3.0, div=12.0, \
        loss=P, norm=P, ws=P, ws_bytes=BIG: \
        L.srcnn_smooth_l1(pred, sel, n_sel, target, w_in, in_row, w_out, out_row, rows, D, sigma, div, loss, norm, ws, ws_bytes, None)
    _refused(L, sl(pred=None), b'null')
    _refused(L, sl(target=None), b'null')
    _refused(L, sl(loss=None), b'null')
    _refused(L, sl(norm=None), b'null')
    _refused(L, sl(ws=None), b'null')
    _refused(L, sl(rows=-1), b'rows')
    _refused(L, sl(D=0), b'D')
    _refused(L, sl(D=65), b'D')
    _refused(L, sl(n_sel=0, sel=P), b'n_sel')
    _refused(L, sl(n_sel=2), b'selector')                  # several slices and nothing to choose with
    _refused(L, sl(sigma=0.0), b'sigma')
    _refused(L, sl(sigma=-1.0), b'sigma')
    _refused(L, sl(div=0.0), b'divisor')
    _refused(L, sl(div=-6.0), b'divisor')
    assert sl(rows=5000, ws_bytes=8) == -3 and b'workspace' in L.srcnn_last_error()


def test_smooth_l1_backward_argument_errors(L):
    bw = lambda pred=P, sel=None, n_sel=1, target=P, w_in=None, in_row=0, w_out=None, out_row=0, rows=10, D=5, sigma=1.0, norm=P, g=P, \
        grad=P: L.srcnn_smooth_l1_backward(pred, sel, n_sel, target, w_in, in_row, w_out, out_row, rows, D, sigma, norm, g, grad, None)
    _refused(L, bw(pred=None), b'null')
    _refused(L, bw(target=None), b'null')
    _refused(L, bw(norm=None), b'null')
    _refused(L, bw(g=None), b'null')
    _refused(L, bw(grad=None), b'null')
    _refused(L, bw(rows=-1), b'rows')
    _refused(L, bw(D=0), b'D')
    _refused(L, bw(D=1000), b'D')
    _refused(L, bw(n_sel=4), b'selector')
    _refused(L, bw(sigma=0.0), b'sigma')


def test_python_entry_points_refuse_cpu_tensors():
    import torch
    from stereo_rcnn_amd.model.stereo_rcnn import losses
    from stereo_rcnn_amd.model.utils.net_utils import _smooth_l1_loss
    x, y = torch.zeros(4, 2), torch.zeros(4, dtype=torch.long)
    with pytest.raises(NotImplementedError):
        losses.cross_entropy_rows(x, y)
    with pytest.raises(NotImplementedError):
        _smooth_l1_loss(torch.zeros(4, 6), torch.zeros(4, 6))
    with pytest.raises(NotImplementedError):
        losses.rpn_losses(torch.zeros(1, 4, 2), torch.zeros(1, 4, 6), y.view(1, 4), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4),
                          torch.zeros(1, 4), torch.zeros(1, 4))
    u = torch.zeros(6, requires_grad=True)
    total = losses.multi_task_loss([torch.tensor(float(i)) for i in range(6)], u)          # plain torch: runs anywhere
    total.backward()
    assert float(total.detach()) == 15.0 and u.grad.tolist() == [1.0 - i for i in range(6)]
