"""CPU: autograd.choose_engine, the rule behind forward_precision / backward_precision 'auto', held to the measured table it was
fitted to (stereo_rcnn_amd/train_engine_table.py, generated from profiles/train_engine_table.txt): every row whose f16x3 / fp32
ratio lies below 0.97 resolves to f16x3 and every row above 1.03 to fp32 -- the +-3 % band is the box-to-box spread of one binary,
rows inside it may fall either way.  Also the rule's purity and the command line."""
import itertools

import pytest

from stereo_rcnn_amd import autograd, train_engine_table, trainval_net


@pytest.mark.parametrize('row', train_engine_table.ROWS, ids=lambda r: '%s-%d-%d-%d' % r[:4])
def test_rule_agrees_with_every_measured_row_outside_the_band(row):
    direction, M, N, K, ratio = row
    got = autograd.choose_engine(direction, M, N, K)
    print('%s M %d N %d K %d: measured f16x3 / fp32 %.3f -> %s' % (direction, M, N, K, ratio, got))
    if ratio < 0.97:
        assert got == 'f16x3'
    if ratio > 1.03:
        assert got == 'f32'


def test_table_covers_both_directions_and_both_outcomes():
    for direction in ('forward', 'backward'):
        ratios = [r[4] for r in train_engine_table.ROWS if r[0] == direction]
        assert len(ratios) >= 10 and min(ratios) < 0.97 and max(ratios) > 1.03


def test_rule_is_a_pure_function_of_its_arguments():
    sizes = (1, 2, 31, 256, 300, 4096, 74400, 297600, 1 << 22)
    for direction, M, N, K in itertools.product(('forward', 'backward'), sizes, (24, 64, 2048), (32, 576, 12544)):
        first = autograd.choose_engine(direction, M, N, K)
        assert first in ('f32', 'f16x3') and autograd.choose_engine(direction, M, N, K) == first
    for direction in ('forward', 'backward'):
        assert autograd.choose_engine(direction, 1, 2048, 12544) == 'f32'            # a degenerate M
    with pytest.raises(ValueError):
        autograd.choose_engine('sideways', 64, 64, 64)


def test_precision_accepts_auto_and_nothing_else_new():
    p = autograd.Precision('auto', 'auto')
    assert p.without_graph().forward == 'f32'
    r = p.resolved(297600, 64, 576)
    assert r.forward == autograd.choose_engine('forward', 297600, 64, 576) and r.backward == autograd.choose_engine('backward', 297600, 64, 576)
    assert autograd.Precision('f16x3', 'f32').resolved(1, 1, 32) == autograd.Precision('f16x3', 'f32')       # explicit engines stay
    assert autograd.Precision('auto', 'f16x3').resolved(1, 1, 32) == autograd.Precision('f32', 'f16x3')
    with pytest.raises(ValueError):
        autograd.Precision('fast')
    with pytest.raises(ValueError):
        autograd.Precision('f32', 'fast')


def test_command_line():
    base = ['--kitti-path', 'k', '--split', 's']
    a = trainval_net.parse_args(base)
    assert (a.forward_precision, a.backward_precision, a.prepared_weights, a.reuse_maxima) == ('f32', 'f32', False, True)
    a = trainval_net.parse_args(base + ['--forward-precision', 'auto', '--backward-precision', 'auto', '--prepared-weights'])
    assert (a.forward_precision, a.backward_precision, a.prepared_weights) == ('auto', 'auto', True)
    with pytest.raises(SystemExit):
        trainval_net.parse_args(base + ['--forward-precision', 'fast'])
