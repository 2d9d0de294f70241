"""CPU: trainval_net's --accum and --guard (training.train_step's accum_steps and guard): defaults, parsing, and the grouping of
loader batches into steps."""
import pytest

from stereo_rcnn_amd import trainval_net

BASE = ['--kitti-path', 'k', '--split', 's']


def test_defaults():
    a = trainval_net.parse_args(BASE)
    assert a.accum == 1 and a.guard is False


def test_flags_parse():
    a = trainval_net.parse_args(BASE + ['--accum', '4'])
    assert a.accum == 4 and a.guard is False
    a = trainval_net.parse_args(BASE + ['--guard'])
    assert a.accum == 1 and a.guard is True
    a = trainval_net.parse_args(BASE + ['--guard', '--accum', '2', '--device-fold'])
    assert a.accum == 2 and a.guard is True and a.prepared_weights is True


@pytest.mark.parametrize('value', ['0', '-3', 'two'])
def test_a_bad_accum_is_refused(value):
    with pytest.raises(SystemExit):
        trainval_net.parse_args(BASE + ['--accum', value])


def test_groups_drop_the_trailing_short_one():
    g = trainval_net._groups
    assert list(g(range(7), 1)) == [[i] for i in range(7)]
    assert list(g(range(7), 2)) == [[0, 1], [2, 3], [4, 5]]
    assert list(g(range(7), 3)) == [[0, 1, 2], [3, 4, 5]]
    assert list(g(range(2), 3)) == []
    it = iter(range(10))
    first = next(g(it, 4))
    assert first == [0, 1, 2, 3] and next(it) == 4              # lazy: a group takes exactly its batches from the loader


def test_both_flags_are_documented():
    assert '--accum N' in trainval_net.__doc__ and '--guard' in trainval_net.__doc__
