"""CPU: tests/loader_ref.py (the numpy restatement of the ground-truth batch and of the flipped image preparation) against the
reference's own roibatchLoader.__getitem__ and minibatch._get_image_blob (tests/golden/reference_loader.npz), bit for bit; and the
host side of the product's table packing."""
import numpy as np
import pytest

import loader_ref


@pytest.fixture(scope='module')
def g():
    return loader_ref.golden()


def test_gt_batch_restatement_equals_the_reference(g):
    seen = set()
    for ci in range(int(g['hand_cases'])):
        e, (n, H, W, target), perm, im_info, expect, num = loader_ref.golden_hand_case(g, ci)
        scale = float(target) / float(min(H, W))
        assert np.float32(scale) == im_info[2]
        got, got_num = loader_ref.gt_padded(e, scale, int(im_info[1]), perm)
        assert got_num == num == min(n, loader_ref.K_DEFAULT)
        for a, b in zip(got, expect):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), ci
        # the keys that stand for the recorded permutation rank back to it
        assert np.array_equal(loader_ref.perm_from_keys(loader_ref.keys_from_perm(perm)), perm)
        seen.add(n)
    assert seen == {1, 2, 30, 31, 40}


def test_truncation_follows_the_shuffle(g):
    e, (n, H, W, target), perm, im_info, expect, num = loader_ref.golden_hand_case(g, 3)
    assert n == 31 and num == 30
    scale = float(target) / float(min(H, W))
    wrong, _ = loader_ref.gt_padded(e, scale, int(im_info[1]), np.arange(n))        # truncating first keeps rows 0..29
    assert perm[30] != 30 and not np.array_equal(np.sort(wrong[0][:30], 0), np.sort(expect[0][:30], 0))


def test_image_restatement_equals_the_reference(g):
    flips, cropped = set(), False
    for ci in range(int(g['img_cases'])):
        pre = 'img_%d_' % ci
        H, W, target, max_size, flipped = (int(v) for v in g[pre + 'meta'])
        bl, br, scale = loader_ref.image_blobs(g[pre + 'left'], g[pre + 'right'], bool(flipped), target, max_size)
        ref_l, ref_r = g[pre + 'blob_left'][0].transpose(2, 0, 1), g[pre + 'blob_right'][0].transpose(2, 0, 1)
        assert bl.shape == ref_l.shape and np.ascontiguousarray(ref_l).tobytes() == np.ascontiguousarray(bl).tobytes(), ci
        assert np.ascontiguousarray(ref_r).tobytes() == np.ascontiguousarray(br).tobytes(), ci
        flips.add(bool(flipped))
        cropped = cropped or bl.shape[2] == max_size
    assert flips == {False, True} and cropped


def test_pack_gt_table(g):
    import math
    from stereo_rcnn_amd import _lib
    from stereo_rcnn_amd.data import pack_gt_table
    entries = [loader_ref.golden_hand_case(g, ci)[0] for ci in range(int(g['hand_cases']))]
    entries[1] = dict(entries[1], gt_classes=np.asarray([1, 0], dtype=np.int32))        # a class-0 row is left out (minibatch.py:43)
    table, off = pack_gt_table(entries)
    assert table.dtype == np.float32 and table.shape == (1 + 1 + 30 + 31 + 40, _lib.GT_COLS)
    assert off.tolist() == [0, 1, 2, 32, 63, 103]
    e = entries[2]
    rows = table[off[2]:off[3]]
    assert np.array_equal(rows[:, 0:4], e['boxes_left']) and np.array_equal(rows[:, 8:12], e['boxes_merge'])
    assert np.array_equal(rows[:, 17:23], e['kpts']) and (rows[:, 23] == 1).all()
    for i in range(30):
        assert rows[i, 15] == np.float32(math.sin(e['dim_orien'][i, 3])) and rows[i, 16] == np.float32(math.cos(e['dim_orien'][i, 3]))
    # what the kernel reads is what the reference computes: sin / cos of the rows equal get_minibatch's
    ref = loader_ref.gt_rows(e, 1.6, 211)[3]
    assert np.array_equal(rows[:, 12:17], ref)
