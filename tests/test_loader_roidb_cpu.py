"""CPU: stereo_rcnn_amd.datasets.kitti (annotations -> roidb, flipped copies, filter, ratio ranking) against the arrays the
reference's own datasets.kitti / datasets.imdb / roi_data_layer.roidb produced from the same label and calibration texts
(tests/golden/reference_loader.npz, written by tests/golden/make_loader_golden.py) -- equal in dtype and bits; and the batch
sampler against trainval_net.py:81-101's formula."""
import numpy as np
import pytest
import torch

import loader_ref


@pytest.fixture(scope='module')
def g():
    return loader_ref.golden()


@pytest.fixture(scope='module')
def product(g, tmp_path_factory):
    from stereo_rcnn_amd.datasets import kitti
    root = tmp_path_factory.mktemp('kitti')
    frames = [(str(i), tuple(int(v) for v in s), str(c), str(l))
              for i, s, c, l in zip(g['ann_ids'], g['ann_shapes'], g['ann_calibs'], g['ann_labels'])]
    split = loader_ref.write_dataset(str(root), frames)
    return kitti.build_roidb(str(root), split, use_flipped=True), frames


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), what


def test_roidb_equals_the_reference(g, product):
    (roidb, ratio_list, ratio_index), frames = product
    assert len(roidb) == int(g['roidb_len']) == 2 * (len(frames) - 1)          # one frame loses every object: dropped, flipped copy too
    import os
    assert [os.path.basename(e['img_left'])[:-4] for e in roidb] == [str(v) for v in g['roidb_ids']]
    n_flipped = 0
    for i, e in enumerate(roidb):
        ref = loader_ref.golden_roidb_entry(g, i)
        names = ['boxes_left', 'boxes_right', 'boxes_merge', 'dim_orien', 'kpts', 'gt_classes']
        if not ref['flipped']:
            names += ['kpts_right', 'truncation', 'occlusion']
        for k in names:
            _same(e[k], ref[k], 'entry %d %s' % (i, k))
        assert e['flipped'] is ref['flipped']
        assert (e['width'], e['height'], e['need_crop']) == (ref['width'], ref['height'], ref['need_crop'])
        n_flipped += int(e['flipped'])
    assert n_flipped == len(roidb) // 2
    _same(np.asarray(ratio_list), g['ratio_list'], 'ratio_list')
    assert np.array_equal(np.asarray(ratio_index), g['ratio_index'])


def test_the_fixture_covers_the_cases(g, product):
    """What the issue asks the frames to contain, seen from the product's side."""
    from stereo_rcnn_amd.datasets import kitti
    from stereo_rcnn_amd.model.utils import kitti_utils
    (roidb, _, _), frames = product
    labelled = sum(sum(1 for ln in f[3].split('\n') if ln.split() and ln.split()[0] in kitti_utils.USED_CLASSES) for f in frames)
    kept = sum(len(e['boxes_left']) for e in roidb if not e['flipped'])
    assert kept < labelled                                  # the filter and the occlusion pass removed objects
    alphas = np.concatenate([e['dim_orien'][:, 3] for e in roidb if not e['flipped']])
    assert (alphas > np.pi).any() and (alphas < -np.pi).any() and (alphas > 0).any() and (alphas < 0).any()
    flipped = np.concatenate([e['dim_orien'][:, 3] for e in roidb if e['flipped']])
    assert (np.abs(flipped) <= np.float32(np.pi) + 1e-6).all()
    boxes = np.concatenate([e['boxes_left'] for e in roidb if not e['flipped']])
    assert (boxes[:, 0] == 0).any() and (boxes[:, 1] == 0).any()
    assert any((e['boxes_left'][:, 2] == e['width'] - 1).any() for e in roidb if not e['flipped'])
    assert any((e['boxes_left'][:, 3] == e['height'] - 1).any() for e in roidb if not e['flipped'])
    assert kitti.filter_roidb([{'boxes_left': [], 'boxes_right': [], 'boxes_merge': []}]) == []


def test_rank_roidb_ratio(g):
    from stereo_rcnn_amd.datasets import kitti
    rd = [{'width': int(w), 'height': int(h)} for w, h in g['rank_wh']]
    ratio_list, ratio_index = kitti.rank_roidb_ratio(rd)
    _same(ratio_list, g['rank_ratio_list'], 'ratio_list')
    assert np.array_equal(ratio_index, g['rank_ratio_index'])
    assert [e['need_crop'] for e in rd] == g['rank_need_crop'].tolist()


@pytest.mark.parametrize('train_size,bs', [(7, 1), (7, 2), (8, 4), (3, 4)])
def test_sampler_follows_trainval_net(train_size, bs):
    from stereo_rcnn_amd.data import BatchSampler
    got = list(BatchSampler(train_size, bs, torch.Generator().manual_seed(9)))
    gen = torch.Generator().manual_seed(9)
    per = int(train_size / bs)                                              # trainval_net.py:84-101
    rand_num = torch.randperm(per, generator=gen).view(-1, 1) * bs
    want = (rand_num.expand(per, bs) + torch.arange(0, bs).view(1, bs).long()).reshape(-1)
    if train_size % bs:
        want = torch.cat((want, torch.arange(per * bs, train_size).long()), 0)
    assert got == want.tolist()
    assert sorted(got) == list(range(train_size))
