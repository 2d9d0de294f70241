"""GPU: stereo_rcnn_amd.data.TrainLoader end to end on a synthetic KITTI-style dataset written into a temporary directory (PNG
pairs of 52 x 164 and 50 x 160, label and calibration text in the style of tests/golden/make_loader_golden.py's frames, scaled to
that image size), cfg.TRAIN.SCALES = (104,): every batch against tests/loader_ref.py bit for bit, the same batches whatever the
number of decode workers, and train_step straight from the loader."""
import numpy as np
import pytest
import torch

import forward_train_ref as C
import loader_ref

pytestmark = pytest.mark.gpu

CALIB, FRAMES = loader_ref.SMALL_CALIB, loader_ref.SMALL_FRAMES


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    from stereo_rcnn_amd.datasets import kitti
    root = str(tmp_path_factory.mktemp('kitti'))
    rng = np.random.RandomState(17)
    images = {fid: (rng.randint(0, 256, (H, W, 3)).astype(np.uint8), rng.randint(0, 256, (H, W, 3)).astype(np.uint8))
              for fid, (H, W), _ in FRAMES}
    split = loader_ref.write_dataset(root, [(fid, hw, CALIB, '\n'.join(lines) + '\n') for fid, hw, lines in FRAMES], images)
    roidb, ratio_list, ratio_index = kitti.build_roidb(root, split)
    assert len(roidb) == 8 and all(len(e['boxes_left']) >= 2 for e in roidb)
    import os
    by_path = {os.path.join(root, 'training', 'image_2', fid + '.png'): images[fid] for fid in images}
    return roidb, ratio_index, by_path


def _epoch(dataset, dev, workers, B, seed=4, record=None):
    from stereo_rcnn_amd import data
    roidb, ratio_index, _ = dataset
    loader = data.TrainLoader(roidb, ratio_index, B, dev, generator=torch.Generator().manual_seed(seed), workers=workers, prefetch=2)
    try:
        batches = [[t.cpu().numpy() for t in batch] for batch in loader]
        assert all(b[2].dtype == np.float32 and b[8].dtype == np.int64 for b in batches)
        return batches, list(loader.visited)
    finally:
        loader.close()


def _replay_draws(roidb, ratio_index, B, seed):
    """The loader's draws, drawn again here: the sampler's order, then per visited sample the scale index and the keys."""
    from stereo_rcnn_amd import data
    gen = torch.Generator().manual_seed(seed)
    order = data.BatchSampler(len(roidb), B, gen).order().tolist()
    keys = []
    for p in order:
        n = len(roidb[int(ratio_index[p])]['boxes_left'])
        assert int(torch.randint(0, 1, (1,), generator=gen)) == 0
        keys.append(torch.randint(0, 2 ** 32, (n,), dtype=torch.int64, generator=gen).numpy().astype(np.uint32))
    return order, keys


@pytest.mark.parametrize('B', [1, 2])
def test_epoch_equals_the_restatement_for_any_worker_count(dataset, dev, monkeypatch, B):
    from stereo_rcnn_amd.model.utils.config import cfg
    monkeypatch.setattr(cfg.TRAIN, 'SCALES', (104,))
    roidb, ratio_index, by_path = dataset
    b0, v0 = _epoch(dataset, dev, 0, B)
    b2, v2 = _epoch(dataset, dev, 2, B)
    assert v0 == v2 and sorted(i for ids in v0 for i in ids) == list(range(len(roidb)))       # every index once
    assert len(b0) == len(b2) == len(roidb) // B
    for x, y in zip(b0, b2):
        for a, b in zip(x, y):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    order, keys = _replay_draws(roidb, ratio_index, B, 4)
    assert [int(ratio_index[p]) for p in order] == [i for ids in v0 for i in ids]
    padded = False
    for j, (batch, ids) in enumerate(zip(b0, v0)):
        entries = [roidb[i] for i in ids]
        want = loader_ref.batch(entries, [by_path[e['img_left']] for e in entries], [104] * len(ids), keys[j * B:j * B + len(ids)])
        for a, w in zip(batch, want):
            assert a.dtype == w.dtype and a.shape == w.shape and a.tobytes() == np.ascontiguousarray(w).tobytes(), j
        padded = padded or len({tuple(r[:2]) for r in batch[2].tolist()}) > 1
        assert batch[0].shape[2:] == (104, max(int(r[1]) for r in batch[2]))
    assert padded == (B == 2)                   # the two image sizes meet in a batch: zero padding, own im_info rows


def test_draws_argument_replays_recorded_draws(dataset, dev, monkeypatch):
    from stereo_rcnn_amd import data
    from stereo_rcnn_amd.model.utils.config import cfg
    monkeypatch.setattr(cfg.TRAIN, 'SCALES', (104,))
    roidb, ratio_index, _ = dataset
    order, keys = _replay_draws(roidb, ratio_index, 1, 4)
    draws = {'order': torch.tensor(order), 'scale_inds': torch.zeros(len(order), dtype=torch.int64),
             'keys': [torch.from_numpy(k.astype(np.int64)) for k in keys]}
    loader = data.TrainLoader(roidb, ratio_index, 1, dev, workers=0, draws=draws)
    got = [[t.cpu().numpy() for t in batch] for batch in loader]
    want, _ = _epoch(dataset, dev, 0, 1)
    for x, y in zip(got, want):
        for a, b in zip(x, y):
            assert a.tobytes() == b.tobytes()


def test_train_steps_straight_from_the_loader(dataset, dev, monkeypatch):
    from stereo_rcnn_amd import data, training
    from stereo_rcnn_amd.model.utils.config import cfg
    C.patch_cfg(monkeypatch)
    monkeypatch.setattr(cfg.TRAIN, 'SCALES', (104,))
    roidb, ratio_index, by_path = dataset
    order, keys = _replay_draws(roidb, ratio_index, 1, 4)

    def run(batches):
        model = C.make_model(dev)
        uncert = torch.full((6,), -1.0, device=dev, requires_grad=True)
        opt = training.make_optimizer(model, uncert)
        gen = torch.Generator(device=dev).manual_seed(21)
        before = model.RCNN_toplayer.weight.detach().clone()
        res = [training.train_step(model, opt, uncert, b, clip_norm=10., generator=gen) for b in batches]
        torch.cuda.synchronize()
        return model, before, [{k: v.cpu().numpy() for k, v in r.items()} for r in res]

    loader = data.TrainLoader(roidb, ratio_index, 1, dev, generator=torch.Generator().manual_seed(4), workers=0)
    it = iter(loader)
    model, before, res = run([next(it), next(it)])
    loader.close()
    for r in res:
        assert all(np.isfinite(v).all() for v in r.values())
    assert not torch.equal(model.RCNN_toplayer.weight.detach(), before)            # a parameter moved
    # step 1 on the same batch assembled by the restatement: bit-equal
    e = roidb[int(ratio_index[order[0]])]
    want = loader_ref.batch([e], [by_path[e['img_left']]], [104], keys[:1])
    ref_batch = [torch.from_numpy(np.ascontiguousarray(t)) for t in want]
    ref_batch = [t if i == 2 else t.to(dev) for i, t in enumerate(ref_batch)]
    _, _, ref = run([ref_batch])
    for k in res[0]:
        assert res[0][k].tobytes() == ref[0][k].tobytes(), k
