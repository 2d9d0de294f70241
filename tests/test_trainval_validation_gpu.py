"""GPU: per-epoch validation inside the training driver (trainval_net --val-split) on synthetic pairs (tests/loader_ref.py's frames:
two training ids, two validation ids, R-50, in-process decode).  Two epochs, so that the second validation goes through
Plan.refresh on the plan the first one built: each writes ap_epoch<E>.json with the keys run_kitti's ap.json has and logs the Car
Moderate line, and the checkpoints equal, tensor for tensor, those of the same run without --val-split."""
import json
import os

import numpy as np
import pytest
import torch

import forward_train_ref as C
import loader_ref

pytestmark = pytest.mark.gpu
CALIB, FRAMES = loader_ref.SMALL_CALIB, loader_ref.SMALL_FRAMES


def _same(a, b, where):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a.cpu(), b.cpu()), where
    elif isinstance(a, dict):
        assert set(a) == set(b), where
        for k in a:
            _same(a[k], b[k], '%s.%s' % (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (where, i))
    else:
        assert a == b, where


def test_validation_writes_ap_and_leaves_training_bit_identical(tmp_path, dev, monkeypatch):
    from stereo_rcnn_amd import kitti_eval, trainval_net
    from stereo_rcnn_amd.model.utils.config import cfg
    C.patch_cfg(monkeypatch)
    monkeypatch.setattr(cfg.TRAIN, 'SCALES', (104,))
    monkeypatch.setattr(cfg.TEST, 'SCALES', (104,))
    root = str(tmp_path / 'kitti')
    rng = np.random.RandomState(5)
    images = {fid: (rng.randint(0, 256, (H, W, 3)).astype(np.uint8), rng.randint(0, 256, (H, W, 3)).astype(np.uint8))
              for fid, (H, W), _ in FRAMES}
    loader_ref.write_dataset(root, [(fid, hw, CALIB, '\n'.join(lines) + '\n') for fid, hw, lines in FRAMES], images)
    train, val = str(tmp_path / 'train2.txt'), str(tmp_path / 'val2.txt')
    open(train, 'w').write('\n'.join(f[0] for f in FRAMES[:2]))
    open(val, 'w').write('\n'.join(f[0] for f in FRAMES[2:]))
    labels = os.path.join(root, 'training', 'label_2')

    def run(save, extra):
        torch.manual_seed(1234)             # the same run: the driver's random initialisation draws from the global generator
        return trainval_net.main(['--kitti-path', root, '--split', train, '--save_dir', save, '--net', '50', '--nw', '0', '--no_flip',
                                  '--disp_interval', '1', '--epochs', '2'] + extra)
    plain, withval = str(tmp_path / 'plain'), str(tmp_path / 'withval')
    a = run(plain, [])
    b = run(withval, ['--val-split', val, '--val-label-dir', labels, '--val-precision', 'f32'])
    assert [os.path.basename(p) for p in a] == [os.path.basename(p) for p in b] and len(a) == 2
    for pa, pb in zip(a, b):
        _same(torch.load(pa, map_location='cpu'), torch.load(pb, map_location='cpu'), os.path.basename(pa))
    assert not os.path.exists(os.path.join(plain, 'ap_epoch1.json'))
    # what run_kitti writes for the same result files
    for epoch in (1, 2):
        got = json.load(open(os.path.join(withval, 'ap_epoch%d.json' % epoch)))
        want = kitti_eval.evaluate_split(labels, os.path.join(withval, 'val_epoch%d' % epoch), [f[0] for f in FRAMES[2:]], dev, log=lambda s: None)
        assert set(got) == set(want) and 'Car' in got
        assert got == json.loads(json.dumps(want))
    log = open(os.path.join(withval, 'trainlog.txt')).read()
    assert log.count('Car Moderate AP@') == 2 and 'AP_2d' in log and 'AP_bev' in log and 'AP_3d' in log
    assert 'inference weights refreshed in place' in log                 # the second validation refreshed the first one's plan
    assert 'Car Moderate' not in open(os.path.join(plain, 'trainlog.txt')).read()
