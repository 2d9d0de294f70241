"""GPU: the training driver stereo_rcnn_amd.trainval_net in-process on three synthetic pairs (tests/test_loader_gpu.py's frames):
one epoch writes a checkpoint that loads back into a fresh model and optimiser bit for bit, and --resume continues from it."""
import os

import numpy as np
import pytest
import torch

import forward_train_ref as C
import loader_ref

pytestmark = pytest.mark.gpu
CALIB, FRAMES = loader_ref.SMALL_CALIB, loader_ref.SMALL_FRAMES


def test_one_epoch_checkpoint_and_resume(tmp_path, dev, monkeypatch, capsys):
    from stereo_rcnn_amd import training, trainval_net
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    from stereo_rcnn_amd.model.utils.config import cfg
    C.patch_cfg(monkeypatch)
    monkeypatch.setattr(cfg.TRAIN, 'SCALES', (104,))
    root, save = str(tmp_path / 'kitti'), str(tmp_path / 'models')
    rng = np.random.RandomState(5)
    frames = FRAMES[:3]
    images = {fid: (rng.randint(0, 256, (H, W, 3)).astype(np.uint8), rng.randint(0, 256, (H, W, 3)).astype(np.uint8))
              for fid, (H, W), _ in frames}
    split = loader_ref.write_dataset(root, [(fid, hw, CALIB, '\n'.join(lines) + '\n') for fid, hw, lines in frames], images)
    common = ['--kitti-path', root, '--split', split, '--save_dir', save, '--net', '50', '--nw', '2', '--no_flip', '--disp_interval', '2']
    written = trainval_net.main(common + ['--epochs', '1'])
    assert written == [os.path.join(save, 'stereo_rcnn_1_2.pth')] and os.path.exists(written[0])
    log = open(os.path.join(save, 'trainlog.txt')).read()
    assert '3 roidb entries' in log and '[epoch  1][iter    0/   3]' in log and '[epoch  1][iter    2/   3]' in log and 'iter    1/' not in log

    ckpt = torch.load(written[0], map_location=dev)
    assert ckpt['epoch'] == 2 and tuple(ckpt['uncert'].shape) == (6,) and not torch.equal(ckpt['uncert'].cpu(), torch.full((6,), -1.0))
    fresh = resnet(C.CLASSES, 50)
    fresh.create_architecture()
    fresh.load_state_dict(ckpt['model'])
    fresh.to(dev)
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, ckpt['model'][k].to(dev)), k
    uncert = torch.full((6,), -1.0, device=dev, requires_grad=True)
    opt = training.make_optimizer(fresh, uncert)
    opt.load_state_dict(ckpt['optimizer'])
    loaded, saved = opt.state_dict(), ckpt['optimizer']
    assert len(loaded['state']) == len(saved['state']) > 0 and loaded['param_groups'] == saved['param_groups']
    for i, st in saved['state'].items():
        assert torch.equal(loaded['state'][i]['momentum_buffer'], st['momentum_buffer'].to(dev)), i

    capsys.readouterr()
    again = trainval_net.main(common + ['--epochs', '2', '--resume', written[0]])
    assert again == [os.path.join(save, 'stereo_rcnn_2_2.pth')]
    out = capsys.readouterr().out
    assert 'loading checkpoint' in out and '[epoch  2]' in out and '[epoch  1]' not in out
    ckpt2 = torch.load(again[0], map_location='cpu')
    assert ckpt2['epoch'] == 3
    moved = [k for k, v in ckpt2['model'].items() if not torch.equal(v, ckpt['model'][k].cpu())]
    assert 'RCNN_toplayer.weight' in moved
    assert all(torch.isfinite(v).all() for v in ckpt2['model'].values() if v.is_floating_point())
