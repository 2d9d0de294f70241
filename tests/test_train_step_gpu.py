"""GPU: stereo_rcnn_amd.training.train_step -- zero-grad, forward_train, multi-task loss, backward and the clipped SGD step as one
call -- on the case of tests/forward_train_ref.py (R-50, one 104 x 328 pair).

The gradients the step must have used come from a separate forward_train + multi_task_loss + backward on an identical model with
the same generator seed (those kernels are run-to-run bit-equal); every trainable parameter and `uncert` after the step must be
BIT-EQUAL to the float32 restatement (tests/optim_ref.py) applied to those gradients with the kernel's own clip coefficient."""
import numpy as np
import pytest
import torch

import forward_train_ref as C
import optim_ref as R

pytestmark = pytest.mark.gpu

GEN_SEED = 11
CLIP = 10.0


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.fixture(scope='module')
def case(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import training
    from stereo_rcnn_amd.model.stereo_rcnn import losses
    mp = pytest.MonkeyPatch()
    C.patch_cfg(mp)
    try:
        batch = [t.to(dev) if i != 2 else t for i, t in enumerate(C.inputs())]          # im_info stays on the host
        # the gradients, from a model of its own
        other = C.make_model(dev)
        uncert_o = torch.full((6,), -1.0, device=dev, requires_grad=True)
        out = training.forward_train(other, *batch, generator=torch.Generator(device=dev).manual_seed(GEN_SEED))
        total_o = losses.multi_task_loss(out[8:14], uncert_o)
        total_o.backward()
        grads = {k: _np(p.grad) for k, p in other.named_parameters() if p.grad is not None}
        grads['uncert'] = _np(uncert_o.grad)
        # the step
        model = C.make_model(dev)
        uncert = torch.full((6,), -1.0, device=dev, requires_grad=True)
        opt = training.make_optimizer(model, uncert)
        before = {k: _np(p).copy() for k, p in model.named_parameters()}
        res = training.train_step(model, opt, uncert, batch, clip_norm=CLIP, generator=torch.Generator(device=dev).manual_seed(GEN_SEED))
        after = {k: _np(p).copy() for k, p in model.named_parameters()}
        norm, coef = (np.float32(v) for v in _np(opt.last_norm))
        buffers = {k: opt.state[p]['momentum_buffer'] for k, p in training.trainable_parameters(model).items()}
        ptrs = {k: b.data_ptr() for k, b in buffers.items()}
        first_m = {k: _np(b).copy() for k, b in buffers.items()}
        uncert1 = _np(uncert).copy()
        res2 = training.train_step(model, opt, uncert, batch, clip_norm=CLIP, generator=torch.Generator(device=dev).manual_seed(GEN_SEED + 1))
        after2 = {k: _np(p).copy() for k, p in model.named_parameters()}
        ptrs2 = {k: opt.state[p]['momentum_buffer'].data_ptr() for k, p in training.trainable_parameters(model).items()}
        second_m = {k: _np(opt.state[p]['momentum_buffer']).copy() for k, p in training.trainable_parameters(model).items()}
        trainable = list(training.trainable_parameters(model))
        groups = [(g['lr'], g['weight_decay'], g['momentum']) for g in opt.param_groups]
    finally:
        mp.undo()
    return dict(grads=grads, before=before, after=after, after2=after2, norm=norm, coef=coef, res=res, res2=res2, ptrs=ptrs, ptrs2=ptrs2,
                first_m=first_m, second_m=second_m, uncert1=uncert1, trainable=trainable, groups=groups, total_o=float(total_o.detach()),
                losses_o=[float(l.detach()) for l in out[8:14]])


def test_groups_follow_the_reference_recipe(case):
    assert len(case['groups']) == len(case['trainable']) + 1
    for key, (lr, wd, momentum) in zip(case['trainable'], case['groups']):
        assert (lr, wd, momentum) == ((0.001, 0, 0.9) if 'bias' in key else (0.001, 0.0001, 0.9)), key
    assert case['groups'][-1] == (0.001, 0, 0.9)                                        # uncert: lr, no weight decay


def test_returned_scalars(case):
    from stereo_rcnn_amd import training
    res = case['res']
    assert set(res) == {'loss', 'grad_norm'} | set(training.LOSS_NAMES)
    assert all(t.is_cuda and t.dim() == 0 for t in res.values())
    assert float(res['loss']) == case['total_o']
    assert [float(res[k]) for k in training.LOSS_NAMES] == case['losses_o']
    assert float(res['grad_norm']) == float(case['norm'])


def test_norm_within_the_derived_bound(case):
    want = R.norm_f64([case['grads'][k] for k in case['trainable']])
    rel = abs(float(case['norm']) - want) / want
    print('train_step gradient norm %.9g (float64 %.9g): relative error %.3e, bound %.3e; coefficient %.9g'
          % (case['norm'], want, rel, R.norm_bound(), case['coef']))
    assert set(case['grads']) == set(case['trainable']) | {'uncert'}
    assert rel <= R.norm_bound()
    assert case['coef'] == np.float32(CLIP) / max(case['norm'], np.float32(CLIP))


def test_trainable_parameters_bit_equal_to_the_restatement(case):
    changed = 0
    for key, (lr, wd, momentum) in zip(case['trainable'], case['groups']):
        p, m = R.sgd_step_f32(case['before'][key], case['grads'][key], None, lr, wd, momentum, True, case['coef'])
        assert _same_bits(case['after'][key], p), key
        assert _same_bits(case['first_m'][key], m), key
        changed += int(not _same_bits(case['after'][key], case['before'][key]))
    assert changed >= 1
    lr, wd, momentum = case['groups'][-1]
    u, _ = R.sgd_step_f32(np.full(6, -1.0, np.float32), case['grads']['uncert'], None, lr, wd, momentum, True, None)     # not clipped
    assert _same_bits(case['uncert1'], u)
    assert not _same_bits(case['uncert1'], np.full(6, -1.0, np.float32))


def test_frozen_parameters_unchanged(case):
    frozen = [k for k in case['before'] if k not in case['trainable']]
    assert len(frozen) > 50
    for key in frozen:
        assert _same_bits(case['after'][key], case['before'][key]), key
        assert _same_bits(case['after2'][key], case['before'][key]), key


def test_second_step_reuses_the_buffers(case):
    assert case['ptrs'] == case['ptrs2']
    moved = sum(int(not _same_bits(case['after2'][k], case['after'][k])) for k in case['trainable'])
    assert moved >= 1
    assert sum(int(not _same_bits(case['second_m'][k], case['first_m'][k])) for k in case['trainable']) >= 1
    assert np.isfinite(float(case['res2']['loss']))
