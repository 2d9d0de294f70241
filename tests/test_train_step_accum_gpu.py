"""GPU: training.train_step's accum_steps and guard on the case of tests/forward_train_ref.py (its model, its TRAIN_SIZES; two
batches: inputs(5) and inputs(6)).  Every comparison is between two runs of the same kernels from the same seeds (they are
run-to-run bit-equal), so every assertion is equality of BITS:
  * accum_steps=1, guard=False given as keywords is the positional call of before;
  * accum_steps=2 is zero-grad, forward / backward of a, forward / backward of b with the generator going on, then
    optimizer.step(clip_norm, clip_params, grad_scale=0.5); the returned loss is (la + lb) * 0.5;
  * guard=True with finite gradients changes nothing;
  * guard=True with a gradient that is not finite (one log-variance of the multi-task loss set so low that exp(-u) overflows:
    the total and every gradient behind that term become Inf or NaN, while every index any kernel computes stays what it was)
    changes no parameter and no momentum buffer, says ok == 0 and counts one skipped step; the next good step moves on."""
import copy

import numpy as np
import pytest
import torch

import forward_train_ref as C

pytestmark = pytest.mark.gpu

GEN_SEED = 11
CLIP = 10.0
PLANTED = 2             # uncert[2] = -100: exp(100) is Inf in float32


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _params(model, uncert):
    out = {k: _bits(p) for k, p in model.named_parameters()}
    out['uncert'] = _bits(uncert)
    return out


def _buffers(model, opt, uncert):
    from stereo_rcnn_amd import training
    named = dict(training.trainable_parameters(model), uncert=uncert)
    return {k: _bits(opt.state[p]['momentum_buffer']) for k, p in named.items()}


def _differing(a, b):
    assert set(a) == set(b)
    return sorted(k for k in a if not np.array_equal(a[k], b[k]))


@pytest.fixture(scope='module')
def case(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import training
    from stereo_rcnn_amd.model.stereo_rcnn import losses
    mp = pytest.MonkeyPatch()
    C.patch_cfg(mp)
    try:
        a, b = ([t.to(dev) if i != 2 else t for i, t in enumerate(C.inputs(seed))] for seed in (5, 6))      # im_info stays on the host
        first = C.make_model(dev)

        def fresh():
            model = copy.deepcopy(first)
            uncert = torch.full((6,), -1.0, device=dev, requires_grad=True)
            return model, uncert, training.make_optimizer(model, uncert), torch.Generator(device=dev).manual_seed(GEN_SEED)

        out = {}
        model, uncert, opt, gen = fresh()
        out['start'] = _params(model, uncert)
        res = training.train_step(model, opt, uncert, a, CLIP, gen)                                   # the call of before
        out['plain'], out['plain_m'], out['plain_res'] = _params(model, uncert), _buffers(model, opt, uncert), res
        out['plain_norm'], out['plain_counter'] = _bits(opt.last_norm), opt.skipped_steps

        model, uncert, opt, gen = fresh()
        res = training.train_step(model, opt, uncert, a, CLIP, gen, accum_steps=1, guard=False)
        out['keywords'], out['keywords_m'], out['keywords_res'] = _params(model, uncert), _buffers(model, opt, uncert), res

        # accum_steps=2 ...
        model, uncert, opt, gen = fresh()
        res = training.train_step(model, opt, uncert, [a, b], CLIP, gen, accum_steps=2)
        out['accum'], out['accum_m'], out['accum_res'] = _params(model, uncert), _buffers(model, opt, uncert), res
        out['accum_norm'] = _bits(opt.last_norm)

        # ... and the sequence it stands for
        model, uncert, opt, gen = fresh()
        opt.zero_grad(set_to_none=True)
        totals = []
        for batch in (a, b):
            o = training.forward_train(model, *batch, generator=gen)
            total = losses.multi_task_loss(list(o[8:14]), uncert)
            total.backward()
            totals.append(total.detach())
        opt.step(clip_norm=CLIP, clip_params=[p for p in model.parameters() if p.requires_grad], grad_scale=0.5)
        out['manual'], out['manual_m'] = _params(model, uncert), _buffers(model, opt, uncert)
        out['manual_loss'], out['manual_norm'] = (totals[0] + totals[1]) * 0.5, _bits(opt.last_norm)

        # guard=True: a good step, a bad one, a good one
        model, uncert, opt, gen = fresh()
        res = training.train_step(model, opt, uncert, a, CLIP, gen, guard=True)
        out['guard'], out['guard_m'], out['guard_res'] = _params(model, uncert), _buffers(model, opt, uncert), res
        out['guard_ok'], out['guard_count'] = float(res['ok']), int(res['skipped_steps'])
        with torch.no_grad():
            saved = uncert[PLANTED].clone()
            uncert[PLANTED] = -100.0
        out['bad_before'], out['bad_before_m'] = _params(model, uncert), _buffers(model, opt, uncert)
        res = training.train_step(model, opt, uncert, b, CLIP, gen, guard=True)
        out['bad'], out['bad_m'] = _params(model, uncert), _buffers(model, opt, uncert)
        out['bad_ok'], out['bad_count'], out['bad_loss'] = float(res['ok']), int(res['skipped_steps']), float(res['loss'])
        out['bad_norm'] = float(res['grad_norm'])
        out['bad_grads_finite'] = all(bool(torch.isfinite(p.grad).all()) for p in training.trainable_parameters(model).values())
        with torch.no_grad():
            uncert[PLANTED] = saved
        out['restored'] = _params(model, uncert)
        res = training.train_step(model, opt, uncert, b, CLIP, gen, guard=True)
        out['after'], out['after_ok'], out['after_count'] = _params(model, uncert), float(res['ok']), int(res['skipped_steps'])
        out['after_loss'] = float(res['loss'])
        out['trainable'] = sorted(training.trainable_parameters(model)) + ['uncert']
    finally:
        mp.undo()
    return out


def test_the_plain_step_moved_the_trainable_parameters(case):
    moved = _differing(case['start'], case['plain'])
    assert moved and set(moved) <= set(case['trainable']) and 'uncert' in moved
    assert case['plain_counter'] is None                     # no guarded call: no counter
    assert case['plain_norm'].shape == (2,)


def test_keywords_at_their_defaults_are_the_positional_call(case):
    from stereo_rcnn_amd import training
    assert _differing(case['plain'], case['keywords']) == [] and _differing(case['plain_m'], case['keywords_m']) == []
    assert set(case['keywords_res']) == {'loss', 'grad_norm'} | set(training.LOSS_NAMES)
    for k, v in case['plain_res'].items():
        assert np.array_equal(_bits(v), _bits(case['keywords_res'][k])), k


def test_two_accumulated_batches_are_the_manual_sequence(case):
    assert _differing(case['accum'], case['manual']) == [] and _differing(case['accum_m'], case['manual_m']) == []
    assert np.array_equal(case['accum_norm'], case['manual_norm']) and case['accum_norm'].shape == (3,)
    assert case['accum_norm'].view(np.float32)[2] == 1.0
    assert np.array_equal(_bits(case['accum_res']['loss']), _bits(case['manual_loss']))
    assert np.isfinite(float(case['accum_res']['loss']))
    assert all(t.is_cuda and t.dim() == 0 for t in case['accum_res'].values())
    assert 'ok' not in case['accum_res'] and 'skipped_steps' not in case['accum_res']
    # two batches are not one: the step differs from batch a's alone
    assert _differing(case['accum'], case['plain'])


def test_guard_with_finite_gradients_changes_no_bit(case):
    assert _differing(case['plain'], case['guard']) == [] and _differing(case['plain_m'], case['guard_m']) == []
    assert case['guard_ok'] == 1.0 and case['guard_count'] == 0
    for k, v in case['plain_res'].items():
        assert np.array_equal(_bits(v), _bits(case['guard_res'][k])), k
    assert case['guard_res']['skipped_steps'].dtype == torch.int32 and case['guard_res']['skipped_steps'].shape == (1,)


def test_a_step_with_a_non_finite_gradient_is_skipped(case):
    print('bad step: loss %r, gradient norm %r' % (case['bad_loss'], case['bad_norm']))
    assert not case['bad_grads_finite'] and not np.isfinite(case['bad_norm'])
    assert case['bad_ok'] == 0.0 and case['bad_count'] == 1
    assert _differing(case['bad_before'], case['bad']) == []              # (the planted value is in both)
    assert _differing(case['bad_before_m'], case['bad_m']) == []
    assert _differing(case['guard'], case['restored']) == []


def test_the_next_good_step_moves_on(case):
    assert case['after_ok'] == 1.0 and case['after_count'] == 1
    assert np.isfinite(case['after_loss'])
    moved = _differing(case['restored'], case['after'])
    assert moved and set(moved) <= set(case['trainable'])
    assert all(np.isfinite(v.view(np.float32)).all() for v in case['after'].values())
