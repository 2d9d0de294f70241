"""GPU: the optimiser step -- srcnn_grad_norm + srcnn_sgd_step behind stereo_rcnn_amd.optim.SGD, and net_utils.clip_gradient --
against the numpy restatements of tests/optim_ref.py.

One list for every test: tensors of 1, 2, 6, 7, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 5 elements, a tensor
without elements, one whose gradient is None, a 4-byte-aligned view (offset of one float from a 16-byte boundary) for each of p, g
and m, and TENSORS_PER_LAUNCH + 3 small tensors so that the list spans launches.  Parameters, gradients and (from the second step
on) momentum buffers are slices of one arena filled with a guard value, at least 16 guard floats on both sides of every slice.

Parameters and momentum buffers must be BIT-EQUAL to the float32 restatement fed the kernel's own coefficient; the norm and the
coefficient are BIT-EQUAL to the restatement of the two summation stages (optim_ref.grad_norm_f32) and the norm is also compared
with float64 within optim_ref.norm_bound(); only the comparison with torch.optim.SGD has a measured tolerance
(tests/optim_tolerances.py)."""
import copy

import numpy as np
import pytest
import torch

import optim_ref as R
import optim_tolerances as OT

pytestmark = pytest.mark.gpu

GUARD = 12345.0
CLIP = 10.0


@pytest.fixture(scope='module')
def lib(dev):
    import __graft_entry__ as ge
    ge.build()
    from stereo_rcnn_amd import _lib
    _lib.lib()
    return _lib


def _sizes(lib):
    C, T = lib.OPT_CHUNK, lib.OPT_TENSORS_PER_LAUNCH
    named = [1, 2, 6, 7, 255, 256, 257, C - 1, C, C + 1, 2 * C + 5, 0, 5, 1000, 1000, 1000]
    return named + [3 + (i % 9) for i in range(T + 3)]


NO_GRAD, VIEW_P, VIEW_G, VIEW_M = 12, 13, 14, 15          # positions in _sizes()


class Arena(object):
    """Slices of one guard-filled device buffer: 16-byte aligned unless `odd` (then one float past such a boundary)."""

    def __init__(self, dev, floats):
        self.buf = torch.full((floats,), GUARD, dtype=torch.float32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.off = 16
        self.mask = torch.ones(floats, dtype=torch.bool, device=dev)        # True = guard

    def take(self, n, odd=False):
        start = (self.off + 3) // 4 * 4 + (1 if odd else 0)
        self.off = start + n + 16
        assert self.off <= self.buf.numel()
        self.mask[start:start + n] = False
        t = self.buf[start:start + n]
        assert n == 0 or (t.data_ptr() % 16 == (4 if odd else 0))
        return t

    def guards_intact(self):
        return bool((self.buf[self.mask] == GUARD).all())


def _u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _bits_equal(t, a):
    return np.array_equal(_u32(t), np.ascontiguousarray(a, np.float32).view(np.uint32))


def _hyper(i):
    """Per-tensor (lr, weight decay, clipped): the reference's groups differ in exactly these."""
    return 0.01 * (1 + i % 3), (0.0 if i % 2 else 1e-3), i % 5 != 0


def _grads(sizes, step, scale):
    rng = np.random.RandomState(100 + step)
    return [(rng.randn(n) * scale).astype(np.float32) for n in sizes]


GRAD_SCALES = (1.0, 0.5, 0.01)      # norms of the clipped tensors: ~135, ~68 (clipped to 10) and ~1.4 (coefficient exactly 1)


def run_steps(lib, dev, momentum, clip_norm=CLIP, check=True):
    """Three steps of optim.SGD over the list, every step checked against the restatement.  Returns the final parameters and
    momentum buffers as uint32 arrays (for the repeatability test)."""
    from stereo_rcnn_amd import optim
    sizes = _sizes(lib)
    arena = Arena(dev, 4 * sum(sizes) * 3 + 64 * 40 * len(sizes))
    rng = np.random.RandomState(7)
    init = [rng.randn(n).astype(np.float32) for n in sizes]
    params = []
    for i, (n, v) in enumerate(zip(sizes, init)):
        t = arena.take(n, odd=(i == VIEW_P))
        t.copy_(torch.from_numpy(v))
        params.append(t.detach().requires_grad_(True))
    groups = [{'params': [p], 'lr': _hyper(i)[0], 'weight_decay': _hyper(i)[1]} for i, p in enumerate(params)]
    opt = optim.SGD(groups, lr=0.5, momentum=momentum)
    clip_params = [p for i, p in enumerate(params) if _hyper(i)[2]]
    ref_p, ref_m = [v.copy() for v in init], [None] * len(sizes)
    norms = []
    for step in range(3):
        gs = _grads(sizes, step, GRAD_SCALES[step])
        for i, (p, g) in enumerate(zip(params, gs)):
            if i == NO_GRAD:
                p.grad = None
                continue
            t = arena.take(p.numel(), odd=(i == VIEW_G))
            t.copy_(torch.from_numpy(g))
            p.grad = t
        if step == 1 and momentum != 0:
            # re-home the buffers step 0 created into the arena (same values): guards around m, and a 4-byte-aligned m
            for i, p in enumerate(params):
                if i == NO_GRAD:
                    continue
                t = arena.take(p.numel(), odd=(i == VIEW_M))
                t.copy_(opt.state[p]['momentum_buffer'])
                opt.state[p]['momentum_buffer'] = t
        opt.step(clip_norm=clip_norm, clip_params=clip_params)
        if clip_norm is None:
            coef = None
        else:
            norm, coef = (np.float32(v) for v in opt.last_norm.cpu().numpy())
            norms.append((float(norm), float(coef)))
        if not check:
            continue
        if clip_norm is not None:
            in_norm = [g for i, g in enumerate(gs) if _hyper(i)[2] and i != NO_GRAD]           # clip_params with a gradient, in list order
            assert _bits_equal(opt.last_norm, np.array(R.grad_norm_f32(in_norm, clip_norm))), ('norm, coefficient', step)
            want = R.norm_f64(in_norm)
            rel = abs(float(norm) - want) / want
            print('step %d: norm %.9g (float64 %.9g), relative error %.3e (bound %.3e), coefficient %.9g' % (step, norm, want, rel, R.norm_bound(), coef))
            assert rel <= R.norm_bound()
            assert coef == np.float32(clip_norm) / max(norm, np.float32(clip_norm))        # one float32 division
            if norm <= clip_norm:
                assert coef == np.float32(1.0)
        for i, (p, g) in enumerate(zip(params, gs)):
            if i == NO_GRAD:
                assert _bits_equal(p, init[i]) and p not in opt.state
                continue
            lr, wd, clipped = _hyper(i)
            ref_p[i], ref_m[i] = R.sgd_step_f32(ref_p[i], g, ref_m[i], lr, wd, momentum, step == 0, coef if (clipped and coef is not None) else None)
            assert _bits_equal(p, ref_p[i]), ('parameter', step, i, sizes[i])
            if momentum != 0:
                assert _bits_equal(opt.state[p]['momentum_buffer'], ref_m[i]), ('momentum buffer', step, i, sizes[i])
            else:
                assert 'momentum_buffer' not in opt.state[p]
            assert _bits_equal(p.grad, g), ('the gradient was modified', step, i)
        assert arena.guards_intact(), step
    if check and clip_norm is not None:
        assert norms[0][1] < 1.0 and norms[1][1] < 1.0 and norms[2][1] == 1.0, norms
    final = [_u32(p) for p in params] + [_u32(opt.state[p]['momentum_buffer']) for p in params if 'momentum_buffer' in opt.state.get(p, {})]
    return final, norms


@pytest.mark.parametrize('momentum', [0.9, 0.0])
def test_three_steps_bit_equal_to_the_restatement(lib, dev, momentum):
    run_steps(lib, dev, momentum)


def test_unclipped_step(lib, dev):
    run_steps(lib, dev, 0.9, clip_norm=None)


def test_two_runs_are_bit_equal(lib, dev):
    a, na = run_steps(lib, dev, 0.9, check=False)
    b, nb = run_steps(lib, dev, 0.9, check=False)
    assert na == nb
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _eager_clip(grads, clip_norm):
    """The reference's clip_gradient in eager torch (net_utils.py:37-49; its np.sqrt of a device value as torch.sqrt)."""
    total = 0
    for g in grads:
        total = total + g.norm() ** 2
    total = torch.sqrt(total)
    coef = clip_norm / torch.clamp(total, min=clip_norm)
    for g in grads:
        g.mul_(coef)


def test_against_torch_sgd_on_the_device(lib, dev):
    from stereo_rcnn_amd import optim
    from tolerances import observe
    sizes = [n for i, n in enumerate(_sizes(lib)) if i != NO_GRAD]
    rng = np.random.RandomState(7)
    init = [torch.from_numpy(rng.randn(n).astype(np.float32)).to(dev) for n in sizes]
    mine = [t.clone().requires_grad_(True) for t in init]
    theirs = [t.clone().requires_grad_(True) for t in init]
    groups = lambda ps: [{'params': [p], 'lr': _hyper(i)[0], 'weight_decay': _hyper(i)[1]} for i, p in enumerate(ps)]
    a, b = optim.SGD(groups(mine), lr=0.5, momentum=0.9), torch.optim.SGD(groups(theirs), lr=0.5, momentum=0.9)
    for step in range(3):
        gs = [torch.from_numpy(g).to(dev) for g in _grads(sizes, step, GRAD_SCALES[step])]
        for p, q, g in zip(mine, theirs, gs):
            p.grad, q.grad = g.clone(), g.clone()
        a.step(clip_norm=CLIP)
        _eager_clip([q.grad for q in theirs], CLIP)
        b.step()
    worst_p = worst_m = 0.0
    for p, q in zip(mine, theirs):
        if p.numel() == 0:
            continue
        worst_p = max(worst_p, float((p.detach().double() - q.detach().double()).abs().max() / q.detach().double().abs().max()))
        ma, mb = a.state[p]['momentum_buffer'], b.state[q]['momentum_buffer']
        worst_m = max(worst_m, float((ma.double() - mb.double()).abs().max() / mb.double().abs().max()))
    print('against torch.optim.SGD after three steps: parameters %.3e, momentum buffers %.3e' % (worst_p, worst_m))
    observe('optim_sgd_vs_torch_param', worst_p), observe('optim_sgd_vs_torch_momentum', worst_m)
    assert worst_p <= OT.LIMITS['optim_sgd_vs_torch_param'] and worst_m <= OT.LIMITS['optim_sgd_vs_torch_momentum']


def test_state_dict_round_trip_through_torch_sgd(lib, dev):
    from stereo_rcnn_amd import optim
    sizes = [7, 257, lib.OPT_CHUNK + 1, 1000]
    rng = np.random.RandomState(3)
    x = [torch.from_numpy(rng.randn(n).astype(np.float32)).to(dev).requires_grad_(True) for n in sizes]
    groups = lambda ps: [{'params': [p], 'lr': _hyper(i)[0], 'weight_decay': _hyper(i)[1]} for i, p in enumerate(ps)]
    a = optim.SGD(groups(x), lr=0.5, momentum=0.9)
    g0, g1 = ([torch.from_numpy(g).to(dev) for g in _grads(sizes, s, 1.0)] for s in (0, 1))
    for p, g in zip(x, g0):
        p.grad = g.clone()
    a.step(clip_norm=CLIP)
    y = [p.detach().clone().requires_grad_(True) for p in x]
    t = torch.optim.SGD(groups(y), lr=0.25, momentum=0.5)
    # (a deep copy, as a checkpoint on disk is: load_state_dict adopts the tensors it is given, and `a` goes on updating its own)
    t.load_state_dict(copy.deepcopy(a.state_dict()))
    assert t.param_groups[0]['momentum'] == 0.9 and t.param_groups[1]['lr'] == _hyper(1)[0]
    assert all(torch.equal(t.state[q]['momentum_buffer'], a.state[p]['momentum_buffer']) for p, q in zip(x, y))
    b = optim.SGD(groups(y), lr=0.25, momentum=0.5)
    b.load_state_dict(copy.deepcopy(t.state_dict()))
    for p, q, g in zip(x, y, g1):
        p.grad, q.grad = g.clone(), g.clone()
    a.step(clip_norm=CLIP)
    b.step(clip_norm=CLIP)
    for p, q in zip(x, y):
        assert np.array_equal(_u32(p), _u32(q))
        assert np.array_equal(_u32(a.state[p]['momentum_buffer']), _u32(b.state[q]['momentum_buffer']))
        assert b.state[q]['momentum_buffer'].data_ptr() != a.state[p]['momentum_buffer'].data_ptr()


def test_refusals_on_the_device(lib, dev):
    from stereo_rcnn_amd import optim
    w = torch.zeros(4, 6, device=dev)
    p = w.t().requires_grad_(True)                          # not contiguous
    opt = optim.SGD([p], lr=0.1)
    p.grad = torch.ones(6, 4, device=dev)
    with pytest.raises(ValueError):
        opt.step()
    h = torch.zeros(8, device=dev, dtype=torch.float16, requires_grad=True)
    opt = optim.SGD([h], lr=0.1)
    h.grad = torch.ones(8, device=dev, dtype=torch.float16)
    with pytest.raises(TypeError):
        opt.step()
    assert float(h.detach().float().abs().sum()) == 0.0


def test_adjust_learning_rate_and_clip_gradient(lib, dev):
    from stereo_rcnn_amd import optim
    from stereo_rcnn_amd.model.utils import net_utils
    model = torch.nn.Sequential(torch.nn.Linear(257, 19), torch.nn.Linear(19, 7)).to(dev)
    model[1].bias.requires_grad_(False)
    opt = optim.SGD([{'params': [p], 'lr': 0.01 * (i + 1)} for i, p in enumerate(model.parameters())], lr=1.0, momentum=0.9)
    net_utils.adjust_learning_rate(opt, 0.1)
    assert [g['lr'] for g in opt.param_groups] == [0.1 * 0.01 * (i + 1) for i in range(4)]
    rng = np.random.RandomState(5)
    for clip_norm, clips in ((1.0, True), (1000.0, False)):
        gs = {}
        for name, p in model.named_parameters():
            gs[name] = rng.randn(*p.shape).astype(np.float32)
            p.grad = torch.from_numpy(gs[name]).to(dev)
        frozen = _u32(model[1].bias.grad)
        norm = net_utils.clip_gradient(model, clip_norm)
        assert norm.is_cuda and norm.dim() == 0
        want = R.norm_f64([g for name, g in gs.items() if name != '1.bias'])
        assert abs(float(norm) - want) / want <= R.norm_bound()
        n32 = np.float32(float(norm))
        coef = np.float32(clip_norm) / max(n32, np.float32(clip_norm))
        assert (coef < 1.0) == clips
        for name, p in model.named_parameters():
            if name == '1.bias':
                assert np.array_equal(_u32(p.grad), frozen)             # requires_grad False: neither counted nor scaled
            else:
                assert _bits_equal(p.grad, (gs[name] * coef).astype(np.float32)), name


@pytest.mark.parametrize('coef', [0.37, 1.0])
def test_scale_grads_over_the_list(lib, dev, coef):
    """srcnn_grad_scale over the module's list (chunk tails, a tensor without elements, a 4-byte-aligned view, more tensors than
    one launch takes): g * float32(coef), one rounding; a coefficient of exactly 1 is the kernel's early return, no bit moves."""
    from stereo_rcnn_amd import optim
    sizes = _sizes(lib)
    arena = Arena(dev, sum(sizes) + 40 * len(sizes))
    gs = _grads(sizes, 0, 1.0)
    slices = []
    for i, g in enumerate(gs):
        t = arena.take(g.size, odd=(i == VIEW_G))
        t.copy_(torch.from_numpy(g))
        slices.append(t)
    k = torch.tensor([coef], dtype=torch.float32, device=dev)
    optim.scale_grads(slices, k)
    for i, (t, g) in enumerate(zip(slices, gs)):
        want = g if coef == 1.0 else (g * np.float32(coef)).astype(np.float32)
        assert _bits_equal(t, want), (i, sizes[i])
    assert _bits_equal(k, [coef]) and arena.guards_intact()


def test_index_past_2_31(lib, dev):
    """A tensor of more than 2^31 elements: chunk offsets beyond 32 bits.  Zeros but for two elements behind the 2^31 mark, so
    the norm (5) and the update are known without a host copy."""
    from stereo_rcnn_amd import optim
    n = (1 << 31) + lib.OPT_CHUNK + 5
    g = torch.zeros(n, dtype=torch.float32, device=dev)
    g[(1 << 31) + 1] = 3.0
    g[n - 1] = 4.0
    out = optim.grad_norm([g], 2.5).cpu().numpy()
    assert out[0] == np.float32(5.0) and out[1] == np.float32(0.5)
    p = torch.zeros(n, dtype=torch.float32, device=dev, requires_grad=True)
    p.grad = g
    optim.SGD([p], lr=0.5).step(clip_norm=2.5)
    assert float(p.detach()[(1 << 31) + 1]) == -0.75 and float(p.detach()[n - 1]) == -1.0
    assert int(torch.count_nonzero(p.detach())) == 2
