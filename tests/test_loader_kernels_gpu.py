"""GPU: the batch assembly kernels (csrc/loader.hip) against the reference's own output (tests/golden/reference_loader.npz) and,
on shapes the golden does not hold, against tests/loader_ref.py (pinned to that golden by tests/test_loader_ref_cpu.py).  Every
comparison is exact; outputs are poisoned first, so an element the kernel does not write shows."""
import os

import numpy as np
import pytest
import torch

import loader_ref

pytestmark = pytest.mark.gpu
K = loader_ref.K_DEFAULT


@pytest.fixture(scope='module')
def g():
    return loader_ref.golden()


def _poisoned_gt(B, dev):
    out = [torch.full((B, K, c), float('nan'), dtype=torch.float32, device=dev) for c in (5, 5, 5, 5, 6)]
    out.append(torch.full((B,), -7, dtype=torch.int64, device=dev))
    return out


def _gt_launch(entries, scales, widths, keys, dev):
    from stereo_rcnn_amd import data, engine
    table, off = data.pack_gt_table(entries)
    B = len(entries)
    stride = max(1, max(len(k) for k in keys))
    kw = torch.zeros((B, stride), dtype=torch.int32)
    for b, k in enumerate(keys):
        kw[b, :len(k)] = data.keys_to_words(torch.from_numpy(np.asarray(k, dtype=np.int64)))
    slots = [(int(off[b]), int(off[b + 1] - off[b]), scales[b], float(widths[b])) for b in range(B)]
    out = engine.gt_batch(torch.from_numpy(table).to(dev), slots, kw.to(dev), K, out=_poisoned_gt(B, dev))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


def test_gt_batch_equals_the_reference(g, dev):
    for ci in range(int(g['hand_cases'])):
        e, (n, H, W, target), perm, im_info, expect, num = loader_ref.golden_hand_case(g, ci)
        scale = float(target) / float(min(H, W))
        got = _gt_launch([e], [scale], [im_info[1]], [loader_ref.keys_from_perm(perm)], dev)
        for a, b, name in zip(got[:5], expect, ('left', 'right', 'merge', 'dim_orien', 'kpts')):
            _same(a[0], b, 'case %d %s' % (ci, name))
            assert not a[0][num:].any(), 'rows past num_boxes are zero'
        assert got[5].dtype == np.int64 and got[5].tolist() == [num]


def test_gt_batch_three_entries_in_one_launch(g, dev):
    cases = [loader_ref.golden_hand_case(g, ci) for ci in (4, 0, 2)]          # n = 40, 1, 30
    rng = np.random.RandomState(3)
    entries, scales, widths, keys = [], [], [], []
    for e, (n, H, W, target), perm, im_info, _, _ in cases:
        entries.append(e)
        scales.append(float(target) / float(min(H, W)))
        widths.append(int(im_info[1]))
        keys.append(rng.randint(0, 2 ** 32, n, dtype=np.int64).astype(np.uint32))          # keys above 2^31 too
    assert max(int(k.max()) for k in keys) >= 2 ** 31
    got = _gt_launch(entries, scales, widths, keys, dev)
    for b, e in enumerate(entries):
        want, num = loader_ref.gt_padded(e, scales[b], widths[b], loader_ref.perm_from_keys(keys[b]))
        for a, w in zip(got[:5], want):
            _same(a[b], w, 'slot %d' % b)
        assert int(got[5][b]) == num


def test_gt_batch_equal_keys_rank_by_index_and_empty_entry(g, dev):
    e, (n, H, W, target), perm, im_info, _, _ = loader_ref.golden_hand_case(g, 3)          # n = 31
    scale = float(target) / float(min(H, W))
    keys = np.full(n, 5, dtype=np.uint32)
    keys[7] = 4                                              # one smaller key goes first, the ties stay in index order
    empty = {k: v[:0] for k, v in e.items() if isinstance(v, np.ndarray)}
    empty['flipped'] = False
    got = _gt_launch([e, empty], [scale, 1.0], [int(im_info[1]), 10], [keys, np.zeros(0, dtype=np.uint32)], dev)
    order = [7] + [i for i in range(n) if i != 7]
    want, num = loader_ref.gt_padded(e, scale, int(im_info[1]), order)
    assert np.array_equal(loader_ref.perm_from_keys(keys), order)
    for a, w in zip(got[:5], want):
        _same(a[0], w, 'ties')
        assert not a[1].any()
    assert got[5].tolist() == [30, 0]


def _images(pairs, flipped, targets, max_size, dev, pinned=False, poison=True):
    from stereo_rcnn_amd import engine
    t = []
    for l, r in pairs:
        l, r = torch.from_numpy(np.ascontiguousarray(l)), torch.from_numpy(np.ascontiguousarray(r))
        t.append((l.pin_memory(), r.pin_memory()) if pinned else (l.to(dev), r.to(dev)))
    scales = [float(tg) / float(min(l.shape[0], l.shape[1])) for (l, _), tg in zip(pairs, targets)]
    out = None
    if poison:
        sizes = [(int(round(l.shape[0] * s)), min(int(round(l.shape[1] * s)), max_size)) for (l, _), s in zip(pairs, scales)]
        shape = (len(pairs), 3, max(s[0] for s in sizes), max(s[1] for s in sizes))
        out = (torch.full(shape, float('nan'), dtype=torch.float32, device=dev), torch.full(shape, float('nan'), dtype=torch.float32, device=dev))
    il, ir, sizes = engine.preprocess_train(t, flipped, scales, max_size, device=dev, out=out)
    torch.cuda.synchronize()
    return il.cpu().numpy(), ir.cpu().numpy(), sizes


def test_preprocess_train_equals_the_reference(g, dev):
    cropped = False
    for ci in range(int(g['img_cases'])):
        pre = 'img_%d_' % ci
        H, W, target, max_size, flipped = (int(v) for v in g[pre + 'meta'])
        il, ir, sizes = _images([(g[pre + 'left'], g[pre + 'right'])], [bool(flipped)], [target], max_size, dev, pinned=(ci % 2 == 1))
        _same(il[0], g[pre + 'blob_left'][0].transpose(2, 0, 1), 'case %d left' % ci)
        _same(ir[0], g[pre + 'blob_right'][0].transpose(2, 0, 1), 'case %d right' % ci)
        assert sizes[0] == (il.shape[2], il.shape[3])
        cropped = cropped or il.shape[3] == max_size
    assert cropped


@pytest.fixture(scope='module')
def demo_pair():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'demo_pair_u8.npz'))


@pytest.fixture(scope='module')
def demo_ref(demo_pair):
    """oracle.preprocess of the demo pair's two eyes, plain and mirrored: computed once."""
    from oracle import preprocess as opre
    out = {}
    for eye in ('left', 'right'):
        out[eye, False] = opre.prepare_image(demo_pair[eye])[0][0]
        out[eye, True] = opre.prepare_image(np.ascontiguousarray(demo_pair[eye][:, ::-1, :]))[0][0]
    return out


@pytest.mark.parametrize('flipped', [False, True])
def test_preprocess_train_full_size(demo_pair, demo_ref, dev, flipped):
    il, ir, sizes = _images([(demo_pair['left'], demo_pair['right'])], [flipped], [600], 2484, dev)
    assert il.shape == (1, 3, 600, 1987) and sizes == [(600, 1987)]
    _same(il[0], demo_ref['right', True] if flipped else demo_ref['left', False], 'left')
    _same(ir[0], demo_ref['left', True] if flipped else demo_ref['right', False], 'right')


def test_preprocess_train_pads_a_batch_of_two_sizes(g, dev):
    a = (g['img_0_left'], g['img_0_right'])            # 7 x 11, target 11
    b = (g['img_4_left'], g['img_4_right'])            # 37 x 41, target 48
    c = (g['img_2_left'], g['img_2_right'])            # 8 x 13, target 13
    il, ir, sizes = _images([a, b, c], [True, False, False], [11, 48, 13], 2484, dev)
    want = []
    for pair, f, t in zip((a, b, c), (True, False, False), (11, 48, 13)):
        want.append(loader_ref.image_blobs(pair[0], pair[1], f, t))
    assert il.shape == (3, 3, 48, 53)
    for s, (wl, wr, _) in enumerate(want):
        oh, ow = wl.shape[1], wl.shape[2]
        assert sizes[s] == (oh, ow)
        _same(il[s, :, :oh, :ow], wl, 'slot %d left' % s)
        _same(ir[s, :, :oh, :ow], wr, 'slot %d right' % s)
        for blob in (il, ir):
            pad = blob[s].copy()
            pad[:, :oh, :ow] = 0
            assert not pad.any() and not np.isnan(pad).any(), 'zero padding on a poisoned buffer'


def test_srcnn_preprocess_is_unchanged(demo_pair, demo_ref, dev):
    from stereo_rcnn_amd import engine
    for eye in ('left', 'right'):
        out, scale = engine.preprocess(torch.from_numpy(demo_pair[eye]).to(dev))
        _same(out[0].cpu().numpy(), demo_ref[eye, False], eye)
        assert scale == 1.6
