"""numpy restatement of the per-iteration half of the reference's data loader (minibatch.py, roibatchLoader.py:72-110, blob.py),
pinned bit for bit to the reference's own output by tests/test_loader_ref_cpu.py (tests/golden/reference_loader.npz), so that the
GPU tests may use it on shapes the golden does not hold.  Images go through oracle.preprocess (the OpenCV restatement)."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import preprocess as opre          # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'reference_loader.npz')
K_DEFAULT = 30                                  # cfg.MAX_NUM_GT_BOXES


def golden():
    return np.load(GOLDEN)


def keys_from_perm(perm):
    """uint32 keys whose (key, index) order is `perm` (shuffled[j] = rows[perm[j]])."""
    keys = np.zeros(len(perm), dtype=np.uint32)
    keys[np.asarray(perm, dtype=np.int64)] = np.arange(len(perm), dtype=np.uint32)
    return keys


def perm_from_keys(keys):
    """Rows ranked by (key, index): a stable sort by key."""
    return np.argsort(np.asarray(keys, dtype=np.uint64), kind='stable')


def image_blobs(left_u8, right_u8, flipped, target, max_size=2484):
    """minibatch._get_image_blob for one pair: (blob_left (3, OH, OWc), blob_right, im_scale).  flipped: the left blob is the
    mirrored RIGHT image and the other way round; the mirror comes before the mean and the resize."""
    if flipped:
        left_u8, right_u8 = right_u8[:, ::-1, :], left_u8[:, ::-1, :]
    bl, scale = opre.prepare_image(np.ascontiguousarray(left_u8), target_short=target, max_size=max_size)
    br, _ = opre.prepare_image(np.ascontiguousarray(right_u8), target_short=target, max_size=max_size)
    return bl[0], br[0], scale


def gt_rows(entry, im_scale, im_width):
    """get_minibatch's five ground-truth arrays before the shuffle (minibatch.py:43-82).  im_scale: the Python float."""
    inds = np.where(entry['gt_classes'] != 0)[0]
    out = []
    for name in ('boxes_left', 'boxes_right', 'boxes_merge'):
        g = np.empty((len(inds), 5), dtype=np.float32)
        g[:, 0:4] = entry[name][inds, :] * im_scale
        for i in range(g.shape[0]):
            g[i, 0] = min(g[i, 0], im_width)
        g[:, 4] = entry['gt_classes'][inds]
        out.append(g)
    dim = np.empty((len(inds), 5), dtype=np.float32)
    dim[:, 0:3] = entry['dim_orien'][inds][:, 0:3]
    for i in range(dim.shape[0]):
        dim[i, 3] = math.sin(entry['dim_orien'][inds][i, 3])
        dim[i, 4] = math.cos(entry['dim_orien'][inds][i, 3])
    out.append(dim)
    kpts = entry['kpts'][inds] * im_scale
    for i in range(kpts.shape[0]):
        for j in range(6):
            if kpts[i, j] < 0 or kpts[i, j] > im_width - 1:
                kpts[i, j] = -1
    out.append(kpts.astype(np.float32))
    return out


def gt_padded(entry, im_scale, im_width, perm, K=K_DEFAULT):
    """roibatchLoader.py:72-110: the rows shuffled by `perm`, the first min(n, K) kept, zero padding.  Returns the five (K, c)
    arrays and num_boxes."""
    rows = gt_rows(entry, im_scale, im_width)
    n = rows[0].shape[0]
    num = min(n, K)
    out = []
    for r in rows:
        p = np.zeros((K, r.shape[1]), dtype=np.float32)
        p[:num] = r[np.asarray(perm, dtype=np.int64)][:num]
        out.append(p)
    return out, num


def batch(entries, images, targets, keys, K=K_DEFAULT, max_size=2484):
    """forward_train's nine inputs as numpy arrays for a batch: entries (roidb dicts), images [(left_u8, right_u8)], targets
    (cfg.TRAIN.SCALES entries), keys (per entry a uint32 array).  B > 1: zero padding to the batch maximum, every im_info row and
    every clamp from the image's own size (stereo_rcnn_amd/data.py)."""
    blobs = [image_blobs(l, r, bool(e['flipped']), t, max_size) for e, (l, r), t in zip(entries, images, targets)]
    B = len(entries)
    Hm, Wm = max(b[0].shape[1] for b in blobs), max(b[0].shape[2] for b in blobs)
    im_left, im_right = np.zeros((B, 3, Hm, Wm), dtype=np.float32), np.zeros((B, 3, Hm, Wm), dtype=np.float32)
    im_info = np.zeros((B, 3), dtype=np.float32)
    gts = [np.zeros((B, K, c), dtype=np.float32) for c in (5, 5, 5, 5, 6)]
    num = np.zeros(B, dtype=np.int64)
    for b, (e, (bl, br, scale)) in enumerate(zip(entries, blobs)):
        oh, ow = bl.shape[1], bl.shape[2]
        im_left[b, :, :oh, :ow], im_right[b, :, :oh, :ow] = bl, br
        im_info[b] = [oh, ow, scale]
        g, num[b] = gt_padded(e, scale, ow, perm_from_keys(keys[b]), K)
        for dst, src in zip(gts, g):
            dst[b] = src
    return [im_left, im_right, im_info] + gts + [num]


def golden_roidb_entry(g, i):
    e = {k: g['roidb_%d_%s' % (i, k)] for k in ('boxes_left', 'boxes_right', 'boxes_merge', 'dim_orien', 'kpts', 'gt_classes')}
    flipped, width, height, need_crop = (int(v) for v in g['roidb_%d_meta' % i])
    e.update(flipped=bool(flipped), width=width, height=height, need_crop=need_crop)
    if not flipped:
        e.update({k: g['roidb_%d_%s' % (i, k)] for k in ('kpts_right', 'truncation', 'occlusion')})
    return e


def golden_hand_case(g, ci):
    pre = 'hand_%d_' % ci
    e = {k: g[pre + k] for k in ('boxes_left', 'boxes_right', 'boxes_merge', 'dim_orien', 'kpts', 'gt_classes')}
    n, H, W, target, flipped = (int(v) for v in g[pre + 'meta'])
    e['flipped'] = bool(flipped)
    expect = [g[pre + k] for k in ('gt_left', 'gt_right', 'gt_merge', 'gt_dim_orien', 'gt_kpts')]
    return e, (n, H, W, target), g[pre + 'perm'], g[pre + 'im_info'], expect, int(g[pre + 'num_boxes'])


def write_dataset(root, frames, images=None):
    """A KITTI-style tree under `root`: frames = [(id, (H, W), calib text, label text)]; images: {id: (left_u8, right_u8)} or
    None for blank ones.  Returns the split file's path."""
    from PIL import Image
    base = os.path.join(root, 'training')
    for d in ('image_2', 'image_3', 'label_2', 'calib'):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    for fid, (H, W), calib, label in frames:
        pair = images[fid] if images is not None else (np.zeros((H, W, 3), dtype=np.uint8),) * 2
        for d, im in zip(('image_2', 'image_3'), pair):
            Image.fromarray(im).save(os.path.join(base, d, fid + '.png'))
        with open(os.path.join(base, 'label_2', fid + '.txt'), 'w') as fh:
            fh.write(label)
        with open(os.path.join(base, 'calib', fid + '.txt'), 'w') as fh:
            fh.write(calib)
    split = os.path.join(root, 'train.txt')
    with open(split, 'w') as fh:
        fh.write('\n'.join(f[0] for f in frames))
    return split


# ---- a KITTI-style dataset at 1/7.6 of KITTI's size for the loader's GPU tests: 52 x 164 and 50 x 160 pairs become 104 x 328 and
# 104 x 333 at cfg.TRAIN.SCALES = (104,), the size of tests/forward_train_ref.py's case
SMALL_CALIB = ("P0: 95 0 82 0 0 95 24 0 0 0 1 0\nP1: 95 0 82 -51.03 0 95 24 0 0 0 1 0\n"
         "P2: 95 0 82 5.906 0 95 24 0.0285 0 0 1 0.002745884\nP3: 95 0 82 -44.70 0 95 24 0.2897 0 0 1 0.002729905\n"
         "R0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 0 -1 0 0 0 0 -1 0 1 0 0 0\nTr_imu_to_velo: 1 0 0 0 0 1 0 0 0 0 1 0\n")


def _car(alpha, x, z, ry, h=1.5, w=1.6, l=3.9, cls='Car', trunc=0.0, occ=0):
    return '%s %.2f %d %.2f 0 0 50 50 %.2f %.2f %.2f %.2f 1.65 %.2f %.2f' % (cls, trunc, occ, alpha, h, w, l, x, z, ry)


SMALL_FRAMES = [
    ('000010', (52, 164), [_car(-1.2, -2.6, 7.5, -1.45), _car(0.6, 2.4, 9.0, 0.85), _car(1.9, 0.2, 13.0, 1.92)]),
    ('000011', (50, 160), [_car(2.2, -3.4, 8.5, 1.8), _car(-0.4, 3.0, 7.0, 0.0), 'DontCare -1 -1 -10 1 1 9 9 -1 -1 -1 -1000 -1000 -1000 -10']),
    ('000012', (52, 164), [_car(-2.0, 3.6, 10.0, -1.7), _car(1.0, -1.8, 6.5, 0.7), _car(0.1, -8.0, 12.0, -0.45, cls='Van')]),
    ('000013', (50, 160), [_car(1.4, 0.4, 8.0, 1.45), _car(-1.6, -4.2, 11.0, -1.95), _car(0.3, 5.0, 12.5, 0.68)]),
]
