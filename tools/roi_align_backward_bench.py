"""ROIAlign backward at the reference's training shape: the fused NHWC gather against what it replaces.

    python tools/roi_align_backward_bench.py [--out profiles/roi_align_backward.txt] [--reps 30]

Shape: 512 rois per image (cfg.TRAIN.BATCH_SIZE), one image of 600 x 1987 (pyramid maps 150x497, 75x249, 38x125, 19x63), 256
channels, A = 7 and A = 14, rois drawn so that all four levels are populated.  One process, warm; the two versions ALTERNATE and
every run is timed with HIP events; medians are reported.
  * product   : srcnn_pyramid_roi_align_backward (one launch, the 2x2 average folded in, every map element written once);
  * reference : the reference's own ROIAlignBackward kernel (oracle/_ref, built by build()) run per level on that level's
    rois PLUS the hipMemsetAsync of the gradient maps it accumulates into.  It is handed the lattice gradient directly (the
    avg_pool2d backward in front of it is not charged to it);
  * compulsory bytes = gradient maps written once + grad_out read once, over the product's time.
Runner and timer: tools/benchlib.py."""
import ctypes

import benchlib

MAPS = [(150, 497), (75, 249), (38, 125), (19, 63)]
IM_H, IM_W, C, N = 600.0, 1987.0, 256, 512
STREAM_TBPS = (4.0, 4.3)        # what the streaming kernels of DESIGN section 4 reach


def rois_all_levels(seed=0):
    import numpy as np
    g = np.random.default_rng(seed)
    side = np.concatenate([g.uniform(12, 45, N // 4), g.uniform(58, 125, N // 4), g.uniform(150, 340, N // 4), g.uniform(400, 590, N // 4)])
    g.shuffle(side)
    aspect = g.uniform(1.0, 1.6, N)                                      # wider than high, as the image: every box fits inside it
    w, h = side * np.sqrt(aspect), side / np.sqrt(aspect)
    x1, y1 = g.uniform(0, 1, N) * (IM_W - 1 - w), g.uniform(0, 1, N) * (IM_H - 1 - h)
    rois = np.stack([np.zeros(N), x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    lv = np.log(np.sqrt((rois[:, 4] - rois[:, 2] + 1.) * (rois[:, 3] - rois[:, 1] + 1.)) / 224.) + 4.
    level = (np.clip(np.floor(np.abs(lv) + 0.5), 2, 5) - 2).astype(int)
    # the kernel routes in float32 (logf): keep every roi far from a rounding boundary, so that product and reference are
    # handed the same rois per level
    margin = np.abs(np.abs(lv - np.floor(lv)) - 0.5)
    keep = margin > 1e-3
    rois[~keep] = rois[keep][0]
    level[~keep] = level[keep][0]
    assert all((level == l).sum() >= N // 8 for l in range(4)), 'a pyramid level is nearly empty'
    return rois, level


def child(reps):
    import numpy as np
    import torch
    from oracle import ref_ops
    from stereo_rcnn_amd import _lib
    dev = benchlib.device()
    L = _lib.lib()
    have_ref = ref_ops.available('fma')
    if have_ref:
        RL = ref_ops.lib('fma')
        RL.ROIAlignBackwardLaucher.restype = ctypes.c_int
        RL.ROIAlignBackwardLaucher.argtypes = [ctypes.c_void_p, ctypes.c_float] + [ctypes.c_int] * 7 + [ctypes.c_void_p] * 3
    rois_np, level = rois_all_levels()
    rois = torch.from_numpy(rois_np).to(dev)
    print('shape: %d rois, %d channels, maps %s, rois per level %s' % (N, C, MAPS, [int((level == l).sum()) for l in range(4)]))
    stream = torch.cuda.current_stream().cuda_stream
    for A in (7, 14):
        gout = torch.randn(N, A, A, C, device=dev)
        grads = [torch.empty(1, h, w, C, device=dev) for h, w in MAPS]
        ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in grads])
        mh = (ctypes.c_int * 4)(*[h for h, _ in MAPS])
        mw = (ctypes.c_int * 4)(*[w for _, w in MAPS])

        def product():
            _lib.check(L.srcnn_pyramid_roi_align_backward(gout.data_ptr(), C, 0, rois.data_ptr(), N, A, C, IM_H, ptrs, mh, mw, 1, 0,
                                                          None, stream))

        # the reference's inputs: per level, that level's rois and a lattice gradient (n_l, C, A+1, A+1) NCHW; NCHW maps
        sel = [torch.from_numpy(np.flatnonzero(level == l)).to(dev) for l in range(4)]
        lrois = [rois[s].contiguous() for s in sel]
        ltop = [torch.randn(len(s), C, A + 1, A + 1, device=dev) for s in sel]
        rgrads = [torch.empty(1, C, h, w, device=dev) for h, w in MAPS]

        def reference():
            for l, (h, w) in enumerate(MAPS):
                rgrads[l].zero_()                                                    # hipMemsetAsync on the current stream
                RL.ROIAlignBackwardLaucher(ltop[l].data_ptr(), float(np.float32(h / IM_H)), 1, len(sel[l]), h, w, C, A + 1, A + 1,
                                           lrois[l].data_ptr(), rgrads[l].data_ptr(), ctypes.c_void_p(stream))

        times = benchlib.alternating([('product', product)] + ([('reference', reference)] if have_ref else []), reps, warmup=5)
        med = {k: benchlib.stats(v)[0] for k, v in times.items()}
        nbytes = 4.0 * (sum(h * w for h, w in MAPS) * C + N * A * A * C)
        tbps = nbytes / (med['product'] * 1e-3) / 1e12
        print('A=%d fused NHWC backward (srcnn_pyramid_roi_align_backward): median %.3f ms (min %.3f, max %.3f, %d runs)'
              % (A, med['product'], min(times['product']), max(times['product']), reps))
        if have_ref:
            print('A=%d reference ROIAlignBackward per level + hipMemsetAsync of the maps: median %.3f ms (min %.3f, max %.3f); '
                  'product / reference = %.2f' % (A, med['reference'], min(times['reference']), max(times['reference']),
                                                  med['product'] / med['reference']))
        else:
            print('A=%d reference kernel: oracle/_ref not built, not measured' % A)
        print('A=%d compulsory bytes %.1f MB (maps written once + grad_out read once) over the product time: %.0f GB/s = %.2f-%.2f of '
              'the %.1f-%.1f TB/s streaming kernels reach' % (A, nbytes / 1e6, tbps * 1e3, tbps / STREAM_TBPS[1], tbps / STREAM_TBPS[0],
                                                              STREAM_TBPS[0], STREAM_TBPS[1]))


def main():
    benchlib.main(__file__, child, out='roi_align_backward.txt', reps=30, timeout=300,
                  header='# python tools/roi_align_backward_bench.py --reps %(reps)d   (see the tool for what each line measures)')


if __name__ == '__main__':
    main()
