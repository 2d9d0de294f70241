"""Records the results of the REFERENCE'S OWN NMS / ROIAlign kernels (oracle/_ref, built by oracle/build.py:build_ref where the
reference sources can be read) on the inputs of tests/test_ref_kernels_gpu.py, run on an MI355X:

    python tests/golden/make_ref_kernels_golden.py [OUT.npz]      # default: tests/golden/reference_kernels.npz

Stored per NMS case: the keep mask, bit-packed (the contracted and un-contracted builds must agree).  Per ROIAlign case: the
SHA-256 of each build's float32 output, a seeded sample of the un-contracted output, and how many elements of the contracted
output differ at all / beyond compiler latitude (test_ref_kernels_gpu.roi_record).  Only outputs are stored; the inputs are
regenerated from seeds by the test module.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_ops                  # noqa: E402
import test_ref_kernels_gpu as T            # noqa: E402


def main(out):
    assert ref_ops.available('fma') and ref_ops.available('nofma'), 'oracle/_ref not built (python -m oracle.build)'
    dev = torch.device('cuda:0')
    g = {}
    for n, size in T.NMS_CASES:
        for thresh in T.NMS_THRESHES:
            t = torch.from_numpy(T.nms_inputs(n, size, thresh)).to(dev)
            keep = ref_ops.nms(t, thresh, 'fma').cpu().numpy()
            assert np.array_equal(ref_ops.nms(t, thresh, 'nofma').cpu().numpy(), keep)
            g[T.nms_key(n, size, thresh)] = T.nms_record(keep, n)
    for a in T.ROI_SIZES:
        for shape, scale in T.ROI_SHAPES:
            feat, rois = T.roi_inputs(a, shape)
            f, r = torch.from_numpy(feat).to(dev), torch.from_numpy(rois).to(dev)
            exact = ref_ops.roi_align_forward(f, r, a, a, scale, 'nofma').cpu().numpy()
            fma = ref_ops.roi_align_forward(f, r, a, a, scale, 'fma').cpu().numpy()
            g.update(T.roi_record(T.roi_key(a, shape), exact, fma))
    np.savez_compressed(out, **g)
    print('wrote %s: %d arrays, %d bytes' % (out, len(g), os.path.getsize(out)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'reference_kernels.npz'))
