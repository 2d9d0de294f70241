"""GPU: the REFERENCE'S OWN CUDA kernels (oracle/_ref, built unchanged for gfx950 by oracle/build.py:build_ref) against
the C restatement of the oracle and against the product's HIP kernels, on the MI355X.  This is the pin for the two
native operators: the same source the reference compiles with nvcc, executed here.

The reference sources are not part of this repository, so oracle/_ref exists only where they could be compiled.  The results of
those builds on these very inputs are stored in tests/golden/reference_kernels.npz (recorded on an MI355X by
tests/golden/make_ref_kernels_golden.py), compactly: an NMS result as its keep mask (the kernel keeps indices in ascending
order), a ROIAlign result as the SHA-256 of its float32 bytes plus a seeded sample of its values, and the contracted build's
deviation from the un-contracted one as counts.  Every test compares against the stored results, bit for bit, and where
oracle/_ref exists it also runs the reference's kernels live and requires them to reproduce the stored results."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_kernels.npz')
NMS_CASES = [(1, 50), (64, 80), (65, 80), (1000, 60), (6000, 40), (6000, 150), (4097, 300)]
NMS_THRESHES = [0.7, 0.3]
ROI_SIZES = [8, 15]
ROI_SHAPES = [((1, 8, 38, 125), 1 / 16.), ((2, 16, 19, 63), 1 / 32.), ((1, 4, 150, 497), 1 / 4.)]


def nms_key(n, size, thresh):
    return 'nms_%d_%d_%g' % (n, size, thresh)


def roi_key(a, shape):
    return 'roi_align_%d_%s' % (a, 'x'.join(str(v) for v in shape))


def _boxes(n, seed, size):
    g = np.random.default_rng(seed)
    cx, cy = g.uniform(0, 1987, n), g.uniform(0, 600, n)
    w, h = size * g.uniform(0.5, 1.5, n), size * g.uniform(0.5, 1.5, n)
    d = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, np.sort(g.uniform(0, 1, n))[::-1]], 1).astype(np.float32)
    d[::7, :4] = np.round(d[::7, :4])            # integer coordinates: exact IoU ties around the threshold
    return d


def nms_inputs(n, size, thresh):
    return _boxes(n, n + int(100 * thresh), size)


def roi_inputs(a, shape):
    g = np.random.default_rng(a + shape[2])
    feat = g.standard_normal(shape).astype(np.float32)
    n = 60
    x1, y1 = g.uniform(-20, 1900, n), g.uniform(-20, 560, n)
    rois = np.stack([g.integers(0, shape[0], n), x1, y1, x1 + g.uniform(1, 400, n), y1 + g.uniform(1, 200, n)], 1).astype(np.float32)
    rois[0, 1:] = [10, 10, 10, 10]                      # degenerate roi
    rois[1, 1:] = [1980, 590, 2100, 700]                # hanging over the border -> zero taps
    return feat, rois


def digest(a):
    """SHA-256 of a float32 array's bytes (C order) as 32 uint8"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).digest(), np.uint8)


def sample_positions(numel, k=512):
    """fixed positions of the stored value sample (diagnostics when a digest differs)"""
    return np.random.default_rng(numel).integers(0, numel, size=min(k, numel))


def fma_close(fma, exact):
    """elementwise: the contracted build within compiler latitude of the un-contracted one (see the ROIAlign test)"""
    return np.isclose(fma, exact, rtol=2e-5, atol=2e-4)


def nms_record(keep, n):
    """stored form of an NMS result: the keep mask over the n boxes, bit-packed"""
    mask = np.zeros(n, bool)
    mask[keep] = True
    assert np.array_equal(np.flatnonzero(mask), keep), 'keep list not ascending'
    return np.packbits(mask)


def nms_from_golden(g, key, n):
    return np.flatnonzero(np.unpackbits(g[key], count=n)).astype(np.int32)


def roi_record(key, exact, fma):
    """stored form of a ROIAlign case: digests of both builds, a sample of the un-contracted output, deviation counts"""
    close = fma_close(fma, exact)
    return {key + '_sha256': digest(exact), key + '_sample': exact.reshape(-1)[sample_positions(exact.size)],
            key + '_fma_sha256': digest(fma), key + '_fma_counts': np.array([int((fma != exact).sum()), int((~close).sum())], np.int64)}


def assert_same(got, golden, key, what):
    """got (float32) bit-equal to the stored result `key`"""
    if not np.array_equal(digest(got), golden[key + '_sha256']):
        smp = got.reshape(-1)[sample_positions(got.size)]
        raise AssertionError('%s differs from the reference kernel (%s): max |diff| on the stored sample %.3e'
                             % (what, key, float(np.abs(smp - golden[key + '_sample']).max())))


@pytest.fixture(scope='module')
def ref():
    """(stored results, oracle.ref_ops or None where oracle/_ref was not built)"""
    from oracle import ref_ops
    assert os.path.exists(GOLDEN), GOLDEN
    live = ref_ops if (ref_ops.available('fma') and ref_ops.available('nofma')) else None
    return np.load(GOLDEN), live


@pytest.mark.parametrize("n,size", NMS_CASES)
@pytest.mark.parametrize("thresh", NMS_THRESHES)
def test_reference_nms_kernel_vs_oracle_and_product(dev, ref, n, size, thresh):
    from oracle import ops as oops
    from stereo_rcnn_amd.model.nms.nms_gpu import nms_gpu
    golden, live = ref
    d = nms_inputs(n, size, thresh)
    t = torch.from_numpy(d).to(dev)
    want = nms_from_golden(golden, nms_key(n, size, thresh), n)
    if live is not None:
        assert np.array_equal(live.nms(t, thresh, 'fma').cpu().numpy(), want)
        assert np.array_equal(live.nms(t, thresh, 'nofma').cpu().numpy(), want)     # devIoU has no multiply-add to contract
    assert np.array_equal(np.asarray(oops.nms(d, thresh), dtype=np.int32), want)           # C restatement
    assert np.array_equal(nms_gpu(t, thresh).view(-1).cpu().numpy(), want)                 # product kernel


@pytest.mark.parametrize("a", ROI_SIZES)
@pytest.mark.parametrize("shape,scale", ROI_SHAPES)
def test_reference_roi_align_kernel_vs_oracle_and_product(dev, ref, a, shape, scale):
    from oracle import ops as oops
    from stereo_rcnn_amd.model.roi_align.functions.roi_align import RoIAlignFunction
    golden, live = ref
    feat, rois = roi_inputs(a, shape)
    f, r = torch.from_numpy(feat).to(dev), torch.from_numpy(rois).to(dev)
    key = roi_key(a, shape)
    counts = golden[key + '_fma_counts']
    if live is not None:
        exact = live.roi_align_forward(f, r, a, a, scale, 'nofma').cpu().numpy()
        assert_same(exact, golden, key, 'the un-contracted reference build')
        fma = live.roi_align_forward(f, r, a, a, scale, 'fma').cpu().numpy()
        assert np.array_equal(digest(fma), golden[key + '_fma_sha256'])
        close = fma_close(fma, exact)
        assert [int((fma != exact).sum()), int((~close).sum())] == counts.tolist()
    # restatement and product are built without floating-point contraction: bit-equal to the reference kernel built the same way
    assert_same(oops.roi_align_forward(feat, rois, a, a, scale), golden, key, 'the C restatement')
    got = RoIAlignFunction(a, a, scale)(f, r).cpu().numpy()
    assert_same(got, golden, key, 'the product kernel')
    # the same source with floating-point contraction allowed (what nvcc's default -fmad=true does to `ph * bin + start` and
    # to the blend): the lattice coordinate moves by <= 1 float ulp, the sample by ~1e-6 relative -- compiler latitude, far
    # inside every tolerance; the restatements follow the un-contracted source semantics
    # one ulp of a coordinate near 500 is 3e-5 of a pixel; the test maps are white noise (unit gradient per pixel)
    # (a coordinate that lands exactly on a lattice line or on the map border can flip floor() / the zero test by that ulp)
    assert 1.0 - float(counts[1]) / got.size > 0.99
    print('contracted vs un-contracted reference build: %d of %d elements differ at all, %d beyond 2e-4'
          % (int(counts[0]), got.size, int(counts[1])))
