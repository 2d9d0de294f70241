"""Float tolerances of the GPU parity tests, in ONE place, next to what was measured.

Every bound below is about twice the largest value any `-m gpu` test observed on an MI355X in round 6 (the tests report their
observations through `observe`; tests/conftest.py writes them to gpurun_out/measured_tolerances.json at the end of a session and
profiles/measured_tolerances_r06.json is that file, committed).  Index outputs (NMS keep lists, proposal selection under identical
inputs, ROIAlign routing, dense-alignment argmin) are not here: they are exact or tie-audited.
"""
import json
import os

# north star: fp32 box / keypoint regressions within 1e-4 of the reference
REGRESSION = 1e-4

# --- about twice the measured maxima (profiles/measured_tolerances_r06.json: 396 GPU tests, one MI355X box)
# proposal layer fed the oracle's own probs / deltas: decoded corners differ by expf vs torch's CPU exp, one float32 ulp of the
# coordinate (measured 3.1e-5 = ulp at 256-512 px; the bound is two ulps at the 1987-px image width)
PROPOSAL_ISOLATED_PX = 2.5e-4
# end to end: distance between a reference proposal and the HIP proposal matched to it (measured 8.9e-4: the RPN deltas carry the
# trunk's accumulation-order differences through exp(dw) * w on boxes hundreds of pixels wide)
PROPOSAL_MATCH_PX = 2e-3
# end to end: head probabilities on matched proposals -- they move with the proposals (measured: kpts_prob 1.7e-4, right border
# 1.5e-4, the others <= 3.2e-5; bbox_pred / dim_orien_pred 2.5e-5 / 2.8e-5 against REGRESSION).  The same heads fed the REFERENCE's
# proposals are held to REGRESSION (test_heads_fed_the_reference_rois_full_size)
HEAD_OUTPUT_E2E = 4e-4
# decode + class NMS kernels on the reference network's outputs vs the reference's demo.py code (bbox_transform.py:92-104): one
# float32 ulp of a coordinate near 1000 px (measured 1.22e-4 = 2^-13); two ulps
DECODED_PX = 2.5e-4

# KITTI evaluation: device BEV / 3-D IoU against exact rational arithmetic (kitti_eval_ref.bev_intersection_exact) on the
# near-degenerate sweep of kitti_synth.bev_sweep, per distance band.  Not twice a device maximum like the rest of this table but
# FOUR TIMES the worst deviation of the float64 vertex-set reference (kitti_eval_ref.bev_intersection) from exact arithmetic
# over the same pairs, measured on the CPU and held there by test_kitti_eval_crowded_cpu.py: a correct float64 evaluation of
# the same area cannot be asked to beat another one by much, a lost vertex costs orders of magnitude more.
#   reference vs exact, measured: near (z <= 80 m) 1.63e-11, far (z ~ 500 m) 1.79e-11
#   device vs exact on an MI355X, measured: near 2.7e-12, far 9.7e-12 (bev(d, g) - bev(g, d): 3.1e-12, 1.4e-11)
KITTI_BEV_EXACT = {'near': 6.6e-11, 'far': 7.2e-11}
KITTI_BEV_REFERENCE_MEASURED = {'near': 1.63e-11, 'far': 1.79e-11}

# Dense-alignment stages (tests/test_dense_align_stages_gpu.py) against the float64 references of tests/dense_align_ref.py, on
# the scenes of tests/dense_align_scenes.py.  As for KITTI_BEV_EXACT: FOUR TIMES the largest deviation of the float32 ORACLE
# (oracle/dense_align.py on the CPU) from the float64 reference over the same scenes, measured and held by
# tests/test_dense_align_ref_cpu.py -- a correct float32 evaluation cannot be asked to beat another one by much.
#   DZ:  the depth offset of a lattice pixel's ray / box intersection (uvz[:, 2], metres)
#   TAP: a left-image tap at a lattice point (grey levels of the mean-subtracted network input; the float32 `unnorm` round trip
#        moves the tap coordinate by some 1e-5 px, which the image gradient turns into this)
#   oracle vs float64, measured on the CPU: dz 4.42e-6 m (objects at 3..25 m), taps 1.61e-4 (values up to 150)
DENSE_ALIGN_DZ_REFERENCE_MEASURED = 4.5e-6
DENSE_ALIGN_TAP_REFERENCE_MEASURED = 1.61e-4
DENSE_ALIGN_DZ = 4 * DENSE_ALIGN_DZ_REFERENCE_MEASURED
DENSE_ALIGN_TAP = 4 * DENSE_ALIGN_TAP_REFERENCE_MEASURED

_measured = {}


def observe(name, value):
    """Remember the largest value seen under `name` (reported at the end of the session); returns the value."""
    v = float(value)
    if name not in _measured or v > _measured[name]:
        _measured[name] = v
    return v


def measured():
    return dict(_measured)


def dump(path):
    if _measured:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, 'w') as f:
            json.dump({k: _measured[k] for k in sorted(_measured)}, f, indent=1)
