"""Tolerances of tests/test_losses_gpu.py: the fused loss kernels against the float64 restatement (tests/losses_ref.py) on the
same float32 inputs.  The project's rule: about twice the largest value measured on an MI355X, the measured value written next
to each entry (the tests report through tests/tolerances.py `observe`, so a GPU session prints its
maxima at the end under the names below).

Loss values: relative error.  Gradients: largest absolute error of the case divided by the largest reference gradient magnitude
of the case.  u = 2^-24.
"""
import math

U = 2.0 ** -24

MEASURED = {                          # MI355X maxima over all cases of the test file
    'loss_ce_value_rel': 1.34e-07,
    'loss_ce_grad': 1.74e-07,
    'loss_smooth_l1_value_rel': 1.21e-07,
    'loss_smooth_l1_grad': 1.54e-07,
    'loss_module_value_rel': 6.78e-08,
    'loss_module_grad': 1.70e-07,
}
CE_VALUE_REL = 2.7e-07          # measured 1.34e-07
CE_GRAD = 3.5e-07               # measured 1.74e-07
SMOOTH_L1_VALUE_REL = 2.5e-07   # measured 1.21e-07
SMOOTH_L1_GRAD = 3.1e-07        # measured 1.54e-07
MODULE_VALUE_REL = 1.4e-07      # measured 6.78e-08
MODULE_GRAD = 3.4e-07           # measured 1.70e-07


def value_ceiling(elements):
    """Derived ceiling on top of the table.  Every term of a loss sum is non-negative and the sum is a tree (four terms per lane,
    a 64-lane butterfly, four wavefronts, then the same over the workgroups' partials: include/srcnn_hip.h), so its depth is
    about log2(elements) and each level costs at most one u of relative error; 8 u cover the terms themselves (exp, log1p, the
    products) and the final division.  A measured error above this means the summation is not what the header says."""
    return (math.log2(max(int(elements), 2)) + 8.0) * U
