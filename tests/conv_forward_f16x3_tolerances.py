"""Measured tolerances of tests/test_conv_forward_f16x3_gpu.py: the 3 x f16 training forward against float64 torch on the same
float32 inputs, max |err| / max |ref| of one case's output.  The project's rule: twice the largest value measured on an MI355X (the
tests report through tests/tolerances.py `observe`).  FP32 holds, for the reader, what the exact-fp32 engine gave for the same case
in the same run: the difference is what the split costs.

These limits hold ON TOP of the derived per-element bound (conv_forward_f16x3_ref.bound), the tests' first assertion; a name that
is missing here has not been measured yet and is held by the derived bound alone.
"""
MEASURED = {
    'conv_fwd_f16x3_channel_offset': 1.52e-07,
    'conv_fwd_f16x3_linear': 6.57e-08,
    'conv_fwd_f16x3_ragged_3x3': 1.61e-07,
    'conv_fwd_f16x3_residual_relu': 7.75e-08,
    'conv_fwd_f16x3_single_k_tile': 1.33e-07,
    'conv_fwd_f16x3_stride2_1x1': 9.79e-08,
    'conv_fwd_f16x3_stride2_3x3': 1.95e-07,
    'conv_fwd_f16x3_two_k_tiles_wide': 2.31e-07,
}                          # MI355X maxima, one run of the test file
FP32 = {
    'conv_fwd_f16x3_channel_offset': 3.18e-07,
    'conv_fwd_f16x3_linear': 2.25e-07,
    'conv_fwd_f16x3_ragged_3x3': 3.94e-07,
    'conv_fwd_f16x3_residual_relu': 1.72e-07,
    'conv_fwd_f16x3_single_k_tile': 2.12e-07,
    'conv_fwd_f16x3_stride2_1x1': 1.29e-07,
    'conv_fwd_f16x3_stride2_3x3': 2.52e-07,
    'conv_fwd_f16x3_two_k_tiles_wide': 3.37e-07,
}                              # the exact-fp32 engine, same cases, same run
LIMITS = {k: 2.0 * v for k, v in MEASURED.items()}          # twice the measured value
