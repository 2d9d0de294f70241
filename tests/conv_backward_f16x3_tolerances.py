"""Measured tolerances of tests/test_conv_backward_f16x3_gpu.py: the 3 x f16 convolution gradients against float64 torch
autograd on the same float32 inputs, max |err| / max |ref| of one gradient tensor of one case.  The project's rule: twice the
largest value measured on an MI355X (the tests report through tests/tolerances.py `observe`).  FP32 holds, for the reader, what the
exact-fp32 backward gave for the same case in the same run: the difference is what the split costs.

These limits hold ON TOP of the derived per-element bound (conv_backward_f16x3_ref.bound), the tests' first assertion; a name
that is missing here has not been measured yet and is held by the derived bound alone.
"""
MEASURED = {
    'conv_bwd_f16x3_channel_offset_db': 1.28e-07,
    'conv_bwd_f16x3_channel_offset_dw': 1.14e-07,
    'conv_bwd_f16x3_channel_offset_dx': 1.67e-07,
    'conv_bwd_f16x3_forced_split_db': 8.44e-08,
    'conv_bwd_f16x3_forced_split_dw': 1.97e-07,
    'conv_bwd_f16x3_forced_split_dx': 4.43e-07,
    'conv_bwd_f16x3_linear_db': 3.68e-08,
    'conv_bwd_f16x3_linear_dw': 1.70e-07,
    'conv_bwd_f16x3_linear_dx': 1.06e-07,
    'conv_bwd_f16x3_ragged_3x3_db': 9.92e-08,
    'conv_bwd_f16x3_ragged_3x3_dw': 1.64e-07,
    'conv_bwd_f16x3_ragged_3x3_dx': 1.84e-07,
    'conv_bwd_f16x3_single_k_tile_db': 9.01e-08,
    'conv_bwd_f16x3_single_k_tile_dw': 1.45e-07,
    'conv_bwd_f16x3_single_k_tile_dx': 1.01e-07,
    'conv_bwd_f16x3_stride2_1x1_db': 5.93e-08,
    'conv_bwd_f16x3_stride2_1x1_dw': 1.27e-07,
    'conv_bwd_f16x3_stride2_1x1_dx': 1.01e-07,
    'conv_bwd_f16x3_stride2_3x3_db': 1.04e-07,
    'conv_bwd_f16x3_stride2_3x3_dw': 1.80e-07,
    'conv_bwd_f16x3_stride2_3x3_dx': 1.31e-07,
}                          # MI355X maxima, one run of the test file
FP32 = {
    'conv_bwd_f16x3_channel_offset_db': 1.28e-07,
    'conv_bwd_f16x3_channel_offset_dw': 1.45e-07,
    'conv_bwd_f16x3_channel_offset_dx': 3.53e-07,
    'conv_bwd_f16x3_forced_split_db': 8.44e-08,
    'conv_bwd_f16x3_forced_split_dw': 4.94e-07,
    'conv_bwd_f16x3_forced_split_dx': 8.96e-07,
    'conv_bwd_f16x3_linear_db': 3.68e-08,
    'conv_bwd_f16x3_linear_dw': 1.03e-07,
    'conv_bwd_f16x3_linear_dx': 1.84e-07,
    'conv_bwd_f16x3_ragged_3x3_db': 9.92e-08,
    'conv_bwd_f16x3_ragged_3x3_dw': 2.55e-07,
    'conv_bwd_f16x3_ragged_3x3_dx': 4.68e-07,
    'conv_bwd_f16x3_single_k_tile_db': 9.01e-08,
    'conv_bwd_f16x3_single_k_tile_dw': 1.08e-07,
    'conv_bwd_f16x3_single_k_tile_dx': 1.58e-07,
    'conv_bwd_f16x3_stride2_1x1_db': 5.93e-08,
    'conv_bwd_f16x3_stride2_1x1_dw': 1.79e-07,
    'conv_bwd_f16x3_stride2_1x1_dx': 2.06e-07,
    'conv_bwd_f16x3_stride2_3x3_db': 1.04e-07,
    'conv_bwd_f16x3_stride2_3x3_dw': 1.22e-07,
    'conv_bwd_f16x3_stride2_3x3_dx': 3.52e-07,
}                              # the exact-fp32 backward, same cases, same run
LIMITS = {k: 2.0 * v for k, v in MEASURED.items()}          # twice the measured value
