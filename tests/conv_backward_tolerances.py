"""Measured tolerances of tests/test_conv_backward_gpu.py and tests/test_autograd_conv_gpu.py: the convolution gradients
against float64 torch autograd on the same float32 inputs.  The project's rule: about twice the largest value measured on an
MI355X, the measured value beside it (the tests report through tests/tolerances.py `observe`, so a GPU session prints its maxima
at the end under the names below).  Every value is max |err| / max |ref| of one gradient tensor of one case.

These limits hold ON TOP of the derived per-element bound (conv_backward_ref.bound), which is the tests' first assertion; a
name that is missing here has not been measured yet and is held by the derived bound alone.
"""
MEASURED = {                          # MI355X maxima, one run of both test files
    'autograd_box_head_grad': 1.75e-06,
    'autograd_conv_dw': 3.02e-07,
    'autograd_conv_dx': 9.37e-07,
    'conv_bwd_channel_offset_db': 1.26e-07,
    'conv_bwd_channel_offset_dw': 5.08e-07,
    'conv_bwd_channel_offset_dx': 2.61e-06,
    'conv_bwd_cout24_db': 1.57e-07,
    'conv_bwd_cout24_dw': 4.59e-07,
    'conv_bwd_cout24_dx': 1.86e-07,
    'conv_bwd_linear_db': 4.60e-08,
    'conv_bwd_linear_dw': 6.32e-08,
    'conv_bwd_linear_dx': 1.60e-07,
    'conv_bwd_ragged_3x3_db': 1.09e-07,
    'conv_bwd_ragged_3x3_dw': 4.75e-07,
    'conv_bwd_ragged_3x3_dx': 1.42e-06,
    'conv_bwd_rcnn_top_db': 6.55e-08,
    'conv_bwd_rcnn_top_dw': 6.69e-08,
    'conv_bwd_rcnn_top_dx': 4.34e-07,
    'conv_bwd_single_k_tile_db': 7.17e-08,
    'conv_bwd_single_k_tile_dw': 2.43e-07,
    'conv_bwd_single_k_tile_dx': 1.83e-07,
    'conv_bwd_stride2_1x1_db': 1.17e-07,
    'conv_bwd_stride2_1x1_dw': 5.42e-07,
    'conv_bwd_stride2_1x1_dx': 2.37e-07,
    'conv_bwd_stride2_3x3_db': 1.15e-07,
    'conv_bwd_stride2_3x3_dw': 2.75e-07,
    'conv_bwd_stride2_3x3_dx': 5.03e-07,
}
LIMITS = {k: 2.0 * v for k, v in MEASURED.items()}          # twice the measured value
