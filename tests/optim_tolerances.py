"""Measured tolerances of tests/test_optim_gpu.py: twice the largest value seen on the MI355X (tests/tolerances.py's rule).

Only the comparison with torch.optim.SGD on the same device is here.  Everything else in the optimiser tests is either bit-equal
to the float32 restatement of tests/optim_ref.py or within the bound derived there for the norm's summation order.  torch's
device kernels may contract a + alpha * b into one fused multiply-add and scale the gradients in a pass of their own, the HIP
step rounds every operation once: after three steps the two differ by a few float32 roundings of the largest element.

Value: max |ours - torch| / max |torch| over the elements of a tensor, the largest over the test's tensors after three steps."""
LIMITS = {
    'optim_sgd_vs_torch_param': 2 * 7.762e-08,         # measured 7.762e-08
    'optim_sgd_vs_torch_momentum': 2 * 8.069e-07,      # measured 8.069e-07: the buffer is linear in the clip coefficient, and torch's
                                                       # norm (its own summation order) moves that by a float32 rounding or two
}
