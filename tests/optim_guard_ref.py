"""numpy restatements of the guarded optimiser pair (include/srcnn_hip.h), float32 with every operation rounded once and
in the kernels' order -- what srcnn_grad_norm_guarded and srcnn_sgd_step_guarded are compared with BIT FOR BIT:
  * grad_norm_guarded_f32: (norm, coefficient, ok) of a list of gradients, the two summation stages of optim_ref.grad_norm_f32
    on g * grad_scale;
  * sgd_step_guarded_f32: one tensor's step under the word `ok`, optim_ref.sgd_step_f32 on g * grad_scale where it is set."""
import numpy as np

import optim_ref as R

F32 = np.float32


def grad_norm_guarded_f32(grads, clip_norm, grad_scale=1.0):
    """(norm, coefficient, ok) as float32 scalars: optim_ref.grad_norm_f32 on g * grad_scale (one rounding) and the third word."""
    norm, coef = R.grad_norm_f32(grads, clip_norm, grad_scale)
    return norm, coef, F32(1.0 if np.isfinite(norm) else 0.0)


def sgd_step_guarded_f32(p, g, m, lr, wd, momentum, first, grad_scale, ok, coef=None):
    """One tensor's guarded step; returns (p_new, m_new).  ok != 0: optim_ref.sgd_step_f32 on g' = g * grad_scale (one rounding,
    first).  ok == 0: p as it is; m as it is, or zeros where `first` (m is then not read); None where momentum == 0."""
    p = np.asarray(p, F32)
    if ok != 0:
        with np.errstate(all='ignore'):
            return R.sgd_step_f32(p, (np.asarray(g, F32) * F32(grad_scale)).astype(F32), m, lr, wd, momentum, first, coef)
    if momentum == 0:
        return p.copy(), None
    return p.copy(), (np.zeros_like(p) if first else np.asarray(m, F32).copy())
