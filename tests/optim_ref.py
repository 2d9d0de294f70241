"""numpy restatements of the optimiser step (include/srcnn_hip.h, "training: optimiser step"):
  * sgd_step_f32: torch.optim.SGD's update (dampening 0, no Nesterov) with the clip coefficient folded in, float32 with every
    operation rounded once and in the kernel's order -- what srcnn_sgd_step is compared with BIT FOR BIT;
  * sgd_step_f64: the same in float64;
  * clip_gradient_f64: the reference's clip_gradient (lib/model/utils/net_utils.py:37-49) in float64;
  * norm_bound: the relative error bound of srcnn_grad_norm's float32 stage for the summation order the header states."""
import numpy as np

F32 = np.float32
CHUNK_TERMS_PER_THREAD = 16     # a thread's sequential squares in one chunk (4 float4 groups)
TREE_LEVELS = 6 + 3             # 64-lane butterfly, then ((w0 + w1) + w2) + w3


def sgd_step_f32(p, g, m, lr, wd, momentum, first, coef=None):
    """One step on float32 arrays; returns (p_new, m_new).  m_new is None where momentum == 0; m is not read where `first`.
    coef: None (not clipped) or the float32 coefficient."""
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    lr, wd, momentum = F32(lr), F32(wd), F32(momentum)
    d = g if coef is None else (g * F32(coef)).astype(F32)
    if wd != 0:
        d = (d + (wd * p).astype(F32)).astype(F32)
    if momentum != 0:
        m_new = d.copy() if first else ((momentum * np.asarray(m, F32)).astype(F32) + d).astype(F32)
        d = m_new
    else:
        m_new = None
    return (p - (lr * d).astype(F32)).astype(F32), m_new


def sgd_step_f64(p, g, m, lr, wd, momentum, first, coef=None):
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    d = g if coef is None else g * float(coef)
    if wd != 0:
        d = d + wd * p
    if momentum != 0:
        m_new = d.copy() if first else momentum * np.asarray(m, np.float64) + d
        d = m_new
    else:
        m_new = None
    return p - lr * d, m_new


def clip_gradient_f64(grads, clip_norm):
    """net_utils.py:37-49: (total norm, coefficient, the scaled gradients) in float64."""
    total = 0.0
    for g in grads:
        total += float(np.sqrt(np.sum(np.asarray(g, np.float64) ** 2))) ** 2
    total = float(np.sqrt(total))
    coef = clip_norm / max(total, clip_norm)
    return total, coef, [np.asarray(g, np.float64) * coef for g in grads]


def norm_f64(grads):
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads)))


def norm_bound():
    """Relative bound on |kernel norm - float64 norm|.  Every term of the sum is non-negative, so each rounding a term passes
    through multiplies it by (1 + e), |e| <= 2^-24: the square and the thread's 16 sequential additions (at most 16 roundings:
    the first addition, to 0, is exact), 9 levels of the workgroup tree; stage 2 is in double.  The square root halves the
    relative error of the sum; + 2 covers the root's own rounding, the conversion to float32 and the second-order terms."""
    return (CHUNK_TERMS_PER_THREAD + TREE_LEVELS + 2) * 2.0 ** -24
