"""numpy restatements of the optimiser step (include/srcnn_hip.h, "training: optimiser step"):
  * sgd_step_f32: torch.optim.SGD's update (dampening 0, no Nesterov) with the clip coefficient folded in, float32 with every
    operation rounded once and in the kernel's order -- what srcnn_sgd_step is compared with BIT FOR BIT;
  * sgd_step_f64: the same in float64;
  * clip_gradient_f64: the reference's clip_gradient (lib/model/utils/net_utils.py:37-49) in float64;
  * chunk_sums_f32, grad_norm_f32: the norm's two summation stages as the header defines them, float32 then float64 -- what
    srcnn_grad_norm (and, through tests/optim_guard_ref.py, srcnn_grad_norm_guarded) is compared with BIT FOR BIT;
  * norm_bound: the relative error bound of srcnn_grad_norm's float32 stage for the summation order the header states."""
import numpy as np

F32 = np.float32
CHUNK, THREADS, WAVE = 4096, 256, 64
_LANES = np.arange(WAVE)
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


def _butterfly(v):
    """The xor butterfly over the last axis (64 lanes), offsets 32 .. 1: lane 0's value.  Every lane ends with the same bits
    (a + b and b + a round alike)."""
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., _LANES ^ o]).astype(v.dtype)
    return v[..., 0]


def chunk_sums_f32(g, grad_scale=None):
    """Stage 1 of one tensor: the float32 sum of g^2 -- of (g * grad_scale)^2 where a scale is given -- of each of its chunks.
    Thread t owns the local elements 4 (256 j + t) + k and adds them in ascending (j, k) order from 0; elements past the end add
    nothing (here: + 0, which changes no bit of a sum that starts at + 0)."""
    g = np.asarray(g, F32).ravel()
    n_chunks = -(-g.size // CHUNK)
    x = np.zeros(n_chunks * CHUNK, F32)
    with np.errstate(all='ignore'):
        x[:g.size] = g if grad_scale is None else (g * F32(grad_scale)).astype(F32)
        sq = (x * x).astype(F32).reshape(n_chunks, CHUNK // (THREADS * 4), THREADS, 4)
        s = np.zeros((n_chunks, THREADS), F32)
        for j in range(sq.shape[1]):
            for k in range(4):
                s = (s + sq[:, j, :, k]).astype(F32)
        w = _butterfly(s.reshape(n_chunks, THREADS // WAVE, WAVE))
        return (((w[:, 0] + w[:, 1]).astype(F32) + w[:, 2]).astype(F32) + w[:, 3]).astype(F32)


def grad_norm_f32(grads, clip_norm, grad_scale=None):
    """(norm, coefficient) as float32 scalars.  grads: the list in list order (tensors without elements add no chunk).
    clip_norm +infinity (the guarded entry's "do not clip"): the coefficient is 1."""
    parts = [chunk_sums_f32(g, grad_scale) for g in grads if np.asarray(g).size]
    partial = np.concatenate(parts) if parts else np.zeros(0, F32)
    with np.errstate(all='ignore'):
        # stage 2, float64: thread t adds partial[t], partial[t + 256], .. in order from 0; butterfly; ((w0 + w1) + w2) + w3
        padded = np.zeros(-(-max(partial.size, 1) // THREADS) * THREADS, np.float64)
        padded[:partial.size] = partial
        s = np.zeros(THREADS, np.float64)
        for row in padded.reshape(-1, THREADS):
            s = s + row
        w = _butterfly(s.reshape(THREADS // WAVE, WAVE))
        norm = F32(np.sqrt(((w[0] + w[1]) + w[2]) + w[3]))
        clip = F32(clip_norm)
        coef = F32(1.0) if np.isinf(clip) else F32(clip / (norm if norm > clip else clip))
    return norm, coef


def norm_bound():
    """Relative bound on |kernel norm - float64 norm|.  Every term of the sum is non-negative, so each rounding a term passes
    through multiplies it by (1 + e), |e| <= 2^-24: the square and the thread's 16 sequential additions (at most 16 roundings:
    the first addition, to 0, is exact), 9 levels of the workgroup tree; stage 2 is in double.  The square root halves the
    relative error of the sum; + 2 covers the root's own rounding, the conversion to float32 and the second-order terms."""
    return (CHUNK_TERMS_PER_THREAD + TREE_LEVELS + 2) * 2.0 ** -24
