"""numpy restatements of the guarded optimiser pair (include/srcnn_optim_guard.h), float32 with every operation rounded once and
in the kernels' order -- what srcnn_grad_norm_guarded and srcnn_sgd_step_guarded are compared with BIT FOR BIT:
  * grad_norm_guarded_f32: (norm, coefficient, ok) of a list of gradients, the two summation stages of include/srcnn_hip.h;
  * sgd_step_guarded_f32: one tensor's step under the word `ok`, optim_ref.sgd_step_f32 on g * grad_scale where it is set."""
import numpy as np

import optim_ref as R

F32 = np.float32
CHUNK, THREADS, WAVE = 4096, 256, 64
_LANES = np.arange(WAVE)


def _butterfly(v):
    """The xor butterfly over the last axis (64 lanes), offsets 32 .. 1: lane 0's value.  Every lane ends with the same bits
    (a + b and b + a round alike)."""
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., _LANES ^ o]).astype(v.dtype)
    return v[..., 0]


def chunk_sums_f32(g, grad_scale=1.0):
    """Stage 1 of one tensor: the float32 sum of (g * grad_scale)^2 of each of its chunks.  Thread t owns the local elements
    4 (256 j + t) + k and adds them in ascending (j, k) order from 0; elements past the end add nothing (here: + 0, which changes
    no bit of a sum that starts at + 0)."""
    g = np.asarray(g, F32).ravel()
    n_chunks = -(-g.size // CHUNK)
    x = np.zeros(n_chunks * CHUNK, F32)
    with np.errstate(all='ignore'):
        x[:g.size] = (g * F32(grad_scale)).astype(F32)
        sq = (x * x).astype(F32).reshape(n_chunks, CHUNK // (THREADS * 4), THREADS, 4)
        s = np.zeros((n_chunks, THREADS), F32)
        for j in range(sq.shape[1]):
            for k in range(4):
                s = (s + sq[:, j, :, k]).astype(F32)
        w = _butterfly(s.reshape(n_chunks, THREADS // WAVE, WAVE))
        return (((w[:, 0] + w[:, 1]).astype(F32) + w[:, 2]).astype(F32) + w[:, 3]).astype(F32)


def grad_norm_guarded_f32(grads, clip_norm, grad_scale=1.0):
    """(norm, coefficient, ok) as float32 scalars.  grads: the list in list order (tensors without elements add no chunk)."""
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
