/* libsrcnn_hip.so, fourth header of the C ABI: the optimiser step with gradient accumulation and a device-side guard against
 * non-finite gradients.
 *
 * An extension of srcnn_hip.h exactly as srcnn_train_weights.h and srcnn_train_fold.h are (types, error codes, srcnn_stream_t and
 * SRCNN_API are srcnn_hip.h's; stereo_rcnn_amd/_lib.py derives the binding from THIS file, _lib.EXTENSIONS); the other headers are
 * unchanged, and so are srcnn_grad_norm, srcnn_grad_scale and srcnn_sgd_step. */
#ifndef SRCNN_OPTIM_GUARD_H
#define SRCNN_OPTIM_GUARD_H

#include "srcnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------- training: optimiser step over accumulated gradients, skipped when not finite
 * srcnn_sgd_step forms g * coef; one Inf or NaN in any gradient makes the norm Inf or NaN, the coefficient 0 or NaN and the
 * product NaN on that element: parameter and momentum buffer are lost for good, and nothing reads the device to notice.  The pair
 * below is srcnn_grad_norm + srcnn_sgd_step with two additions: every gradient enters multiplied by the host float grad_scale
 * (1 / N after N backward passes have summed into .grad: the update of the mean gradient), and the update is predicated on a
 * DEVICE word that says whether the norm is finite.  Nothing is read back.
 *
 * Every convention is that of srcnn_hip.h, "training: optimiser step": HOST arrays of device pointers and long long numels, an
 * entry with numel 0 skipped, at most SRCNN_OPT_TENSORS_PER_LAUNCH tensors per launch, chunks of SRCNN_OPT_CHUNK elements, float4
 * where all pointers of a tensor are 16-byte aligned and single floats otherwise with the same arithmetic, every float32 operation
 * rounded once, no atomics, results independent of the grid and of alignment.
 *
 * srcnn_grad_norm_guarded: out is THREE device floats.
 *     x      = g * grad_scale                                   (one rounding per element, before the square)
 *     out[0] = sqrt(sum over every listed element of x * x)     srcnn_grad_norm's two stages in srcnn_grad_norm's order
 *     out[1] = clip_norm / max(out[0], clip_norm)               (1 where clip_norm is +infinity: "do not clip")
 *     out[2] = out[0] is finite ? 1.0f : 0.0f
 * With grad_scale == 1.0f, out[0] and out[1] carry srcnn_grad_norm's bits.  The squares and the per-chunk sums are float32, and
 * a float32 sum of squares is finite exactly when every term is finite and the sum did not overflow: out[2] is 0 for an Inf or a
 * NaN anywhere in the list AND for finite gradients whose squares (or a chunk's sum of them) overflow float32.  Such a step has no
 * usable norm, so it counts as a bad step too.  clip_norm: > 0, finite or +infinity.  workspace:
 * srcnn_grad_norm_workspace_bytes(n_tensors, numel_host) bytes.
 *
 * srcnn_sgd_step_guarded: ok is a device float, e.g. out + 2 of srcnn_grad_norm_guarded on the same stream; every workgroup loads
 * it once (a uniform value: no branch depends on a gradient's data).
 *   *ok != 0:  per element, in this order, every operation rounded once
 *                  g' = g * grad_scale
 *                  then srcnn_sgd_step's sequence on g' (d = clipped[i] && coef ? g' * *coef : g'; the weight decay; the momentum
 *                  buffer; p = p - lr[i] * m).
 *              With grad_scale == 1.0f, p and m carry srcnn_sgd_step's bits.
 *   *ok == 0:  no gradient is read and p is not written.  With first_step == 0, m is not written either.  With first_step != 0
 *              (the buffers are uninitialised), m is written as zeros: the next step, which is no first step any more, then
 *              computes momentum * 0 + d = d, which is what a first step would have stored (to the bit, but that a d of -0
 *              is stored as +0), so a freshly allocated buffer never keeps what the allocator left in it and the skipped step
 *              leaves no trace in the arithmetic.
 *   skipped:   NULL, or a device unsigned that counts the skipped steps: on a bad step one thread of the call's FIRST launch adds
 *              one with a plain load and store (a list longer than one launch still counts once; a list without elements
 *              launches nothing and counts nothing).  Do not share it between streams that run concurrently.
 * coef: NULL or a device float (out + 1).  clipped_host: NULL = every tensor is clipped.  Tensors must not overlap.
 *
 * Errors (SRCNN_ERR_ARG / SRCNN_ERR_WORKSPACE, before any launch): those of srcnn_grad_norm / srcnn_sgd_step; a grad_scale that
 * is not finite or <= 0; a clip_norm that is <= 0 or NaN; a null or misaligned ok; a misaligned skipped. */
SRCNN_API int srcnn_grad_norm_guarded(const float *const *g_host, const long long *numel_host, int n_tensors, float clip_norm,
                                      float grad_scale, float *out, void *workspace, size_t workspace_bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_sgd_step_guarded(float *const *p_host, const float *const *g_host, float *const *m_host, const long long *numel_host,
                                     const float *lr_host, const float *weight_decay_host, const int *clipped_host, int n_tensors,
                                     float momentum, int first_step, float grad_scale, const float *coef, const float *ok,
                                     unsigned *skipped, srcnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SRCNN_OPTIM_GUARD_H */
