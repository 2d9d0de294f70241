/* libsrcnn_hip.so, second header of the C ABI: the f16x3 training weights prepared once per optimiser step.
 *
 * An extension of srcnn_hip.h (types, error codes, srcnn_stream_t and SRCNN_API are its): the four entries below live in the same
 * library and follow the same conventions -- device pointers, validation before the first launch, the reason of a refusal in
 * srcnn_last_error().  stereo_rcnn_amd/_lib.py derives their binding from THIS file as it derives the others from srcnn_hip.h
 * (_lib.EXTENSIONS); srcnn_hip.h itself is unchanged by it. */
#ifndef SRCNN_TRAIN_WEIGHTS_H
#define SRCNN_TRAIN_WEIGHTS_H

#include "srcnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------- 3 x f16 training calls: weights prepared once per step
 * max|w| and the split of w are functions of the weights alone, and the weights change only in the optimiser step: what every
 * srcnn_conv2d_forward_f16x3 call (clear, max|w|, split) and every srcnn_conv2d_backward_f16x3 call (clear, max|w|, re-layout +
 * split) computes for itself can be computed once per step for ALL layers.  srcnn_train_weights_prepare does that for a list; the
 * two *_prepared entries are the *_maxima entries reading its results.  Every result keeps the bits of the plain entries.
 *
 * srcnn_train_weight_desc, one layer (field order: w, w_amax, w_hi, w_lo, wt_hi, wt_lo, Cout, KH, KW, Cin):
 *   w       the folded fp32 weight in engine layout (Cout, KH, KW, Cin), 16-byte aligned, Cin a multiple of 32;
 *   w_amax  one word (4-byte aligned) that receives the float bits of max|w| (0 for an all-zero weight);
 *   w_hi, w_lo    the forward planes (Cp, KH KW, Cin) float16, Cp = Cout rounded up to 32, rows [Cout, Cp) zero -- what the plain
 *                 forward's split writes into its workspace;
 *   wt_hi, wt_lo  the backward planes (Cin, KH KW, Cp) float16, element (c, tap, n) = split(w[n][tap][c]), columns [Cout, Cp) zero --
 *                 what the plain backward's re-layout + split writes.  All four planes 16-byte aligned, Cp KH KW Cin halves each.
 *   t = s w, hi = f16(t), lo = f16(t - hi), s = 2^(14 - floor(log2 max|w|)) with the exponent clamped to +-126 (an all-zero weight:
 *   s = 2^126, exact-zero planes).
 * `layers_host` is a HOST array.  It travels in kernel-argument blocks, 48 layers per block, into a
 * table in the workspace (srcnn_train_weights_workspace_bytes(n) = n records of 80 bytes, rounded up to
 * 256; 0 for n < 1): nothing is copied by the host runtime, nothing is read back.  Launches, one stream, in order:
 *   (1) per 48 layers one small launch that writes their table rows and clears their words;
 *   (2) ONE launch over the whole list that finds every layer's max|w|: a layer is cut into chunks of 8192 floats, a workgroup takes
 *       one chunk and finds its layer by a binary search over the table's running chunk counts; one integer atomicMax on the float
 *       bits per wave (order-independent).  A clear and an atomicMax on the same word cannot share a launch without a device-scope
 *       fence, which is why (1) clears;
 *   (3) ONE launch that writes every layer's four planes: the unit of work is 32 rows of w x up to 8 K tiles (a K tile = 32 channels
 *       of one tap), found by the same search, so RCNN_top's (2048, 7, 7, 256) is thousands of units and a (24, 1, 1, 512) head
 *       two.  Per K tile the 32 x 32 floats are read as one float4 per thread, split, parked in LDS as halves, and leave as
 *       16-byte runs on both sides: 8 channels of a row for w_hi / w_lo, 8 rows of a channel (read transposed from LDS) for wt_*.
 * So a list of up to 48 layers takes three launches and every further block of that many one more.
 * No host read, no device-scope fence, no float atomics; every plane element is written exactly once (pass uninitialised buffers).
 * Errors, before any launch (nothing is written): a null list / workspace, n_layers < 1, "layer i: ..." for a null or misaligned
 * pointer, non-positive sizes, Cin not a multiple of 32 or a layer of 2^31 elements or more (SRCNN_ERR_ARG); a workspace smaller
 * than the query's (SRCNN_ERR_WORKSPACE).
 *
 * srcnn_conv2d_forward_f16x3_prepared: srcnn_conv2d_forward_f16x3_maxima (same descriptor, x_amax, y_amax, validation, workspace
 *   query) with w_amax, w_hi, w_lo of the layer as srcnn_train_weights_prepare left them and plane_bytes, the bytes each plane
 *   holds.  Neither the scan of w nor the split is launched; the clear launch zeroes the max|x| word only when the call scans x
 *   itself, copies *w_amax into the workspace word the GEMM reads s_w from, and clears y_amax.  The GEMM kernel is the same.
 * srcnn_conv2d_backward_f16x3_prepared: srcnn_conv2d_backward_f16x3_maxima likewise with w_amax, wt_hi, wt_lo; the three may be
 *   NULL when dx is not asked for (the weight gradient reads no weights).
 *   Additional refusals, before any launch: a null word or plane ("null"), a word not 4-byte or a plane not 16-byte aligned
 *   ("aligned"), plane_bytes below Cp KH KW Cin halves ("plane_bytes"). */
typedef struct srcnn_train_weight_desc {
    const float *w;
    unsigned *w_amax;
    void *w_hi, *w_lo;
    void *wt_hi, *wt_lo;
    int Cout, KH, KW, Cin;
} srcnn_train_weight_desc;
SRCNN_API size_t srcnn_train_weights_workspace_bytes(int n_layers);
SRCNN_API int srcnn_train_weights_prepare(const srcnn_train_weight_desc *layers_host, int n_layers, void *workspace,
                                          size_t workspace_bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_conv2d_forward_f16x3_prepared(const srcnn_conv_fwd_f16x3_desc *d, const unsigned *x_amax, unsigned *y_amax,
                                                  const unsigned *w_amax, const void *w_hi, const void *w_lo, size_t plane_bytes,
                                                  void *workspace, size_t workspace_bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_conv2d_backward_f16x3_prepared(const srcnn_conv_bwd_desc *d, const unsigned *x_amax, const unsigned *w_amax,
                                                   const void *wt_hi, const void *wt_lo, size_t plane_bytes, void *workspace,
                                                   size_t workspace_bytes, srcnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SRCNN_TRAIN_WEIGHTS_H */
