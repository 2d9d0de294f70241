/* libsrcnn_hip.so, third header of the C ABI: the training weights folded and re-laid-out on the device, with the adjoint.
 *
 * An extension of srcnn_hip.h exactly as srcnn_train_weights.h is one (types, error codes, srcnn_stream_t and SRCNN_API are
 * srcnn_hip.h's; stereo_rcnn_amd/_lib.py derives the binding from THIS file, _lib.EXTENSIONS); both other headers are unchanged. */
#ifndef SRCNN_TRAIN_FOLD_H
#define SRCNN_TRAIN_FOLD_H

#include "srcnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------- training: frozen-BN fold + engine layout of every weight, both directions
 * What feeds srcnn_train_weights_prepare: every layer's parameter (as nn.Conv2d / nn.Linear / nn.ConvTranspose2d hold it), with
 * its frozen BatchNorm folded in, written in the conv engine's layout (Cout, KH, KW, Cin) -- and, on the way back, the gradient of
 * that folded tensor carried to the parameter.  The arithmetic is stereo_rcnn_amd.autograd._fold's, operation for operation, so
 * the results carry the bits of the eager torch path (float64, one rounding per operation, never an FMA):
 *   forward   s = (double)gamma / sqrt((double)var + 1e-5);  w' = (float)((double)w * s);
 *             b' = (float)((double)beta - (double)mean * s)                    without a convolution bias,
 *             b' = (float)((double)bias * s + ((double)beta - (double)mean * s))   with one;
 *   backward  dw = (float)((double)dw' * s);  db = (float)((double)db' * s);  the BN tensors receive nothing;
 *   without a BN both directions move data and compute nothing.
 *
 * srcnn_train_fold_desc, one layer (field order: w[3], bias[3], grad_w[3], grad_b[3], bn_weight, bn_bias, bn_mean, bn_var, dst_w,
 * dst_b, rows[3], n_parts, kind, Cout, KH, KW, Cin):
 *   n_parts 1..3 source parts, concatenated along the output rows (rpn_head is two, box_heads three): part p is the parameter
 *           w[p] with rows[p] output rows and its optional bias[p] (all parts carry one, or none does); the rows sum to Cout;
 *   kind    SRCNN_TRAIN_FOLD_CONV       part (rows, Cin, KH, KW) -> dst_w (Cout, KH, KW, Cin) (RCNN_top.0's (2048, 512, 7, 7) ->
 *                                       (2048, 1, 1, 49 * 512) is this kind: the same memory);
 *           SRCNN_TRAIN_FOLD_LINEAR     part (rows, Cin) -> dst_w (Cout, 1, 1, Cin), a copy; KH = KW = 1;
 *           SRCNN_TRAIN_FOLD_DECONV2X2  one part (Cin, Cout, 2, 2) -> dst_w (4 Cout, 1, 1, Cin), row (i, j, co) = (2 i + j) Cout + co;
 *                                       KH = KW = 2, rows[0] = Cout; dst_b (4 Cout) is bias four times;
 *   bn_*    the frozen BatchNorm's weight, bias, running_mean, running_var (Cout floats each): all four or none; one part only;
 *   dst_w, dst_b   the folded weight and bias.  dst_b is required with a BN or a bias and must be NULL otherwise;
 *   grad_w[p], grad_b[p]   (backward only) receive the gradient of part p in the PARAMETER's own contiguous layout.
 * Cin is a multiple of 32, KH KW <= 128; w[p], dst_w, grad_w[p] and the dw_folded entries are 16-byte aligned (vector loads and
 * stores), every other pointer 4-byte.
 *
 * srcnn_train_weights_fold writes dst_w and dst_b of every layer.
 * srcnn_train_weights_fold_backward takes dw_folded_host[i] / db_folded_host[i], the gradients of layer i's dst_w / dst_b (HOST
 * arrays of n device pointers, the arrays themselves may not be NULL).  A NULL dw entry skips the layer's weights, a NULL db
 * entry its biases: nothing of theirs is written (a layer with both NULL costs no work).  db of a layer without a convolution
 * bias reaches no parameter and is ignored.  THE DECONVOLUTION'S BIAS STAYS EAGER: its adjoint is the sum of four floats whose
 * order torch.Tensor.repeat's backward does not document, so the entry refuses a non-NULL db_folded_host[i] for a DECONV2X2
 * layer and the caller keeps `bias.repeat(4)` (256 floats) as a torch operator; the forward's copy is exact and is done here.
 *
 * Conventions are srcnn_train_weights_prepare's.  `layers_host` is a HOST array; it travels in kernel-argument blocks,
 * SRCNN_TRAIN_FOLD_LAYERS_PER_BLOCK layers per block, into a table in the workspace (srcnn_train_fold_workspace_bytes(n) = n
 * records of 144 bytes rounded up to 256; 0 for n < 1).  Launches, one stream, in order: per block of layers one small launch
 * that writes their table rows, then ONE launch that does all the work.  Its unit is R output rows x C input channels (all taps)
 * with R C KH KW <= 4096 floats, found by a binary search over the table's running unit counts (RCNN_top.0 is 16384 units, a
 * (24, 512) head three): the unit is read in the source's order, staged in LDS, and written in the destination's order, so both
 * sides move as contiguous 16-byte runs (parameter side: C KH KW floats of a row; engine side: per tap C floats).
 * No host read, no device-scope fence, no atomics; every destination element is written exactly once (pass uninitialised
 * buffers); the same bits on every run.
 * Errors, before any launch (nothing is written): a null list / workspace / gradient array, n_layers < 1, "layer i: ..." for a
 * null or misaligned pointer, n_parts outside 1..3, non-positive sizes, Cin not a multiple of 32, rows not summing to Cout, an
 * unknown kind, a BN over several parts or given in part, a bias on some parts only, dst_b not matching, a layer of 2^31 elements
 * or more (SRCNN_ERR_ARG); a workspace smaller than the query's (SRCNN_ERR_WORKSPACE). */
#define SRCNN_TRAIN_FOLD_CONV 0
#define SRCNN_TRAIN_FOLD_LINEAR 1
#define SRCNN_TRAIN_FOLD_DECONV2X2 2
#define SRCNN_TRAIN_FOLD_LAYERS_PER_BLOCK 24
typedef struct srcnn_train_fold_desc {
    const float *w[3];
    const float *bias[3];
    float *grad_w[3];
    float *grad_b[3];
    const float *bn_weight, *bn_bias, *bn_mean, *bn_var;
    float *dst_w, *dst_b;
    int rows[3];
    int n_parts, kind, Cout, KH, KW, Cin;
} srcnn_train_fold_desc;
SRCNN_API size_t srcnn_train_fold_workspace_bytes(int n_layers);
SRCNN_API int srcnn_train_weights_fold(const srcnn_train_fold_desc *layers_host, int n_layers, void *workspace, size_t workspace_bytes,
                                       srcnn_stream_t stream);
SRCNN_API int srcnn_train_weights_fold_backward(const srcnn_train_fold_desc *layers_host, int n_layers,
                                                const float *const *dw_folded_host, const float *const *db_folded_host,
                                                void *workspace, size_t workspace_bytes, srcnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SRCNN_TRAIN_FOLD_H */
