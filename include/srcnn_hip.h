/*
 * srcnn_hip.h -- flat C ABI of libsrcnn_hip.so, the MI355X (gfx950) native
 * replacement for the Stereo R-CNN inference hot path.
 *
 * This is the drop-in boundary.  The reference crosses it with cffi
 * (torch.utils.ffi) into two CUDA extensions; every entry point below names the
 * reference interface it replaces (paths relative to /root/reference).
 *
 * Conventions:
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless
 *     the name ends in _host; no torch types;
 *   - the caller allocates every output and every workspace (query the size
 *     with the matching *_workspace_bytes); the library never allocates memory
 *     the caller can see and never frees/syncs behind the caller's back;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the null stream) and is hipGraph-capturable;
 *   - return value: 0 = SRCNN_OK, negative = error (srcnn_last_error() gives
 *     text).  The legacy-named wrappers keep the reference's "1 = ok,
 *     0 = bad roi shape" convention (roi_align_cuda.c:19-22,39; nms_cuda.c:18).
 *   - activations are NHWC float32 inside the library; NCHW only at the edge.
 */
#ifndef SRCNN_HIP_H
#define SRCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRCNN_OK 0
#define SRCNN_ERR_ARG (-1)
#define SRCNN_ERR_HIP (-2)
#define SRCNN_ERR_WORKSPACE (-3)

#define SRCNN_FMT_F32 0
#define SRCNN_FMT_SPLIT16 1

typedef void *srcnn_stream_t; /* hipStream_t */

#define SRCNN_API __attribute__((visibility("default")))

SRCNN_API int srcnn_version(void);   /* 310 = result visualisation: srcnn_render_overlay, srcnn_overlay_workspace_bytes, srcnn_bev_lidar; 300 = training: optimiser step: srcnn_grad_norm (+ _workspace_bytes), srcnn_grad_scale, srcnn_sgd_step; 290 = training: remaining adjoints: srcnn_upsample_add_backward, srcnn_subsample2_backward, srcnn_pixel_shuffle2; 280 =convolution backward: srcnn_conv_bwd_desc, srcnn_conv2d_backward, srcnn_conv2d_backward_workspace_bytes; 270 = training target layers: srcnn_anchor_targets, srcnn_proposal_targets and their *_workspace_bytes; 260 = training losses: srcnn_cross_entropy, srcnn_smooth_l1, their _backward, srcnn_loss_workspace_bytes; 250 = KITTI object evaluation: srcnn_kitti_overlaps, srcnn_kitti_match (srcnn_kitti_split, srcnn_kitti_match_desc); 230 = round 5, second half: srcnn_conv_desc.up_top / up_format / up_H / up_W appended, srcnn_stem_pack_pair, srcnn_pool2x2_s1; 220 = round 5: srcnn_conv_desc.head_wf / head_rows / head_parts / head_plane appended, srcnn_rpn_score_levels / _parts, srcnn_box_head_tail, srcnn_proposal_workspace_layout; 210 = round 4: stream creation, placement probe, srcnn_conv_desc.head_* appended (older callers that zero the struct are unaffected) */
SRCNN_API const char *srcnn_last_error(void);

/* ------------------------------------------------------------------ NMS (A6)
 * Replaces  int nms_cuda(THCudaIntTensor *keep_out, THCudaTensor *boxes_host,
 *                        THCudaIntTensor *num_out, float nms_overlap_thresh)
 *           lib/model/nms/src/nms_cuda.h:4-5, nms_cuda.c:8-19, and the kernel +
 *           host greedy loop nms_cuda_kernel.cu:31-161.
 * dets (n, dim>=4) float32 [x1,y1,x2,y2,(score)], ALREADY score-sorted.
 * keep_out (n) int32, num_out (1) int32 -- both on the device, as in the
 * reference (nms_gpu.py:8-9).  The greedy reduction also runs on the device:
 * nothing is copied to the host.  Keep lists are bit-identical to the reference's own
 * kernel (built for gfx950 and run on the MI355X by tests/test_ref_kernels_gpu.py).
 * LIMIT: n <= 16384 boxes per problem (the reference's RPN uses 6000, cfg.TEST.RPN_PRE_NMS_TOP_N); a larger n
 * returns SRCNN_ERR_ARG (tests/test_ops_gpu.py covers 16384 and 16385).
 */
SRCNN_API size_t srcnn_nms_workspace_bytes(int n);
SRCNN_API int srcnn_nms(int *keep_out, const float *dets, int *num_out, int n, int dim, float thresh,
              void *workspace, size_t workspace_bytes, srcnn_stream_t stream);
/* nb independent problems of n boxes each (RPN: {left,right} x batch). n_valid (nb) may be NULL. */
SRCNN_API size_t srcnn_nms_batched_workspace_bytes(int nb, int n);
SRCNN_API int srcnn_nms_batched(int *keep_out, const float *dets, int *num_out, const int *n_valid,
                      int nb, int n, int dim, float thresh,
                      void *workspace, size_t workspace_bytes, srcnn_stream_t stream);
/* legacy name/return convention: 1 = ok. Scratch comes from a library-owned pool sized at first use. */
SRCNN_API int nms_cuda(int *keep_out, const float *boxes, int *num_out, int boxes_num, int boxes_dim,
             float nms_overlap_thresh, srcnn_stream_t stream);

/* ------------------------------------------------------------- ROIAlign (A8)
 * Replaces  int roi_align_forward_cuda(int aligned_height, int aligned_width,
 *                 float spatial_scale, THCudaTensor *features,
 *                 THCudaTensor *rois, THCudaTensor *output)
 *           lib/model/roi_align/src/roi_align_cuda.h:1-2, roi_align_cuda.c:7-40,
 *           kernel roi_align_kernel.cu:15-91.
 * features (B,C,H,W) NCHW, rois (n, roi_cols) [batch,x1,y1,x2,y2], output (n,C,ah,aw).
 * Returns 1 on success, 0 when roi_cols != 5 (output untouched) -- reference convention.
 */
SRCNN_API int roi_align_forward_cuda(int aligned_height, int aligned_width, float spatial_scale,
                           const float *features, int batch, int channels, int height, int width,
                           const float *rois, int num_rois, int roi_cols, float *output,
                           srcnn_stream_t stream);
/* The reduction behind RoIAlignAvg / RoIAlignMax (modules/roi_align.py:26-29, 41-44: avg_pool2d / max_pool2d(kernel 2,
 * stride 1) of the (A+1) x (A+1) lattice roi_align_forward_cuda returns): x (planes, h, w) -> y (planes, h-1, w-1).
 * take_max 0: ((a + b) + c) + d over rows then columns, x 0.25 (ATen's order); 1: the maximum (NaN propagates). */
SRCNN_API int srcnn_pool2x2_s1(const float *x, long long planes, int h, int w, float *y, int take_max, srcnn_stream_t stream);
/* Fused PyramidRoI_Feat (stereo_rcnn.py:110-139) = level routing (natural log, round half away)
 * + RoIAlignAvg (modules/roi_align.py:26-29: (A+1)^2 lattice, then 2x2/s1 avg-pool), NHWC maps.
 * maps[l] is the level-(l+2) map (B, mh[l], mw[l], C) NHWC.  out is (n, A, A, out_cstride) NHWC and
 * channels [out_coffset, out_coffset+C) are written (lets left|right be concatenated in place).
 * roi_limit: NULL, or a device int -- only rois [0, *roi_limit) are pooled (the keypoint head on the kept detections). */
SRCNN_API int srcnn_pyramid_roi_align(const float *const *maps_host, const int *mh_host, const int *mw_host,
                            int channels, float im_height, const float *rois, int num_rois, int A,
                            float *out, int out_cstride, int out_coffset, int maps_format, int out_format,
                            const int *roi_limit, srcnn_stream_t stream);
/* ------------------------------------------------- ROIAlign backward (training: the gradient with respect to the maps)
 * Replaces  int roi_align_backward_cuda(int aligned_height, int aligned_width, float spatial_scale,
 *                 THCudaTensor *top_grad, THCudaTensor *rois, THCudaTensor *bottom_grad)
 *           lib/model/roi_align/src/roi_align_cuda.h:4-5, roi_align_cuda.c:42-76, kernel roi_align_kernel.cu:94-162.
 * top_grad (n,C,ah,aw), rois (n, roi_cols), bottom_grad (B,C,H,W) NCHW.  Returns 1 on success, 0 when roi_cols != 5
 * (bottom_grad untouched; checked before any launch) -- reference convention.
 * DEFINED SUMMATION ORDER.  The reference scatters with float atomicAdd, so its result depends on arrival order; here every
 * map element is gathered: the float32 sum, starting from 0, of its contributions in ascending (roi index, ph, pw) order
 * (the four taps of one lattice point always fall on four different elements), each element written exactly once, no
 * atomics: results are run-to-run bit-equal.  One contribution of lattice point (n, c, ph, pw) with gradient g is the
 * reference's expression with C++'s promotions (roi_align_kernel.cu:137-140: `1.` is a double, `1 - w_ratio` a float):
 *   up-left    (float)((double)g * (1. - (double)h_ratio) * (double)(1.f - w_ratio))
 *   up-right   (float)((double)g * (1. - (double)h_ratio) * (double)w_ratio)
 *   down-left  (g * h_ratio) * (1.f - w_ratio)            down-right  (g * h_ratio) * w_ratio          (float products)
 * with the forward's geometry, outside-the-map test and hstart / wstart clamps.
 * OVERWRITE, NOT ACCUMULATE: on success bottom_grad is overwritten with the gradient (zeros where no roi reaches; no
 * zero fill is needed before the call).  The reference accumulates into bottom_grad, and its only caller passes a tensor
 * it has just zeroed (functions/roi_align.py:38-39): for that caller the two are the same.  A roi whose truncated batch
 * index (int)rois[n][0] lies outside [0, batch) contributes nothing (the reference would write outside the tensor). */
SRCNN_API int roi_align_backward_cuda(int aligned_height, int aligned_width, float spatial_scale,
                            const float *top_grad, const float *rois, int num_rois, int roi_cols,
                            float *bottom_grad, int batch, int channels, int height, int width,
                            srcnn_stream_t stream);
/* Adjoint of srcnn_pool2x2_s1: grad_y (planes, h-1, w-1) -> grad_x (planes, h, w), every element written.
 * take_max 0: a lattice point receives ((g00 + g01) + g10) + g11 over the (up to four) outputs that read it, taken in
 * row-major order of the outputs starting with the first that exists, x 0.25f; x may be NULL.
 * take_max 1: each output's gradient goes to the one lattice point torch.nn.functional.max_pool2d picks on the CPU
 * (first maximum in row-major window order; a NaN wins, the last one of several); a point picked by several outputs
 * adds them in the same row-major order; x is the forward's input (planes, h, w). */
SRCNN_API int srcnn_pool2x2_s1_backward(const float *grad_y, const float *x, long long planes, int h, int w, float *grad_x,
                              int take_max, srcnn_stream_t stream);
/* Adjoint of srcnn_pyramid_roi_align with respect to the four maps.  grad_out is (n, A, A, out_cstride) NHWC and channels
 * [out_coffset, out_coffset+C) are read (both multiples of 4); rois, A, im_height, roi_limit and the level routing as in
 * the forward.  grad_maps[l] is (batch, mh[l], mw[l], C) NHWC, maps_format must be SRCNN_FMT_F32 (anything else is an
 * error), and every element of every level is written (zeros where no roi reaches): one launch over the tiles of all
 * four levels.  The 2x2 average is folded in -- the lattice gradient of a point is ((g00 + g01) + g10) + g11 over the
 * outputs that exist, row-major, x 0.25f, formed in registers -- and the map sums follow roi_align_backward_cuda's
 * order, so the result is bit-equal to srcnn_pool2x2_s1_backward (average) followed by roi_align_backward_cuda on each
 * level's rois. */
SRCNN_API int srcnn_pyramid_roi_align_backward(const float *grad_out, int out_cstride, int out_coffset, const float *rois,
                                     int num_rois, int A, int channels, float im_height, float *const *grad_maps_host,
                                     const int *mh_host, const int *mw_host, int batch, int maps_format,
                                     const int *roi_limit, srcnn_stream_t stream);
/* format conversion of an NHWC activation tensor (pixels x C): F32 <-> SPLIT16 (API edge / tests) */
SRCNN_API int srcnn_act_convert(const void *x, int x_format, void *y, int y_format, long long pixels, int C,
                      srcnn_stream_t stream);

/* ------------------------------------------------- convolution engine (A1-A3, A9, A10)
 * Replaces the cuDNN calls behind nn.Conv2d / nn.ConvTranspose2d / nn.Linear in
 * stereo_rcnn/resnet.py:66-146,243-286, rpn/stereo_rpn.py:32-40.  Implicit GEMM on the
 * fp32 MFMA (v_mfma_f32_32x32x2_f32) or, with desc.precision = 1, on the f16 MFMA with an
 * error-compensated 3-term split: y = act(conv(x, w) + bias + residual).
 * x: (B,H,W,*) NHWC with pixel stride x_cstride floats, Cin must be a multiple of 32.
 * w: (Cout, KH, KW, Cin) float32 (K-contiguous rows).  Frozen BN is folded by the caller.
 */
typedef struct srcnn_conv_desc {
    const float *x;
    const float *w;
    const float *bias;     /* (Cout) or NULL */
    const float *residual; /* NHWC with pixel stride res_cstride, or NULL */
    float *y;              /* NHWC, pixel stride y_cstride, channels [y_coffset, y_coffset+Cout) */
    int B, H, W, Cin, x_cstride;
    int OH, OW, Cout;
    int KH, KW, stride, pad;
    int y_cstride, y_coffset, res_cstride;
    int relu;
    int mode;              /* 0 = conv; 1 = ConvTranspose2d(k=2,s=2): Cout = 4*Cq ordered (i,j,co); 2 = conv over a batch of
                            * B = 2*B' images whose second half is written beside the first: image b >= B' goes to pixel
                            * (b - B', oh, ow), channels y_coffset + Cout + co -- the stereo RPN's [left | right] concatenation
                            * (stereo_rpn.py:77-78) in one launch (SPLIT16 f16x3 engine only, no residual) */
    /* precision 0: fp32 MFMA, `w` is float32.
     * precision 1: error-compensated 3xf16 MFMA (fp32-class result): `w` = hi halves and `w_lo` = lo
     *   halves of (weight * 2^k), both (Cout, KH, KW, Cin) _Float16; w_inv_scale = 2^-k. */
    int precision;
    const void *w_lo;
    float w_inv_scale;
    /* launch plan override (0 = built-in heuristic): workgroup tile = (64*tile_mr) x (64*tile_nr), tile_mr/tile_nr
     * in {1,2}; splits = number of K slices (deterministic workspace reduction).  The SPLIT16 f16x3 engine also
     * takes tile_waves (4 or 8 wavefronts per workgroup; 0 = 4) and tile_stages (LDS ring depth 2..4 = K tiles of
     * DMA in flight + 1; 0 = 2), and with 8 waves tile_mr = 4 (256x128, 3 stages) and tile_mr = tile_nr = 4 (256x256,
     * 2 stages; layers whose channel counts / offsets are multiples of 8).  An override the engine does not
     * implement falls back to the heuristic.  Lets the host autotune each layer shape on the device it runs on. */
    int tile_mr, tile_nr, splits;
    /* activation formats (SRCNN_FMT_*).  SPLIT16: per pixel, each group of 8 channels is stored as
     * [8 x f16 hi][8 x f16 lo] (hi = f16(v), lo = f16(v - hi); same bytes as float32, channel strides
     * are still given in float32-equivalents).  With precision 1 and x_format SPLIT16 both GEMM
     * operands are DMA'd straight into LDS (buffer_load ... lds, 32-bit offsets relative to each tile's first input row).  fp32 engine: all formats must be F32. */
    int x_format, y_format, res_format;
    int tile_waves, tile_stages;
    int layer_tag;         /* caller's id of this layer (> 0) for srcnn_range_flag_read; 0 = untagged */
    /* Device-side row limit (SPLIT16 f16x3 engine; NULL = none): only output rows m < (*m_limit) * m_limit_mul are needed.
     * Workgroups whose whole tile lies beyond exit at once; rows beyond the limit inside a computed tile are still written.
     * Lets a fixed-shape launch list serve a data-dependent row count without a host read-back: the keypoint head runs on
     * the detections that survived class NMS only (*m_limit = the device-side keep count, m_limit_mul = rows per roi). */
    const int *m_limit;
    int m_limit_mul;
    /* Second input (SPLIT16 f16x3 engine, KH = KW = 1, pad 0, mode 0; NULL = none): y = act(W[:, :Cin] . x + W[:, Cin:] . x2' + bias)
     * with x2' = the (B, H2, W2, x2_cstride) SPLIT16 tensor x2 sampled at (oh * stride2, ow * stride2), Cin2 channels -- the
     * ResNet projection shortcut (resnet.py:86-100: out = bn3(conv3(.)) + downsample(x)) computed inside the block's last 1x1
     * conv as one GEMM over K = Cin + Cin2 instead of a launch of its own whose result is written and read back as the residual.
     * w / w_lo are (Cout, Cin + Cin2); both inputs must carry the same activation scale; no split-K. */
    const void *x2;
    int Cin2, H2, W2, x2_cstride, stride2;
    /* Fused narrow 1x1 head (SPLIT16 f16x3 engine; NULL = none): instead of storing y, the epilogue applies a second, 1x1
     * convolution with head_cout (= 6) output channels to the activated output pixel and stores only that:
     *   head_y[pixel, k] = head_scale * sum_c act(conv(x))[pixel, c] * head_w[k, c] + head_bias[k]      (float32, pixel stride 6)
     * head_w is float32 (head_cout, Cq) with Cq the channels of an output pixel (Cout, or Cout / 4 in mode 1), which must be 256
     * = the N extent of the 256x256 tile this form always runs on (one workgroup then owns every channel of its pixels);
     * head_scale undoes the activation scale 2^k the caller folded into w_inv_scale / bias.  The products are float32 FMAs in
     * a fixed order (8 channels per lane, then a DPP scan over the 32 lanes of a pixel): deterministic.  The keypoint branch
     * uses it for ConvTranspose2d + ReLU + the 6-channel classifier (resnet.py:258-262 of the reference: RCNN_kpts[12:14],
     * kpts_class): the (300, 28, 28, 256) upsampled tensor is neither written nor read back, one launch goes.  y may be NULL. */
    const void *head_w;
    const void *head_bias;
    void *head_y;
    int head_cout;
    float head_scale;
    /* MFMA form of the fused narrow head (NULL = none; not together with head_w): the same second 1x1 convolution, computed as a
     * small GEMM on the matrix pipe from the tile the epilogue holds in LDS -- 3-term f16 split like the engine itself, so the
     * result equals what a separate launch of the head on the stored SPLIT16 activations gives (up to the summation order).
     * head_wf: the head's weights (head_cout, C_h) split into hi / lo f16 (x 2^k like any weight) and zero-padded to head_rows
     *   (a multiple of 8, <= 24) rows, in FRAGMENT ORDER: [C_h / 16 steps][hi, lo][k group 0, 1][head_rows][8 halves], element
     *   (step s, g, n, i) = W[n][16 s + 8 g + i]   (stereo_rcnn_amd/engine.py: head_fragments builds it).
     * head_parts = 0, FINAL form (Cq = 256: the 256x256 tile owns every channel of its pixels; modes 0 and 1):
     *   head_y[pixel, k] = head_scale * sum_c act(conv(x))[pixel, c] W[k, c] + head_bias[k]     (head_cout floats per pixel)
     * head_parts > 0, PARTIAL form (modes 0 and 2; Cout a multiple of 256): C_h = Cout (mode 0) or 2 Cout (mode 2: the head reads
     *   [left Cout | right Cout], rows of the second half of the batch are the right eye) and every (eye, N tile) of the launch
     *   stores its share   head_y[(eye * ntiles + nt) * head_plane + pixel * head_cout + k] = head_scale * partial sum;
     *   the caller adds the planes in a fixed order and the bias (srcnn_rpn_score_parts).  ntiles = Cout / 256 (256x256 tile) or
     *   Cout / 128 (tile_mr = tile_nr = 2: the 128x128 8-wave tile): size head_y for head_parts >= eyes * Cout / 128 planes.
     * In both forms y is not written; the SPLIT16 range guard watches the activations that enter the head. */
    const void *head_wf;
    int head_rows;
    int head_parts;
    long long head_plane;
    /* Fused _upsample_add (SPLIT16 f16x3 engine, mode 0, no residual / head / split-K, channel counts multiples of 8; NULL = none):
     *   y = bilinear_align_corners(up_top -> (OH, OW)) + act(conv(x) + bias)
     * with up_top the coarser pyramid level, (B, up_H, up_W, Cout) NHWC in up_format -- the FPN lateral 1x1 conv and the
     * top-down addition behind it (stereo_rcnn.py:91-108, 161-167) in ONE launch: the float32 lateral map is neither written nor
     * read back.  The interpolation is srcnn_upsample_add's arithmetic operation by operation, and the conv's value is rounded to
     * float32 exactly as the two-launch form stores it, so the result is bit-identical to srcnn_conv2d (y float32) followed by
     * srcnn_upsample_add.  Not available on the 256x256 tile (an override asking for it falls back to the heuristic plan). */
    const void *up_top;
    int up_format, up_H, up_W;
} srcnn_conv_desc;
SRCNN_API size_t srcnn_conv2d_workspace_bytes(const srcnn_conv_desc *d);
/* The plan srcnn_conv2d would launch for d: plan_host[5] = (tile_mr, tile_nr, waves, stages, splits), waves and stages as the
 * launch table sees them (the engines without tile variants report 4 and 2).  An override the library does not implement for
 * this convolution is answered by the heuristic plan, never by an error: this is how a caller learns which one ran.  Nothing is
 * launched and no stream is touched. */
SRCNN_API int srcnn_conv2d_plan(const srcnn_conv_desc *d, int *plan_host);
SRCNN_API int srcnn_conv2d(const srcnn_conv_desc *d, void *workspace, size_t workspace_bytes, srcnn_stream_t stream);

/* CHAIN: up to three convolutions over the SAME output rows in ONE launch (SPLIT16 f16x3 engine, SPLIT16 in and out, mode 0,
 * unsplit).  descs[0] is any convolution; descs[i > 0] must be a 1x1 / stride 1 / pad 0 convolution whose input is exactly the
 * tensor descs[i-1] writes (same pointer, channel stride = y_cstride, y_coffset 0).  A workgroup owns one M tile and computes
 * every N tile of descs[0], then of descs[1], then of descs[2]: what a phase reads is what the SAME workgroup has just
 * written (read back from the L2), so nothing but a workgroup barrier orders the phases and the results are bit-identical to
 * the same convolutions launched one after the other with the same tiles.  This is the ResNet bottleneck
 * (/root/reference/lib/model/stereo_rcnn/resnet.py:82-102) SHIFTED BY ONE convolution -- [conv2 3x3 -> conv3 (+ residual or
 * projection shortcut) -> conv1 of the next block] -- so that the only convolution with a spatial footprint comes first and
 * reads a tensor the previous launch completed.  No phase may write the tensor descs[0] reads (other workgroups still need its
 * halo rows): the caller double-buffers it.  Residuals / second inputs are read at the workgroup's own rows and must be
 * tensors no phase writes.
 * Tile: descs[i].tile_mr / tile_waves / tile_stages must agree; tile_nr may take two values (the narrow and the wide
 * convolutions of a bottleneck); srcnn_conv2d_chain_supported says whether (tile_mr, waves, stages, narrow nr, wide nr) is
 * instantiated: (2,4,2,1,2) (2,4,2,1,1) (2,4,2,2,2) (2,8,2,2,2) (2,8,4,2,2) (4,8,3,2,2) (4,8,2,4,4).  Returns SRCNN_ERR_ARG otherwise
 * -- an explicit request is never silently replaced. */
SRCNN_API int srcnn_conv2d_chain_supported(int tile_mr, int tile_waves, int tile_stages, int nr_narrow, int nr_wide);
SRCNN_API int srcnn_conv2d_chain(const srcnn_conv_desc *descs, int n, srcnn_stream_t stream);
/* GROUP: up to five independent convolutions with ONE tile configuration in one launch (SPLIT16 f16x3 engine, unsplit; all with
 * the same output format and, if any, the same MFMA-form head shape): the grid runs over the tiles of all of them.  The stereo
 * RPN applies the shared RPN_Conv + heads to five pyramid levels (/root/reference/lib/model/rpn/stereo_rpn.py:73-95); the
 * coarse levels are launches of 6 to 76 tiles.  Tiles: (2,2,8,2) (4,2,8,3) (4,4,8,2) (2,1,4,2) as (tile_mr, tile_nr, waves, stages).
 * Each convolution's result is bit-identical to its own srcnn_conv2d launch with that tile. */
SRCNN_API int srcnn_conv2d_group(const srcnn_conv_desc *descs, int n, srcnn_stream_t stream);

/* ------------------------------------------------- convolution backward (training; exact-fp32 engine)
 * The gradients of y = act(conv(x, w) + bias + residual) as srcnn_conv2d computes it with mode 0, precision 0, F32 formats:
 * what torch.autograd derives for nn.Conv2d / nn.Linear (the reference has no kernel of its own here).  Both GEMMs run on
 * v_mfma_f32_32x32x2_f32.  With g = dy where relu == 0 and g = dy * [y > 0] where relu != 0 (y the saved forward output;
 * y == 0 gives 0, torch's convention):
 *   db[n]          = sum over (b, oh, ow) of g[b, oh, ow, n]
 *   dx[b, h, w, c] = sum over (kh, kw, n) of g[b, oh, ow, n] * w[n, kh, kw, c]   for the (oh, ow) with oh * stride - pad + kh = h
 *                    (and the same for w); taps with no such output pixel contribute nothing
 *   dw[n, kh, kw, c] = sum over (b, oh, ow) of g[b, oh, ow, n] * x[b, oh * stride - pad + kh, ow * stride - pad + kw, c]
 *   g_out          = g itself, dense (B, OH, OW, Cout): the gradient of the residual branch
 * Layouts follow the forward: x and dx are (B, H, W, *) NHWC with pixel stride x_cstride (channels [0, Cin) of every pixel of dx are
 * written, zeros included -- a 1x1 / stride 2 layer writes 0 to the three pixels in four it never read; floats between Cin and
 * the stride are left alone); y and dy are read at channels [y_coffset, y_coffset + Cout) of pixels of y_cstride floats; w and dw are
 * (Cout, KH, KW, Cin); db is (Cout).  Any of dx / dw / db / g_out may be NULL: that gradient is skipped (at least one must be
 * given); outputs are overwritten, never accumulated into, and need no zero fill.
 *
 * SCHEME.  (1) One mask / bias pass reads dy (and y) once and writes g into the workspace as (M, Cp) rows, M = B OH OW, Cp = Cout
 * rounded up to 32 with zeros in the padding, so that both GEMMs read aligned 128-byte runs whatever Cout is; the same pass
 * forms the bias partials and writes g_out.  The pass is skipped -- the GEMMs then read dy in place through y_cstride /
 * y_coffset -- when relu == 0, db and g_out are NULL, Cout is a multiple of 32 and y_cstride, y_coffset are multiples of 4.
 * (2) dx: a re-layout kernel writes w as (Cin, KH, KW, Cp) into the workspace (weights change every step: it is part of
 * the call), then an implicit GEMM in gather form, rows = the B H W input pixels, columns = Cin, K = (kh, kw, 32-channel tiles of Cp);
 * every element of dx is stored once by the workgroup that owns its tile: no memset, no atomics.  (3) dw: a GEMM with rows =
 * Cout, columns = (kh, kw, c), K = the M output pixels in tiles of 32, split over `splits` contiguous ranges of K tiles.
 *
 * DEFINED SUMMATION ORDER (no atomics anywhere; for a given descriptor -- tile_mr, tile_nr and splits included -- results are
 * run-to-run bit-equal).
 *   db: stage 1, workgroup q (256 threads) owns pixels [256 q, 256 q + 256) of one 32-channel tile; thread (r = t / 32, c = t % 32)
 *     adds pixels r, r + 8, r + 16, .. of the block in ascending order from 0; the eight r-sums of a channel are added in
 *     ascending r from 0 into partial[q][n].  Stage 2, one workgroup per 32-channel tile: thread (r, c) adds partial[r], [r + 8],
 *     .. in ascending order from 0, then the eight r-sums in ascending r from 0.
 *   dx: one fmaf chain per element (the MFMA's arithmetic) over taps in (kh, kw) row-major order, inside a tap over the 32-channel
 *     tiles of Cp in ascending order, inside a tile over the channel pairs (8 j + s, 8 j + 4 + s) for j = 0..3, s = 0..3 in (j, s)
 *     order -- srcnn_conv2d's K order.  Never split.
 *   dw: one fmaf chain per element and K slice over the slice's pixels in ascending m = (b, oh, ow) order; slice s covers K tiles
 *     [s T, min(s T + T, nkt)), T = ceil(nkt / splits), nkt = ceil(M / 32); with more than one slice the slices' sums are added
 *     in ascending s from 0 by a reduction kernel (partials in the workspace).  Pixels beyond M and taps outside the image enter
 *     as exact zeros.  splits = 0 lets the library choose (about two workgroups per compute unit, >= 8 K tiles per slice, <= 64
 *     slices); srcnn_conv2d_backward_workspace_bytes grows with it.
 * tile_mr / tile_nr in {1, 2} choose the (64 tile_mr) x (64 tile_nr) workgroup tile of BOTH GEMMs (0 = heuristic); any other
 * value is an error.
 *
 * Errors, all before the first launch (SRCNN_ERR_ARG with the reason in srcnn_last_error(); SRCNN_ERR_WORKSPACE for a workspace
 * smaller than srcnn_conv2d_backward_workspace_bytes, which returns 0 for a descriptor the call would refuse): a null desc /
 * dy / every output null / x null with dw / w null with dx / y null with relu ("null"); non-positive sizes or OH, OW that are
 * not the forward's ("shape"); Cin not a multiple of 32; strides too small or x_cstride, not a multiple of 4 ("stride");
 * mode != 0 ("mode"); precision != 0 ("precision"); a non-F32 format ("format"); head_w / head_wf ("fused head"), x2 ("second
 * input"), up_top ("upsample") -- the fields exist so that a forward descriptor copied over is refused, not misread. */
typedef struct srcnn_conv_bwd_desc {
    const float *x;        /* forward input (needed for dw) */
    const float *w;        /* forward weights (needed for dx) */
    const float *y;        /* saved forward output (needed when relu != 0), else NULL */
    const float *dy;       /* upstream gradient, laid out like y */
    float *dx, *dw, *db;   /* outputs; NULL = skip */
    float *g_out;          /* optional: the masked gradient, dense (B, OH, OW, Cout) */
    int B, H, W, Cin, x_cstride;
    int OH, OW, Cout;
    int KH, KW, stride, pad;
    int y_cstride, y_coffset;
    int relu;
    int mode, precision;                   /* mode 0; precision 0 for srcnn_conv2d_backward, 1 for srcnn_conv2d_backward_f16x3 */
    int x_format, y_format;                /* must be SRCNN_FMT_F32 */
    int tile_mr, tile_nr, splits;          /* 0 = heuristic */
    const void *head_w, *head_wf, *x2, *up_top;   /* must be NULL */
} srcnn_conv_bwd_desc;
SRCNN_API size_t srcnn_conv2d_backward_workspace_bytes(const srcnn_conv_bwd_desc *d);
SRCNN_API int srcnn_conv2d_backward(const srcnn_conv_bwd_desc *d, void *workspace, size_t workspace_bytes, srcnn_stream_t stream);

/* ------------------------------------------------- convolution backward, 3 x f16 split (training; opt-in)
 * The same gradients from the same descriptor, definitions (db, dx, dw, g_out), layouts and NULL-output rules, with the two GEMMs on
 * v_mfma_f32_32x32x16_f16 (fp32 accumulation).  desc.precision must be 1 here ("precision"); every other refusal is the fp32
 * call's, before the first launch.  srcnn_conv2d_backward itself keeps refusing precision != 0: neither call replaces the other.
 *
 * SCHEME.  Every product is  a b ~ (a_hi b_hi + a_hi b_lo + a_lo b_hi) / (s_a s_b),  t = s v, hi = f16(t), lo = f16(t - hi) (t and
 * t - hi are exact in fp32; lo lo is dropped): fp32-class results, a relative error of about 3 * 2^-22 per product plus the
 * fp32 accumulation.  SCALES: s is one power of two per operand tensor -- the masked gradient g, the weights w, and x for dw --
 * s = 2^(14 - floor(log2 max|v|)) with the exponent clamped to +-126, so the tensor's largest element lands in [2^14, 2^15)
 * whatever its range (gradients of 1e-6 and below would otherwise sit in the f16 subnormals).  What is left of a tensor's
 * dynamic range: an element below 2^-28 of its tensor's maximum has a subnormal hi and is carried with an absolute error of
 * up to 2^-39 of the maximum.  max|v| is found on the device (its float bits under an integer atomicMax, which no order can
 * change): for g in the mask / bias pass, for w and x in one read-only pass each; the words live in the workspace, are cleared
 * by the call's first kernel, and are read by the kernels that split.  Nothing is read back by the host.  Scaling dy (or x, or
 * w) by a power of two scales the results by exactly that power, bit for bit, as long as nothing leaves the fp32 range.  An
 * all-zero tensor gives exact zeros.
 * (1) The fp32 call's mask / bias pass -- the same code: g_out and db are bit-equal to srcnn_conv2d_backward's, db with the
 * same defined order -- always runs and writes g as fp32 (M, Cp) rows.  (2) dx: max|w|; the re-layout kernel writes w as two f16
 * planes hi, lo of (Cin, KH, KW, Cp); the implicit GEMM in gather form splits g while staging it into LDS; every element of dx is
 * stored once, zeros included.  (3) dw: max|x|; g and x are split and transposed (K = pixels must be contiguous per MFMA
 * lane) in registers while they are staged; split-K and its reduction are the fp32 call's.
 *
 * DEFINED SUMMATION ORDER (run-to-run bit-equal for a given descriptor, tile_mr, tile_nr and splits included).
 *   dx: K tiles over taps in (kh, kw) row-major order, inside a tap over the 32-channel tiles of Cp ascending; a K tile is two
 *     matrix steps of 16 channels.  Per step and element: cross += lo hi, main += hi hi, cross += hi lo (two fp32 accumulators;
 *     the 16 products of a step are summed by the matrix unit in its own fixed order).  Result (main + cross) / s_g / s_w.
 *   dw: per K slice (the fp32 call's slices) K tiles of 32 pixels in ascending m, two steps of 16 pixels each, the same two
 *     accumulators; (main + cross) / s_g / s_x per slice, slices added in ascending order by the reduction kernel.
 * The workspace query grows by the scale words; the re-laid weights take the same bytes as in the fp32 call. */
SRCNN_API size_t srcnn_conv2d_backward_f16x3_workspace_bytes(const srcnn_conv_bwd_desc *d);
SRCNN_API int srcnn_conv2d_backward_f16x3(const srcnn_conv_bwd_desc *d, void *workspace, size_t workspace_bytes, srcnn_stream_t stream);

/* ------------------------------------------------- convolution forward, 3 x f16 split with device-found scales (training; opt-in)
 *   y = relu?(conv(x, w) + bias + residual)
 * for weights that change every step: fp32 x and w in, fp32 y out, the GEMM on v_mfma_f32_32x32x16_f16 (fp32 accumulation) with
 * srcnn_conv2d_backward_f16x3's arithmetic and scales.  It is not srcnn_conv2d with precision 1 (prepared hi / lo weights, a
 * host-known weight exponent, SPLIT16 activations), which stays as it is; neither call replaces the other.
 * Layouts: x (B, H, W, *) NHWC with pixel stride x_cstride, channels [0, Cin) read and nothing behind them; w (Cout, KH, KW, Cin)
 * fp32, BN already folded; y written at channels [y_coffset, y_coffset + Cout) of pixels of y_cstride floats, nothing else of y
 * touched; bias (Cout) or NULL; residual dense (B, OH, OW, Cout) or NULL.
 *
 * SCHEME.  Every product is  a b ~ (a_hi b_hi + a_hi b_lo + a_lo b_hi) / (s_x s_w),  t = s v, hi = f16(t), lo = f16(t - hi), with
 * one power of two per operand tensor, s = 2^(14 - floor(log2 max|v|)), exponent clamped to +-126.  Passes, one stream, in order:
 * (1) the two max words in the workspace are cleared; (2) max|w| and (3) max|x| as float bits under an integer atomicMax; (4) w
 * is split into two f16 planes (Cp, KH, KW, Cin), Cp = Cout rounded up to 32, rows beyond Cout zero -- K is already contiguous,
 * nothing is transposed; (5) the implicit GEMM: rows = the B OH OW output pixels, columns = Cout, K = (kh, kw, 32-channel tiles of
 * Cin).  x stays fp32 in memory and is split while it is staged into LDS; taps outside the image and rows beyond M enter as exact
 * zeros.  Epilogue per element, every operation rounded once: (main + cross) * (1 / s_x) * (1 / s_w), + bias, + residual, ReLU;
 * each element of y is stored exactly once.  No atomics other than the max words -- the two of x and w and, in
 * srcnn_conv2d_forward_f16x3_maxima, the third word y_amax, all integer maxima that no order can change -- nothing read back by the
 * host, no device-scope fence; the call can be captured into a graph.
 * Scaling x or w by a power of two scales the GEMM's result by exactly that power, bit for bit (as long as nothing leaves the
 * normal fp32 range); an all-zero x gives y = relu?(bias + residual) exactly.
 *
 * DEFINED SUMMATION ORDER (a function of the geometry alone: run-to-run bit-equal, and bit-equal across tile_mr / tile_nr, since K
 * is never split and an element's K order does not depend on the tile that holds it).  K tiles over taps in (kh, kw) row-major
 * order, inside a tap over the 32-channel tiles of Cin ascending; a K tile is two matrix steps of 16 channels.  Per step and
 * element: cross += lo hi, main += hi hi, cross += hi lo (two fp32 accumulators; the 16 products of a step are summed by the
 * matrix unit in its own fixed order).
 * tile_mr / tile_nr in {1, 2} choose the (64 tile_mr) x (64 tile_nr) workgroup tile (0 = heuristic); any other value is an error.
 *
 * Errors, all before the first launch (SRCNN_ERR_ARG with the reason in srcnn_last_error(); SRCNN_ERR_WORKSPACE for a workspace
 * smaller than srcnn_conv2d_forward_f16x3_workspace_bytes, which returns 0 for a descriptor the call would refuse): a null desc /
 * x / w / y ("null"); non-positive sizes or OH, OW that are not the forward's ("shape"); Cin not a multiple of 32; strides too
 * small or x_cstride not a multiple of 4 ("stride"); x or w not 16-byte aligned ("aligned"); a non-F32 format ("format"); a tile
 * outside {0, 1, 2} ("tile").  The struct has no fused-head, second-input or upsample fields. */
typedef struct srcnn_conv_fwd_f16x3_desc {
    const float *x, *w;
    const float *bias;         /* (Cout) or NULL */
    const float *residual;     /* dense (B, OH, OW, Cout) or NULL */
    float *y;
    int B, H, W, Cin, x_cstride;
    int OH, OW, Cout;
    int KH, KW, stride, pad;
    int y_cstride, y_coffset;
    int relu;
    int x_format, y_format;    /* must be SRCNN_FMT_F32 */
    int tile_mr, tile_nr;      /* 0 = heuristic */
} srcnn_conv_fwd_f16x3_desc;
SRCNN_API size_t srcnn_conv2d_forward_f16x3_workspace_bytes(const srcnn_conv_fwd_f16x3_desc *d);
SRCNN_API int srcnn_conv2d_forward_f16x3(const srcnn_conv_fwd_f16x3_desc *d, void *workspace, size_t workspace_bytes, srcnn_stream_t stream);

/* ------------------------------------------------- 3 x f16 training calls: max |x| handed from layer to layer
 * A scale is a function of max|x| alone, and a maximum does not depend on who computed it: the three entries below let a training
 * step find the maximum of an activation once and read it from a device word everywhere else.  The results keep the bits of the
 * plain entries.  A word is one 4-byte aligned unsigned in device memory holding the float bits of a maximum (0 for an all-zero
 * tensor; NaNs are dropped by fmaxf).  Nothing is read by the host and there is no device-scope fence: all three can be captured.
 *
 * srcnn_conv2d_forward_f16x3_maxima: srcnn_conv2d_forward_f16x3 (same descriptor, validation, messages and workspace query) with
 *   x_amax: NULL, or the word of max|x| over channels [0, Cin) of ALL B H W input pixels -- what the call's own pass scans,
 *     pixels a strided layer never reads included.  When given, the max|x| launch is not issued and the GEMM takes s_x from it.
 *   y_amax: NULL, or a word the call OVERWRITES (it is cleared by the call's clear launch, whatever it held) with max|y| over
 *     exactly the elements it stores: rows < M, columns < Cout, after bias, residual and ReLU.  Each thread of the GEMM's epilogue
 *     keeps fmaxf(mx, |v|) of what it stores, a wave reduces it, and one integer atomicMax per wave with a non-zero maximum lands in
 *     the word.  With y_amax NULL the GEMM kernel is the plain entry's.
 *   Additional refusals, before any launch: a word that is not 4-byte aligned ("aligned"); x_amax == y_amax ("alias").
 * srcnn_conv2d_backward_f16x3_maxima: srcnn_conv2d_backward_f16x3 with the weight gradient's max|x| launch replaced by the word
 *   x_amax when it is not NULL (same definition as above: channels [0, Cin) of all B H W pixels of the saved x); the mask / bias
 *   pass, max|g|, max|w|, dx, split-K and its reduction are unchanged, db and g_out stay bit-equal to the fp32 call's.
 * srcnn_absmax: the calls' own scan behind an entry: *word is overwritten with the float bits of max|x| over `rows` rows of `len`
 *   floats at a stride of `stride` >= len floats; floats behind len are never read.  For an activation that no f16x3 convolution
 *   produced and that several calls consume.  Refused: null x / word, misaligned pointers, non-positive rows / len. */
SRCNN_API int srcnn_conv2d_forward_f16x3_maxima(const srcnn_conv_fwd_f16x3_desc *d, const unsigned *x_amax, unsigned *y_amax,
                                                void *workspace, size_t workspace_bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_conv2d_backward_f16x3_maxima(const srcnn_conv_bwd_desc *d, const unsigned *x_amax, void *workspace,
                                                 size_t workspace_bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_absmax(const float *x, long long rows, int len, long long stride, unsigned *word, srcnn_stream_t stream);

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

/* ------------------------------------------------- training: remaining adjoints
 * The three differentiable operators of the reference's training branch that are neither a convolution, a ROIAlign nor a loss:
 * _upsample_add (stereo_rcnn.py:91-108), MaxPool2d(1, stride 2) (stereo_rcnn.py:39,168) and the layout step of
 * ConvTranspose2d(256, 256, 2, 2) (conv mode 1).  NHWC float32, channel counts multiples of 8, 16-byte aligned pointers.  No
 * atomics: every output element is owned by one thread and written exactly once (zeros included), so outputs need no zero fill
 * and results are run-to-run bit-equal.
 *
 * srcnn_upsample_add_backward: the adjoint of srcnn_upsample_add with respect to top; dy (B, H, W, C), d_top (B, TH, TW, C).  (The
 * lateral's gradient is dy itself; no kernel.)  With the forward's float32 expressions rh = (TH - 1) / (H - 1) (0 for H == 1),
 * h1 = (int)(rh * h), h1p = [h1 < TH - 1], h1l = rh * h - h1, h0l = 1 - h1l, and the same for columns, the forward reads for
 * output pixel (h, w) the four taps  (h1, w1) (h1, w1 + w1p) (h1 + h1p, w1) (h1 + h1p, w1 + w1p)  with coefficients
 * h0l w0l, h0l w1l, h1l w0l, h1l w1l.  Then
 *   d_top[b, th, tw, c] = sum over (h, w, tap) with tap position == (th, tw) of coefficient * dy[b, h, w, c]
 * in gather form, one thread per (top pixel, 8-channel group).  Candidate rows are taken from th / rh with one row of slack on
 * each side and accepted only after h1 has been recomputed the forward's way, so a rounding disagreement can neither drop nor
 * double a term; at the last top row, where h1p == 0, both row taps of an output row are the same top row and both count.
 * DEFINED SUMMATION ORDER: ascending h, inside a row ascending w, inside an output pixel the four taps in the order above; one
 * chain acc = fmaf(k, dy, acc) from 0 with k = hl * wl rounded to float32 once.  rh == 0 (H == 1 or TH == 1): every output
 * row reads top row 0.  Holds for any H >= TH, W >= TW, not only H ~ 2 TH.
 *
 * srcnn_subsample2_backward: dx[b, 2i, 2j, :] = dy[b, i, j, :] and 0 elsewhere; dy (B, OH, OW, C), dx (B, H, W, C),
 * OH = ceil(H / 2), OW = ceil(W / 2) (H, W may be odd).  No sum.
 *
 * srcnn_pixel_shuffle2: the layout step of conv mode 1 as a copy of its own.  packed (M, h, w, 4 Cq), channels ordered (i, j, co)
 * as engine.prep_deconv2x2 orders the GEMM's rows, and wide (M, 2h, 2w, Cq):  wide[m, 2a + i, 2b + j, co] =
 * packed[m, a, b, (2i + j) Cq + co].  inverse == 0: x is packed, y is wide; inverse == 1: x is wide, y is packed.  No sum.  With it
 * the differentiable deconvolution is a mode-0 1x1 convolution to 4 Cq channels (+ ReLU) followed by the shuffle, and its
 * backward the inverse shuffle of dy followed by srcnn_conv2d_backward, which keeps refusing mode != 0.
 *
 * Errors, all before the first launch (SRCNN_ERR_ARG with the reason in srcnn_last_error()): a null pointer ("null"); a
 * non-positive size, H < TH or W < TW, OH / OW that are not ceil(H / 2) / ceil(W / 2), inverse outside {0, 1}, a map beyond the
 * launch grid ("shape"); a channel count that is not a multiple of 8 ("stride"); a pointer that is not 16-byte aligned
 * ("aligned"). */
SRCNN_API int srcnn_upsample_add_backward(const float *dy, int B, int H, int W, int C, float *d_top, int TH, int TW,
                                          srcnn_stream_t stream);
SRCNN_API int srcnn_subsample2_backward(const float *dy, int B, int OH, int OW, int C, float *dx, int H, int W, srcnn_stream_t stream);
SRCNN_API int srcnn_pixel_shuffle2(const float *x, int M, int h, int w, int Cq, float *y, int inverse, srcnn_stream_t stream);

/* SPLIT16 range guard.  The format stores hi = f16(v) unscaled: an activation beyond +-65504 (or a NaN) becomes inf and
 * poisons what it touches, where the fp32 engine would carry on.  Every kernel that writes SPLIT16 from fresh arithmetic
 * records it: a library-owned device word keeps max(layer_tag + 1) over the launches that produced such a value since
 * the last reset (0 = every SPLIT16 tensor was in range; 9001 = srcnn_upsample_add, 9002 = an input converted by
 * srcnn_stem_pack / srcnn_act_convert, 9003 = an F32 input pooled into SPLIT16 by srcnn_maxpool3x3s2_ceil; a NaN is looked for BEFORE a ReLU, which would turn it into 0).  srcnn_range_flag_read copies the word
 * to the host (it SYNCHRONISES the device) and optionally clears it; srcnn_pack_detections also drops it into
 * rec[0][1], so that the 3-D flow sees it without an extra copy.  A caller that finds it set re-runs the pair with
 * desc.precision = 0 (exact fp32 engine, F32 activations): stereo_rcnn_amd/pipeline.py does. */
SRCNN_API int srcnn_range_flag_read(int reset);
SRCNN_API const void *srcnn_range_flag_device_word(void);
/* Gives the calling THREAD its own flag word (4 zero-initialised bytes of device memory owned by the caller, on the device
 * the launches go to) for every library call it makes from now on; NULL returns to the library's process-wide word.
 * With several forwards in flight on different streams each one binds its own word before it is enqueued, so that a
 * forward is judged by its own range flag only.  srcnn_pack_detections copies the bound word into the record (row 0,
 * column 1) and clears it on its stream; srcnn_range_flag_read reads (and resets) the bound word. */
SRCNN_API int srcnn_range_flag_bind(void *device_word);

/* A0 preprocessing (demo.py:103-129, blob.py:39-64): uint8 RGB (H,W,3) on the device -> BGR, PIXEL_MEANS subtracted
 * (in double, stored float32, as numpy's float32 -= float64), then cv2.resize(img, None, None, fx=scale, fy=scale,
 * INTER_LINEAR) restated operation by operation from OpenCV's float path (oracle/preprocess.py cites it): bit-equal
 * to that restatement.  OH/OW MUST be what cv::resize derives: cvRound(H*scale), cvRound(W*scale) (ties to even).
 * Outputs (either may be NULL): out_nchw = float32 (3,OH,OW) planes, the network input forward()/dense alignment take;
 * packed = the stem's zero-bordered NHWC4 input (1, OH+6, OW+8, 4) exactly as srcnn_stem_pack would write it from
 * out_nchw, in packed_format F32 or SPLIT16 -- the fused form: no float32 intermediate is re-read to feed the stem. */
SRCNN_API int srcnn_preprocess(const unsigned char *img_rgb, int H, int W, double scale, float *out_nchw, int OH, int OW,
                     float *packed, int packed_format, srcnn_stream_t stream);
/* stem input repack: NCHW (B,3,H,W) -> zero-bordered NHWC4 (B, H+6, W+8, 4) so that the 7x7/2
 * stem (resnet.py:109) becomes 7 taps of 32 contiguous floats for the conv engine (srcnn_conv2d with Cin = 32,
 * x_cstride = 4, KH = 7, KW = 1, stride 2, pad 0).  out_format SRCNN_FMT_SPLIT16: the same bytes hold, per padded row,
 * one [8 x f16 hi][8 x f16 lo] group per two pixels (groups aligned to the row start; an odd last pixel is not
 * written -- the stem never reads it), which is what the DMA form of the f16x3 engine takes as x_format. */
SRCNN_API int srcnn_stem_pack(const float *im_nchw, int B, int H, int W, float *out, int out_format,
                              srcnn_stream_t stream);
/* ... of a stereo batch in one launch: out (2B, H+6, W+8, 4) = the B left images, then the B right ones -- the batch order
 * the shared trunk runs on (stereo_rcnn.py:155-158 feeds both eyes through the same RCNN_layer0..4). */
SRCNN_API int srcnn_stem_pack_pair(const float *left_nchw, const float *right_nchw, int B, int H, int W, float *out,
                                   int out_format, srcnn_stream_t stream);
/* MaxPool2d(3, stride 2, pad 0, ceil_mode) NHWC (resnet.py:113). */
SRCNN_API int srcnn_maxpool3x3s2_ceil(const float *x, int B, int H, int W, int C, float *y, int OH, int OW,
                            int y_format, srcnn_stream_t stream);
/* _upsample_add (stereo_rcnn.py:91-108): y = bilinear_align_corners(top -> (H,W)) + lateral, NHWC. */
SRCNN_API int srcnn_upsample_add(const float *top, int TH, int TW, const float *lateral, int B, int H, int W, int C,
                       float *y, int top_format, int y_format /* lateral is always F32 */, srcnn_stream_t stream);
/* MaxPool2d(1, stride 2) (stereo_rcnn.py:39,168): y[b,i,j,:] = x[b,2i,2j,:]. */
SRCNN_API int srcnn_subsample2(const float *x, int B, int H, int W, int C, float *y, int OH, int OW, srcnn_stream_t stream);
/* layout edge helpers */
SRCNN_API int srcnn_nhwc_to_nchw(const float *x, int B, int H, int W, int C, float *y, srcnn_stream_t stream);
SRCNN_API int srcnn_nchw_to_nhwc(const float *x, int B, int C, int H, int W, float *y, srcnn_stream_t stream);

/* ---------------------------------------------------- stereo RPN scoring + proposals (A3-A5)
 * head: (B, hw, head_cstride>=24) NHWC rows of one level's fused 1x1 heads, channels [0,6) =
 * RPN_cls_score logits, [6,24) = RPN_bbox_pred_left_right.  Writes that level's slice of probs
 * (B, A, 2) and deltas (B, A, 6) (anchor index = level_offset + loc*3 + a) in the reference's
 * flattened order, reproducing the (c, c+3) softmax pairing quirk (stereo_rpn.py:81-83,89-91). */
SRCNN_API int srcnn_rpn_score(const float *head, int B, int hw, int head_cstride, float *probs, float *deltas,
                    int level_offset, int num_anchors_total, srcnn_stream_t stream);
/* The same for ALL pyramid levels in one launch: heads[l] (B, level_hw[l], head_cstride) of level l (host arrays of nlevels <= 5
 * entries); level l's anchors start at 3 x the locations of the levels before it; num_anchors_total = 3 x all locations. */
SRCNN_API int srcnn_rpn_score_levels(const float *const *heads, const int *level_hw, int nlevels, int B, int head_cstride,
                                     float *probs, float *deltas, int num_anchors_total, srcnn_stream_t stream);
/* ... and from the per-(eye, N tile) PARTIAL sums the RPN conv's fused head leaves (srcnn_conv_desc.head_wf, partial form): level l
 * has nparts[l] planes of plane_floats[l] >= B * level_hw[l] * 24 floats each, plane q at parts[l] + q * plane_floats[l], rows
 * (b * hw + loc) x 24 channels; the planes are added in index order, then bias24 (the head's 24 biases, device), then as above. */
SRCNN_API int srcnn_rpn_score_parts(const float *const *parts, const int *nparts, const long long *plane_floats, const int *level_hw,
                                    int nlevels, int B, const float *bias24, float *probs, float *deltas, int num_anchors_total,
                                    srcnn_stream_t stream);
/* Whole _ProposalLayer.forward (proposal_layer.py:42-145): anchors (generate_anchors.py:112-173),
 * decode+clip (bbox_transform.py:79-104,177-185), stable descending sort / top pre_nms,
 * NMS(left) & NMS(right), sorted intersection, first post_nms, zero pad, batch index in col 0.
 * probs (B, A, 2), deltas (B, A, 6); level_hw_host: nlevels x {H, W}; rois_* (B, post_nms, 5).
 * The scores probs[..., 1] must be finite and non-negative (softmax outputs; no -0.0f, no NaN): the selection orders them by bits.
 * LIMITS: specialised to the reference's anchor configuration (config.py: FPN_ANCHOR_SCALES {32,64,128,256,512} one per
 * level, FPN_FEAT_STRIDES {4,8,16,32,64}, ANCHOR_RATIOS {0.5,1,2}, i.e. nlevels == 5 and 3 anchors per location:
 * num_anchors must equal 3 * sum(H_l * W_l) and stay below 4M); pre_nms <= 8192 (radix top-K buffer), post_nms <= pre_nms.  Anything else
 * returns SRCNN_ERR_ARG with the reason in srcnn_last_error(). */
SRCNN_API size_t srcnn_proposal_workspace_bytes(int B, int num_anchors, int pre_nms, int post_nms);
SRCNN_API int srcnn_proposal_layer(const float *probs, const float *deltas, int B, int num_anchors,
                         const int *level_hw_host, int nlevels, const float *im_info /* (B,3) device */,
                         int pre_nms, int post_nms, float nms_thresh,
                         float *rois_left, float *rois_right, int *num_valid /* (B) device, may be NULL */,
                         void *workspace, size_t workspace_bytes, srcnn_stream_t stream);
/* Inspection (tests; not on the hot path): where srcnn_proposal_layer leaves its intermediates in the caller's workspace after
 * a call with the same (B, num_anchors, pre_nms) -- byte offsets of: [0] order (B x n int32: the n = min(pre_nms, A) best
 * anchors, descending score, ties by ascending index), [1] dets (B x 2 x n x 5 float32: decoded + clipped left / right boxes and
 * the score, in that order), [2] keep (B x 2 x n int32: ascending row indices that survive the NMS; the left / right scans of an
 * image stop together once post_nms rows survive in both, so each list is a PREFIX of the full greedy list), [3] num (B x 2
 * int32: entries of each keep list), [4] total bytes.  This is what lets a test compare the kernels' actual discrete decisions
 * with a reference run's (tests/tie_audit.py).  Returns SRCNN_OK, or SRCNN_ERR_ARG for n_offsets < 5. */
SRCNN_API int srcnn_proposal_workspace_layout(int B, int num_anchors, int pre_nms, size_t *offsets, int n_offsets);

/* ------------------------------------------------------------------ heads (A9-A12)
 * cls softmax over n_cls logits (stereo_rcnn.py:257). */
SRCNN_API int srcnn_softmax_rows(const float *x, int rows, int cols, int x_stride, float *y, srcnn_stream_t stream);
/* The box head's stacked fc output (rows, fc_stride >= n_bbox + n_dim + n_cls): columns [RCNN_bbox_pred | RCNN_dim_orien_pred |
 * RCNN_cls_score] (stereo_rcnn.py:251-257) split in ONE launch into the three tensors the forward returns -- the regressions
 * copied bit for bit into contiguous rows, the class logits through the softmax above. */
SRCNN_API int srcnn_box_head_tail(const float *fc, int rows, int n_bbox, int n_dim, int n_cls, int fc_stride, float *bbox_pred,
                                  float *dim_orien_pred, float *cls_prob, srcnn_stream_t stream);
/* keypoint tail (stereo_rcnn.py:262-271): logits (n, G, G, 6) NHWC from kpts_class ->
 * sum over H, softmax over 4*G (kpts) and G (left/right borders).  roi_limit: NULL, or a device int -- rows [0, *roi_limit) only. */
SRCNN_API int srcnn_kpts_tail(const float *logits, int n, int G, float *kpts_prob, float *left_prob, float *right_prob,
                    const int *roi_limit, srcnn_stream_t stream);
/* detection decode (demo.py:144-218, bbox_transform.py:133-155) for B == 1 blocks of n rois. */
/* Keypoint head on the kept detections only ("lazy" form of stereo_rcnn.py:260-271 + demo.py:196-209: the reference computes the
 * keypoint branch for all 300 rois and its scripts then read the rows that survive score threshold + NMS; every roi's
 * keypoint computation is independent of the others).
 * srcnn_gather_rows: dst[r] = src[max(idx[r], 0)] for r < n_idx (rows of `cols` floats; -1 padded index lists repeat row 0).
 * srcnn_decode_kept_kpts: for r < *num_keep, i = keep_idx[r]: kpts[i] (5 floats, as srcnn_decode_detections writes them)
 *   from row r of the kept-order probability arrays and roi i of rois_left; other rows of `kpts` are left alone. */
SRCNN_API int srcnn_gather_rows(const float *src, const int *idx, int n_idx, int cols, float *dst, srcnn_stream_t stream);
SRCNN_API int srcnn_decode_kept_kpts(const float *rois_left, const float *kpts_prob, const float *left_prob,
                                     const float *right_prob, const int *keep_idx, const int *num_keep, const float *im_info,
                                     int n, int G, float *kpts, srcnn_stream_t stream);
SRCNN_API int srcnn_decode_detections(const float *rois_left, const float *rois_right, const float *bbox_pred,
                            const float *dim_orien_pred, const float *kpts_prob, const float *left_prob,
                            const float *right_prob, const float *im_info, int n, int n_cls, int G,
                            float *boxes_left, float *boxes_right, float *dim_orien, float *kpts,
                            srcnn_stream_t stream);
/* per-class filter + sort + NMS (demo.py:231-257): scores (n, n_cls) column j; outputs the kept
 * ORIGINAL roi indices in descending score order and their count, all on the device. */
SRCNN_API size_t srcnn_class_nms_workspace_bytes(int n);
SRCNN_API int srcnn_class_nms(const float *scores, int n, int n_cls, int j, const float *boxes_left /* (n,4*n_cls) */,
                    float score_thresh, float nms_thresh, int *keep_idx, int *num_keep,
                    void *workspace, size_t workspace_bytes, srcnn_stream_t stream);

/* fixed-size, zero-padded detection record of one image: what the 3-D stage works on in place and what the multi-GPU
 * gather moves (new: the reference writes per-image txt files instead, kitti_utils.py:456-460).
 * rec ((n+1), rec_cols) float32, row 0 = [count, 0...], row 1+r = the r-th kept detection (descending score):
 *   0 score | 1-4 left box | 5-8 right box | 9-13 dim_orien (w,h,l,sin,cos) | 14-18 kpts (u,type,prob,left,right border)
 *   19 roi index | 20 4-DoF status | 21-24 x,y,z,theta of the 4-DoF solve (float32, = the reference's poses_all)
 *   25 dense-alignment status | 26 aligned disparity | 27-30 final x,y,z,theta | 31 alpha (poses_all[:,7])
 * srcnn_pack_detections fills columns 0-19 (rec_cols >= 20) and zeroes the rest; the 3-D calls need SRCNN_REC_COLS. */
#define SRCNN_REC_COLS 32
SRCNN_API int srcnn_pack_detections(const float *scores, const float *boxes_left, const float *boxes_right,
                          const float *dim_orien, const float *kpts, const int *keep_idx, const int *num_keep,
                          int n, int n_cls, int j, int rec_cols, float *rec, srcnn_stream_t stream);

/* ------------------------------------------------------------ dense alignment (A15-A16)
 * Replaces lib/model/dense_align/dense_align.py:13-69,175-300 + box_3d.py:12-106 (align_parallel).
 * im_left/right: (3, H, W) planar float32 network-input tensors; the 2x align_corners bilinear
 * upsample of dense_align.py:256-257 is done inside (workspace).  boxes (R,4) and borders (R,2)
 * in ORIGINAL-image pixels (borders = keypoints[:,3:5]), poses (R,7) [x,y,z,w,h,l,theta].
 * scale = im_info[0,2]; p2_00/p2_02/p2_12 = P2 focal/cx/cy; p2_03_minus_p3_03 = P2[0,3]-P3[0,3]
 * (host doubles, as in the reference).  max_pixels bounds the per-object sample count; the reference's lattice has at
 * most 113 x 46 points, so 8192 can never overflow -- an object whose lattice does not fit a smaller bound is reported
 * with status -1 (never silently truncated).  Outputs status (R: 1 ok, 0 no valid pixel, -1 overflow) and best_dis (R)
 * float32 on the device. */
SRCNN_API size_t srcnn_dense_align_workspace_bytes(int H, int W, int R, int max_pixels);
/* Where, inside the workspace of a finished srcnn_dense_align call with the same sizes, the intermediate results of the depth
 * search live (byte offsets; for parity audits of the discrete argmin -- reference dense_align.py:225-232 -- and diagnostics):
 *   offsets[0] = int32 cnt[2 R]: valid lattice pixels per object, then overflow flags
 *   offsets[1], [2], [3] = coarse stage: float depth_enum[50][R], float cost[50][R] (sum over pixels and channels of |L - R|,
 *                          workgroup-reduced in a fixed order), float best_depth[R] (first minimum)
 *   offsets[4], [5], [6] = fine stage: depth_enum[20][R] (rows 20..49 unused), cost[20][R], best_depth[R]
 * n_offsets must be >= 7.  With n_offsets >= 11 the stages BEFORE the search are located too (stage-level parity tests):
 *   offsets[7], [8] = float up_left[3][2H][2W], up_right[3][2H][2W]: the 2x upsampled images
 *   offsets[9]      = float uvz[R][max_pixels][3]: (u, v, dz) of every valid lattice pixel, compacted in row-major lattice order;
 *                     rows cnt[r].. of an object are never written
 *   offsets[10]     = float left_val[R][max_pixels][3]: the left image's taps at (u, v), per channel
 * A caller passing 7..10 gets offsets[0..6] only, as before. */
SRCNN_API int srcnn_dense_align_workspace_layout(int H, int W, int R, int max_pixels, size_t *offsets, int n_offsets);
SRCNN_API int srcnn_dense_align(const float *im_left, const float *im_right, int H, int W, double scale,
                      double p2_00, double p2_02, double p2_12, double p2_03_minus_p3_03,
                      const float *boxes, const float *borders, const float *poses,
                      const float *valid /* (R) or NULL: rows with valid <= 0 are skipped (status 0), so a fixed-size
                                            batch can be aligned without compacting it on the host */,
                      int R, int max_pixels,
                      float *status, float *best_dis, void *workspace, size_t workspace_bytes,
                      srcnn_stream_t stream);

/* ------------------------------------------------------------ 3-D stage on the device (A13, A14, A17)
 * All three work IN PLACE on one image's record (see srcnn_pack_detections), asynchronously, no host round trip.
 * srcnn_infer_boundary: kitti_utils.py:398-437 (occlusion "depth line" over the image columns from the left boxes) and
 *   the replacement rule of demo.py:262-265 -- columns 17/18 are overwritten where the regressed borders are narrower
 *   than half the inferred ones.  workspace: srcnn_box3d_workspace_bytes(n, im_w).
 * srcnn_solve_4dof: demo.py:282-302 = box_estimator.py:169-385 for every row with score > eval_thresh: scipy's Newton-CG
 *   (optimize/_optimize.py:_minimize_newtoncg + MINPACK-2 dcsrch / wolfe2 line searches) restated in double precision,
 *   one detection per workgroup, the eight re-projection residuals of every cost / gradient evaluation on eight lanes of its
 *   wavefront, summed in lane order (csrc/box_solver_wave.h).  Writes columns 20-24, 27-31 and state4 (n,4) doubles
 *   (x, y, z, theta).  srcnn_solve_4dof_scalar / srcnn_solve_3dof_scalar: the same iteration with one lane evaluating the
 *   residuals one after another (the form of rounds 2-5) -- bit-identical results, ~4x the time; kept as the lane form's test.
 * srcnn_align_inputs: the arrays align_parallel takes (boxes (n,4), borders (n,2), poses (n,7), valid (n)) from the record.
 * srcnn_solve_3dof: demo.py:311-319 = box_estimator.py:387-545 for rows whose 4-DoF solve and dense alignment
 *   succeeded (align_status / best_dis (n) from srcnn_dense_align, or both NULL = no alignment): columns 25-30 and
 *   state (n,4) doubles (x, y, z = f b / disparity, theta).
 * P2 / P3 entries are host doubles as in the reference (calib.p2[0,0], [0,2], [1,2], p2[0,3] - p3[0,3]).
 *
 * PARITY GRADE of the two device solvers: numerically equivalent to the reference, NOT reference-identical.  They run the
 * reference's iteration (same Newton-CG, same line searches, same stopping rules) with ROCm ocml's cos / sin / atan2 and
 * exact squares where the reference's scipy / numpy path goes through glibc's libm and pow(v, 2).  Those differ in the last
 * bit, and the reference's end point is not a smooth function of its inputs (its gradient is not the gradient of its cost;
 * the iteration stops on scipy's step tolerance, 1e-3..1e-2 short of the optimum): against the host build, on the same
 * inputs, 72 % of the 4-DoF and 98 % of the 3-DoF end points of well-posed cases agree within 1e-4 and the rest jump like
 * the reference itself does when its inputs move by 1e-5 (tests/test_box3d_gpu.py, tests/test_box3d_conditioning.py,
 * DESIGN.md section 7).  Status columns are identical.  Callers that need the reference's boxes bit for bit use the record
 * forms on host memory below (srcnn_solve_*_records_host: the default of stereo_rcnn_amd.pipeline, solver='host').
 *
 * "Bit-identical to the reference's scipy path" is a statement about NumPy >= 2 (NEP 50) scalar promotion, the NumPy of
 * this image: 1050.0f / b[3] in infer_boundary and the float32-row arithmetic of the solvers' box-size tests, start
 * disparity and kpt2alpha ratio are evaluated in float32, as numpy 2 does for python-scalar (op) float32.  Under the
 * reference's own era (numpy 1.x value-based casting) those four expressions are float64; tie cases of depth < pixel and
 * the Newton-CG start point then differ in last bits -- srcnn_solve_4dof_host(..., boxes_are_float32 = 0) gives that
 * arithmetic for the solver. */
SRCNN_API size_t srcnn_box3d_workspace_bytes(int n, int im_w);
SRCNN_API int srcnn_infer_boundary(float *rec, int n, int rec_cols, int im_w, void *workspace, size_t workspace_bytes,
                         srcnn_stream_t stream);
SRCNN_API int srcnn_solve_4dof(float *rec, int n, int rec_cols, int im_h, int im_w, double p2_00, double p2_02, double p2_12,
                     double p2_03_minus_p3_03, float eval_thresh, double *state4, srcnn_stream_t stream);
SRCNN_API int srcnn_solve_4dof_scalar(float *rec, int n, int rec_cols, int im_h, int im_w, double p2_00, double p2_02, double p2_12,
                     double p2_03_minus_p3_03, float eval_thresh, double *state4, srcnn_stream_t stream);
SRCNN_API int srcnn_align_inputs(const float *rec, int n, int rec_cols, float *boxes, float *borders, float *poses, float *valid,
                       srcnn_stream_t stream);
SRCNN_API int srcnn_solve_3dof(float *rec, int n, int rec_cols, int im_h, int im_w, double p2_00, double p2_02, double p2_12,
                     double p2_03_minus_p3_03, const float *align_status, const float *best_dis, double *state,
                     srcnn_stream_t stream);
SRCNN_API int srcnn_solve_3dof_scalar(float *rec, int n, int rec_cols, int im_h, int im_w, double p2_00, double p2_02, double p2_12,
                     double p2_03_minus_p3_03, const float *align_status, const float *best_dis, double *state,
                     srcnn_stream_t stream);
/* Record forms on HOST memory (pinned copies of `rec` / `state`): row for row the function the two kernels above run, built
 * for the host and using the host's libm, i.e. bit-identical to the reference's scipy path (scipy Newton-CG, numpy scalar
 * `**2` = pow, glibc cos / sin / atan2).  Rows are spread over host threads: one per 8 rows, at most 16, and at most `threads` when > 0
 * (a budget, not a demand: creating 16 threads for 40 rows costs more than the rows). */
SRCNN_API int srcnn_solve_4dof_records_host(float *rec, int n, int rec_cols, int im_h, int im_w, double p2_00, double p2_02,
                                  double p2_12, double p2_03_minus_p3_03, float eval_thresh, double *state4, int threads);
SRCNN_API int srcnn_solve_3dof_records_host(float *rec, int n, int rec_cols, int im_h, int im_w, double p2_00, double p2_02,
                                  double p2_12, double p2_03_minus_p3_03, const float *align_status, const float *best_dis,
                                  double *state, int threads);
/* the same solver code compiled for the host (HOST pointers, no GPU needed): the reference's
 * solve_x_y_z_theta_from_kpt(im_shape, calib, alpha, dim, box_left, box_right, kpts) -> (status, state) and
 * solve_x_y_theta_from_kpt(im_shape, calib, alpha, dim, box_left, disparity, kpts) -> (state, z), flattened.
 * newton_status (may be NULL): scipy's OptimizeResult.status (0 ok, 1 maxiter, 2 line search, 3 CG / NaN), -1 = early-out. */
SRCNN_API int srcnn_solve_4dof_host(int im_h, int im_w, double p2_00, double p2_02, double p2_12, double p2_03_minus_p3_03,
                          double alpha, const double *dim3, const double *box_left4, const double *box_right4,
                          const double *kpts5, double *state4, int *newton_status,
                          int boxes_are_float32 /* the boxes hold float32 values the reference's numpy evaluates in float32
                                                   (box-size early-outs, start disparity); the device kernels always do */);
                          /* returns status 0 / 1 */
SRCNN_API int srcnn_solve_3dof_host(int im_h, int im_w, double p2_00, double p2_02, double p2_12, double p2_03_minus_p3_03,
                          double alpha, const double *dim3, const double *box_left4, double disparity,
                          const double *kpts5, double *state3, double *z, int *newton_status);
/* cost and the reference's (non-)gradient of either problem at (x, y, z, theta): box_right4 NULL = the 3-DoF terms */
SRCNN_API int srcnn_solver_evaluate_host(int im_h, int im_w, double p2_00, double p2_02, double p2_12,
                               double p2_03_minus_p3_03, double alpha, const double *dim3, const double *box_left4,
                               const double *box_right4_or_null, const double *kpts5, const double *xyzt, double *cost,
                               double *grad4);

/* ------------------------------------------------------------------ training losses
 * The six loss terms of Stereo R-CNN as two kernel families, each a forward and a backward:
 *   srcnn_cross_entropy  rpn_loss_cls (stereo_rpn.py:113-119: nonzero + index_select + F.cross_entropy), RCNN_loss_cls
 *                        (stereo_rcnn.py:287) and the keypoint / left-border / right-border terms (stereo_rcnn.py:292-310);
 *   srcnn_smooth_l1      _smooth_l1_loss (net_utils.py:79-99) for rpn_loss_box_left_right, RCNN_loss_bbox and
 *                        RCNN_loss_dim_orien, with the torch.gather by rois_label (stereo_rcnn.py:274-280) folded in.
 * Nothing is read back to the host: the ignore rule, the `sum(w) < 1` rule and the slice selection run on the device, the
 * backward takes the upstream gradient and the normaliser from device memory.  All tensors float32, labels / selectors int32.
 *
 * DEFINED SUMMATION ORDER (no atomics; results are run-to-run bit-equal).  Stage 1: workgroup b (256 threads) owns rows
 * [b * SRCNN_LOSS_ROWS_PER_WG, (b + 1) * SRCNN_LOSS_ROWS_PER_WG) -- a compile-time constant, independent of the device.  A
 * thread adds its terms in ascending row order starting from 0 (cross-entropy: at most 4 rows; smooth L1: local elements
 * t, t + 256, .. of the workgroup's rows x D block, as 4 groups of D consecutive ones, each group added from 0 and the 4 group
 * sums added from 0); a wavefront adds its 64 lanes by an xor butterfly (offsets 32, 16, 8, 4, 2, 1); thread 0 adds the four
 * wavefront sums ((w0 + w1) + w2) + w3 and writes the pair {sum, normaliser sum} to workspace[b].  Stage 2: one workgroup;
 * thread t adds workspace[t], workspace[t + 256], .. in that order from 0, then the same butterfly and four-term sum; thread 0
 * divides and writes *loss_out and *norm_out.  Which cross-entropy row a lane adds: cols == 2, rows t, t + 256, t + 512, t + 768 of the
 * workgroup; otherwise a row lies on lpr = min(64, max(2, cols rounded up to a power of two)) adjacent lanes, pass p of the
 * workgroup takes rows p * (256 / lpr) + (t / lpr), and lane p mod lpr of the row's lanes adds it.
 *
 * srcnn_cross_entropy: logits (rows, cols) with row stride `row_stride` >= cols floats, 1 <= cols <= SRCNN_CE_MAX_COLS.  The loss
 * of a row is log(sum_c exp(x_c - m)) + (m - x_label), m the row maximum (logits of magnitude 1e4 stay finite), the logarithm
 * taken as log1p of the terms other than the first maximum's.  A row is KEPT when 0 <= label < cols; every other label (-1, the
 * RPN's "don't care", or anything else out of range) is ignored and never used as an index: the row contributes to no sum.
 * With w_i = weights[i] (1 where weights is NULL), S = sum over kept rows of loss_i w_i and N = sum over kept rows of w_i:
 *   SRCNN_CE_MEAN_KEPT  loss = S / N   (weights NULL: the mean over the kept rows; *norm_out = N, the kept count)
 *   SRCNN_CE_WEIGHTED   loss = S if N < 1, else S / N   (the comparison is made on the device; *norm_out = N)
 * DELIBERATE DIFFERENCE from the reference: when no row is kept (or N = 0) the loss is 0 and the gradient all zeros, where
 * F.cross_entropy over an empty selection gives NaN or raises.  rows == 0 succeeds and writes loss 0.
 * srcnn_cross_entropy_backward: grad_logits (rows, cols) with row stride grad_stride >= cols; columns [0, cols) of EVERY row are
 * written (zeros for ignored rows; the caller need not zero it, and floats between cols and the stride are left alone):
 *   (softmax(x)_c - [c == label]) * w_i * (*grad_loss / n),  n = the forward's divisor rebuilt from *norm (1 where it did not divide).
 *
 * srcnn_smooth_l1: pred (rows, n_sel * D), target (rows, D), 1 <= D <= SRCNN_SMOOTH_L1_MAX_D, 1 <= n_sel <= SRCNN_SMOOTH_L1_MAX_SEL.
 * selector NULL (then n_sel must be 1): row r uses pred[r, 0:D]; otherwise its slice [sel[r] * D, sel[r] * D + D), and a row
 * whose selector lies outside [0, n_sel) contributes nothing and indexes nothing.  w_in / w_out: NULL (= 1), (rows, D), or with
 * *_per_row != 0 one weight per row (rows) -- the RPN's per-anchor weight, never expanded to 6 columns.  With
 * d = w_in * (pred - target) and t = (float)(1.0 / sigma^2) an element is   0.5 sigma^2 d^2  where |d| < t (strictly),
 * |d| - 0.5 / sigma^2  otherwise, times w_out; loss = (sum over all elements) / divisor.  The divisor is the caller's: it carries the
 * reference's sum-over-`dim`-then-.mean() rule ((B, A, 6) with dim=[1] gives B * 6, not B * A).  *norm_out = divisor.
 * srcnn_smooth_l1_backward: every element of grad_pred (rows, n_sel * D) is written (zeros in the slices the selector does not
 * pick):  sigma^2 d w_in w_out (*grad_loss / *norm)  on the quadratic branch,  sign(d) w_in w_out (*grad_loss / *norm)  on the linear one.
 *
 * Errors (SRCNN_ERR_ARG / SRCNN_ERR_WORKSPACE, before any launch): a null required pointer, rows < 0, cols / D / n_sel out of
 * range, a stride smaller than cols, sigma <= 0, divisor <= 0, a workspace smaller than srcnn_loss_workspace_bytes(rows). */
#define SRCNN_LOSS_ROWS_PER_WG 1024
#define SRCNN_CE_MAX_COLS 256
#define SRCNN_CE_MEAN_KEPT 0
#define SRCNN_CE_WEIGHTED 1
#define SRCNN_SMOOTH_L1_MAX_D 64
#define SRCNN_SMOOTH_L1_MAX_SEL 1024
SRCNN_API size_t srcnn_loss_workspace_bytes(long long rows);
SRCNN_API int srcnn_cross_entropy(const float *logits, long long rows, int cols, long long row_stride, const int *labels,
                        const float *weights, int mode, float *loss_out, float *norm_out, void *workspace,
                        size_t workspace_bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_cross_entropy_backward(const float *logits, long long rows, int cols, long long row_stride, const int *labels,
                                 const float *weights, int mode, const float *norm, const float *grad_loss,
                                 float *grad_logits, long long grad_stride, srcnn_stream_t stream);
SRCNN_API int srcnn_smooth_l1(const float *pred, const int *selector, int n_sel, const float *target, const float *w_in,
                    int w_in_per_row, const float *w_out, int w_out_per_row, long long rows, int D, float sigma, float divisor,
                    float *loss_out, float *norm_out, void *workspace, size_t workspace_bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_smooth_l1_backward(const float *pred, const int *selector, int n_sel, const float *target, const float *w_in,
                             int w_in_per_row, const float *w_out, int w_out_per_row, long long rows, int D, float sigma,
                             const float *norm, const float *grad_loss, float *grad_pred, srcnn_stream_t stream);

/* ------------------------------------------------------------------ training target layers
 * srcnn_anchor_targets    _AnchorTargetLayer.forward (lib/model/rpn/anchor_target_layer.py:64-154),
 * srcnn_proposal_targets  _ProposalTargetLayer.forward (lib/model/rpn/proposal_target_layer.py:36-333),
 * both without a host read: every count the reference reads back (nonzero, sum(keep) > 0, sum_fg[i] > num_fg, union1d
 * through .cpu()) stays on the device.  Floats are float32, labels / selections int32.
 *
 * RANDOMNESS IS AN INPUT.  The reference samples with np.random.permutation / np.random.rand; here the caller passes the draws.
 *   without replacement (anchor fg, anchor bg, proposal fg): one uint32 key per candidate slot; candidates are ranked by
 *     (key, index), the lower index winning a tie.  The anchor layer keeps the `quota` lowest-ranked candidates and sets the
 *     other ones to -1; the proposal layer's output row j of the foreground block is the candidate of rank j.
 *   with replacement (proposal bg, and the fg-only / bg-only branches of proposal_target_layer.py:262-283): one float64
 *     u[b, r] in [0, 1) per OUTPUT ROW r; row r takes the candidate whose position in ascending index order is
 *     floor(u[b, r] * count), the product in double as numpy forms it (rows of the without-replacement block ignore their u).
 *
 * IoU (bbox_overlaps_batch, bbox_transform.py:230-305) is evaluated as separately rounded float32 operations in the
 * reference's order -- no contraction, correctly rounded division -- with its zero-area masks (a ground-truth row with
 * w == 1 && h == 1 gives 0, such an anchor / roi gives -1): an overlap is bit-equal to torch's float32 CPU value, so
 * `overlaps == gt_max` (:91) means the same thing here.  The argmax is the FIRST maximum (lowest ground-truth index).  The only
 * floating reduction is a maximum (order-independent; integer atomics on the order-preserving bit pattern): results are
 * run-to-run bit-equal.  The regression targets follow bbox_transform_batch operation by operation; dw / dh go through the
 * device's logf, the one place where a last-bit difference from the CPU reference can appear.
 *
 * srcnn_anchor_targets: anchors (N, 4) as generate_anchors_all_pyramids gives them; gt_left / gt_right / gt_merge (B, K, 5)
 * zero-padded, K <= SRCNN_TARGETS_MAX_GT; im_info (B, 3) device, row 0 is used for every image as in the reference (:70-71);
 * fg_keys / bg_keys (B, N) uint32.  Steps in the reference's order: inside test x2 < (long)im_w, y2 < (long)im_h (anchors outside
 * take part in no maximum and come out as label -1, targets 0, weights 0: _unmap folded in); labels :88, :90-94 with
 * gt_max == 0 -> 1e-5, :97, clobber_positives choosing :88 or :100; sum_fg / sum_bg counted BEFORE any subsampling;
 * foreground kept to num_fg where sum_fg > num_fg; num_bg = batch_size - sum_fg (pre-subsample sum_fg, as the reference), background
 * kept to num_bg where sum_bg > num_bg, a negative num_bg disabling every background anchor; targets_left / targets_right from
 * gt_left / gt_right at the MERGED argmax, written for every inside anchor; inside_w = inside_weight on label 1; outside_w =
 * 1 / num_examples on labels 0 and 1, num_examples = the kept labels >= 0 of the LAST image of the batch (the `i` of :140 is
 * the loop's leftover; kept).  Outputs: labels (B, N) int32, targets_* (B, N, 4), inside_w / outside_w (B, N), and
 * max_overlaps (B, N), may be NULL: the merged maximum, -2 outside.  Four launches and one memset.
 *
 * srcnn_proposal_targets: rois_left / rois_right (B, R, 5), gt_left / gt_right (B, K, 5), gt_dim_orien (B, K, 5), gt_kpts
 * (B, K, 6), fg_keys (B, R + K) uint32, u (B, rois_per_image) float64; R + K <= SRCNN_TARGETS_MAX_ROIS, rois_per_image <=
 * SRCNN_TARGETS_MAX_BATCH_ROIS.  One workgroup per image: the ground-truth boxes are appended as rois R .. R+K-1 (:45-53); both
 * IoU matrices; foreground = left >= fg_thresh && right >= fg_thresh && the two argmax agree; background = in [bg_thresh_lo,
 * bg_thresh_hi) on the left OR the right, in index order (np.union1d); the four branches of :246-285 -- where the reference
 * raises (no foreground and no background) the image's outputs are all zero and status[b] = 1 (0 otherwise); gathers of
 * :291-310 (labels from gt_left[..., 4], rows past the foreground count 0; column 0 of the rois = b; dim_orien and kpts by the
 * LEFT assignment); box targets normalised by bbox_means / bbox_stds, dim_orien by dim_means / dim_stds; keypoint targets of
 * :168-192 (torch 0.3's round = HALF AWAY FROM ZERO, made explicit; -225 out of range; first maximum of the four keypoints;
 * type * grid + pos; weight 0 where negative); expansion of :77-138 (boxes / dim_orien for label > 0, keypoints for label == 1,
 * inside = inside_weights, outside = inside > 0).  The foreground ranking compares every pair of foreground candidates (at most
 * (R + K)^2 / 1024 LDS reads per thread).  Outputs: rois_left / rois_right (B, S, 5), labels (B, S) int32, bbox_targets_left /
 * _right (B, S, 4), dim_orien_targets (B, S, 5), kpts_targets (B, S, 3) int32, kpts_weight (B, S, 3), inside_w / outside_w
 * (B, S, 4), status (B) int32, keep_inds (B, S) int32 or NULL (the selected roi rows), S = rois_per_image.  One launch.
 *
 * Errors (SRCNN_ERR_ARG / SRCNN_ERR_WORKSPACE, before any launch): a null required pointer or params, B / N / R < 1 or K < 1,
 * K > SRCNN_TARGETS_MAX_GT, R + K or rois_per_image over their maxima, batch_size < 0, a quota (num_fg, fg_rois_per_image)
 * below 0 or above its batch size, kpts_grid < 1, a zero std, a workspace smaller than the matching *_workspace_bytes. */
#define SRCNN_TARGETS_MAX_GT 64
#define SRCNN_TARGETS_MAX_ROIS 4096
#define SRCNN_TARGETS_MAX_BATCH_ROIS 1024
typedef struct srcnn_anchor_target_params {
    float negative_overlap, positive_overlap;   /* cfg.TRAIN.RPN_NEGATIVE_OVERLAP / RPN_POSITIVE_OVERLAP */
    int clobber_positives;                      /* cfg.TRAIN.RPN_CLOBBER_POSITIVES */
    int batch_size;                             /* cfg.TRAIN.RPN_BATCHSIZE */
    int num_fg;                                 /* int(RPN_FG_FRACTION * RPN_BATCHSIZE) */
    float inside_weight;                        /* cfg.TRAIN.RPN_BBOX_INSIDE_WEIGHTS[0] */
} srcnn_anchor_target_params;
typedef struct srcnn_proposal_target_params {
    float fg_thresh, bg_thresh_hi, bg_thresh_lo;
    int rois_per_image, fg_rois_per_image;      /* cfg.TRAIN.BATCH_SIZE, int(round(FG_FRACTION * BATCH_SIZE)) */
    int kpts_grid;                              /* cfg.KPTS_GRID */
    float bbox_means[4], bbox_stds[4], dim_means[5], dim_stds[5], inside_weights[4];
} srcnn_proposal_target_params;
SRCNN_API size_t srcnn_anchor_targets_workspace_bytes(int B, int K);
SRCNN_API int srcnn_anchor_targets(const float *anchors, int N, const float *gt_left, const float *gt_right, const float *gt_merge,
                         int B, int K, const float *im_info, const unsigned *fg_keys, const unsigned *bg_keys,
                         const srcnn_anchor_target_params *params, int *labels, float *targets_left, float *targets_right,
                         float *inside_w, float *outside_w, float *max_overlaps, void *workspace, size_t workspace_bytes,
                         srcnn_stream_t stream);
SRCNN_API size_t srcnn_proposal_targets_workspace_bytes(int B, int R, int K);
SRCNN_API int srcnn_proposal_targets(const float *rois_left, const float *rois_right, int B, int R, const float *gt_left,
                           const float *gt_right, const float *gt_dim_orien, const float *gt_kpts, int K, const unsigned *fg_keys,
                           const double *u, const srcnn_proposal_target_params *params, float *out_rois_left, float *out_rois_right,
                           int *labels, float *bbox_targets_left, float *bbox_targets_right, float *dim_orien_targets,
                           int *kpts_targets, float *kpts_weight, float *inside_w, float *outside_w, int *status, int *keep_inds,
                           void *workspace, size_t workspace_bytes, srcnn_stream_t stream);

/* ------------------------------------------------------------------ training: optimiser step
 * clip_gradient (lib/model/utils/net_utils.py:37-49) and torch.optim.SGD with momentum as trainval_net.py:158-168, 224-227
 * uses it (dampening 0, no Nesterov), over a LIST of tensors per call.  The reference takes one norm per parameter, reads the
 * total back to the host, scales every gradient in a second pass and then makes four more passes over parameters, gradients
 * and momentum buffers; here one pass reads the gradients for the norm and one pass reads p, g, m and writes p, m, the clip
 * coefficient staying on the device.  Nothing is read back, nothing is uploaded: the lists are HOST arrays (device pointers,
 * element counts, per-tensor scalars) and travel in the kernels' argument blocks, at most SRCNN_OPT_TENSORS_PER_LAUNCH tensors per
 * launch, a longer list taking several launches.  All tensors are dense float32.  An entry with numel 0 is skipped (its pointers
 * may be NULL); every other pointer must be non-NULL and 4-byte aligned.  Tensors whose pointers are all 16-byte aligned are
 * read and written as float4, any other one element by element, with the same arithmetic and the same summation order.
 *
 * CHUNKS.  Tensor i is cut into ceil(numel[i] / SRCNN_OPT_CHUNK) chunks of SRCNN_OPT_CHUNK consecutive elements (the last one
 * shorter); the chunks of the whole list are numbered in list order, tensor 0's first.  One workgroup of 256 threads handles a
 * chunk at a time; the grid is min(chunks of the launch, 2048) workgroups which loop over the rest, and which workgroup takes
 * which chunk has no influence on any result.
 *
 * srcnn_grad_norm: out[0] = sqrt(sum over every listed element of g^2), out[1] = clip_norm / max(out[0], clip_norm) (exactly 1
 * where the norm does not exceed clip_norm), both float32 in device memory.  DEFINED SUMMATION ORDER (no atomics; the result
 * depends on the list and the data only, never on the grid, the device or the pointers' alignment).  Stage 1, float32: in chunk c
 * thread t owns the local elements 4 (256 j + t) + k, j = 0..3, k = 0..3; it adds their squares (each rounded once) in ascending
 * (j, k) order starting from 0, elements past the tensor's end adding nothing; a wavefront adds its 64 lanes by an xor butterfly
 * (offsets 32, 16, 8, 4, 2, 1); thread 0 adds the four wavefront sums ((w0 + w1) + w2) + w3 and writes workspace[c], c the
 * chunk's number in the whole list.  Stage 2, one workgroup, float64: thread t adds workspace[t], workspace[t + 256], .. in
 * ascending order starting from 0, then the same butterfly and four-term sum in double; thread 0 takes the square root in
 * double, rounds it to float32 and divides in float32.  A list without elements gives norm 0, coefficient 1.
 * workspace: srcnn_grad_norm_workspace_bytes(n_tensors, numel_host) bytes (one float per chunk), 0 for an invalid list.
 *
 * srcnn_grad_scale: g *= *coef for every listed tensor (one rounding per element) -- the in-place effect of the reference's
 * clip_gradient for callers that keep their own optimiser; srcnn_sgd_step does not need it.
 *
 * srcnn_sgd_step: per element, every float32 operation rounded once (no fused multiply-add), in this order
 *     d = clipped[i] && coef ? g * *coef : g
 *     d = weight_decay[i] != 0 ? d + weight_decay[i] * p : d
 *     m = first_step ? d : momentum * m + d          (momentum == 0: d is used directly, m_host and its entries may be NULL)
 *     p = p - lr[i] * m
 * p and m are updated in place, g is only read.  first_step != 0 says that the momentum buffers are uninitialised: they are
 * written and not read.  coef: NULL (nothing is clipped) or a device float, e.g. out + 1 of srcnn_grad_norm on the same stream.
 * clipped_host: NULL = every tensor is clipped.  Tensors must not overlap.
 *
 * Errors (SRCNN_ERR_ARG / SRCNN_ERR_WORKSPACE, before any launch): a null array, n_tensors <= 0, a negative numel, more than
 * 2^31 - 1 chunks, a NULL or misaligned p / g / m entry of a tensor with elements (m only when momentum != 0), momentum < 0 or
 * not finite, clip_norm <= 0, a null out / coef where required, a workspace smaller than srcnn_grad_norm_workspace_bytes. */
#define SRCNN_OPT_CHUNK 4096
#define SRCNN_OPT_TENSORS_PER_LAUNCH 64
SRCNN_API size_t srcnn_grad_norm_workspace_bytes(int n_tensors, const long long *numel_host);
SRCNN_API int srcnn_grad_norm(const float *const *g_host, const long long *numel_host, int n_tensors, float clip_norm, float *out,
                    void *workspace, size_t workspace_bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_grad_scale(float *const *g_host, const long long *numel_host, int n_tensors, const float *coef,
                     srcnn_stream_t stream);
SRCNN_API int srcnn_sgd_step(float *const *p_host, const float *const *g_host, float *const *m_host, const long long *numel_host,
                   const float *lr_host, const float *weight_decay_host, const int *clipped_host, int n_tensors, float momentum,
                   int first_step, const float *coef, srcnn_stream_t stream);

/* ------------------------------------------------- training: optimiser step over accumulated gradients, skipped when not finite
 * srcnn_sgd_step forms g * coef; one Inf or NaN in any gradient makes the norm Inf or NaN, the coefficient 0 or NaN and the
 * product NaN on that element: parameter and momentum buffer are lost for good, and nothing reads the device to notice.  The pair
 * below is srcnn_grad_norm + srcnn_sgd_step with two additions: every gradient enters multiplied by the host float grad_scale
 * (1 / N after N backward passes have summed into .grad: the update of the mean gradient), and the update is predicated on a
 * DEVICE word that says whether the norm is finite.  Nothing is read back.
 *
 * Every convention is that of "training: optimiser step" above: HOST arrays of device pointers and long long numels, an
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

/* ------------------------------------------------------------------ weight preparation
 * What engine.prep_conv / prep_conv_shortcut / prep_stem / prep_deconv2x2 / prep_linear_stack, ConvW.split_f16x3 and
 * engine.head_fragments do with eager torch ops, for a LIST of layers in one call, on the device, into destinations the caller
 * supplies: the in-place refresh of an inference plan's weights from live (trained) parameters.  The descriptors are a HOST
 * array and travel in the kernels' argument blocks (at most SRCNN_PREP_LAYERS_PER_LAUNCH layers per launch): nothing is
 * uploaded, nothing is read back.  Every result is bit-equal to the eager path's.
 *
 * Per layer, sources float32 in nn.Module layout:
 *   SRCNN_PREP_CONV       n_src (1..3) weights (cout[s], cin, kh, kw), concatenated along Cout (the RPN head, the stacked box
 *                         heads; nn.Linear is kh = kw = 1) -> dst_w (sum cout, kh, kw, cin); dst_b = the sources' biases (all or
 *                         none), or the folded BN's (n_src == 1 only)
 *   SRCNN_PREP_SHORTCUT   w[0] (cout, cin, 1, 1) with BN 0 and w[1] (cout, cin2, 1, 1) with BN 1 -> dst_w (cout, cin + cin2)
 *                         = [conv3 | downsample] along K; dst_b = float32(float64(b'0) + float64(b'1))
 *   SRCNN_PREP_STEM       w[0] (cout, 3, 7, 7) with BN 0 -> dst_w (cout, 7 row taps, 8 pixels, 4): element (co, kh, p, c) =
 *                         w'(co, c, kh, p) for p < 7 and c < 3, zero otherwise (the zeros are written)
 *   SRCNN_PREP_DECONV2X2  w[0] (cin, cout, 2, 2), b[0] (cout) -> dst_w (4 cout, cin), rows ordered (i, j, co); dst_b = b[0]
 * Frozen BN (bn_g / bn_b / bn_m / bn_v = weight, bias, running_mean, running_var; all NULL = none), float64, each operation
 * rounded once, never contracted:  s = g / sqrt(v + 1e-5),  w' = float32(w s),  b' = float32(beta - mean s).
 * m = max |w'| over the layer (a NaN wins, as in torch.max); k = floor(log2(16384 / m)) taken from m's exponent and mantissa,
 * 0 for m == 0 or a non-finite m; k_out[i] = k (device int32, one per layer of the list).  With dst_hi / dst_lo (float16, the
 * shape of dst_w): hi = f16(w' 2^k), lo = f16(w' 2^k - hi), round to nearest even.  With dst_frag (1x1, cin % 16 == 0; frag_rows
 * = rows rounded up to a multiple of 8): the fused head's fragment layout (cin / 16, 2, 2, frag_rows, 8) of the same hi / lo,
 * element (s, h, g, n, i) = W_h[n][16 s + 8 g + i], rows past Cout zero.
 * alias_of >= 0: this layer shares dst_w / dst_b (and so m and k) with the EARLIER layer alias_of of the list, which writes
 * them; the layer itself only writes its own dst_hi / dst_lo / dst_frag (two ConvW over one weight tensor).  -1 otherwise.
 * Every destination element is written exactly once (pass uninitialised buffers); no float atomics: the max is an integer max
 * of bit patterns, the same on every run.  The workspace holds one word per layer.
 *
 * Errors (SRCNN_ERR_ARG with "layer i: reason" in srcnn_last_error(), before any launch): a null array / k_out / workspace /
 * dst_w / source, an unknown form, sizes that do not fit the form ("size mismatch", kernel size, cin2, n_src), half of a BN,
 * hi without lo, misaligned pointers, a layer of 2^31 elements or more; SRCNN_ERR_WORKSPACE: a workspace smaller than
 * srcnn_prep_weights_workspace_bytes. */
#define SRCNN_PREP_LAYERS_PER_LAUNCH 16
#define SRCNN_PREP_CONV 0
#define SRCNN_PREP_SHORTCUT 1
#define SRCNN_PREP_STEM 2
#define SRCNN_PREP_DECONV2X2 3
typedef struct srcnn_prep_layer {
    int form, n_src, kh, kw, cin, cin2;
    int cout[3];
    int frag_rows, alias_of, pad_;
    const float *w[3], *b[3];
    const float *bn_g[2], *bn_b[2], *bn_m[2], *bn_v[2];
    float *dst_w, *dst_b;
    void *dst_hi, *dst_lo, *dst_frag;
} srcnn_prep_layer;
SRCNN_API size_t srcnn_prep_weights_workspace_bytes(int n_layers);
SRCNN_API int srcnn_prep_weights(const srcnn_prep_layer *layers_host, int n_layers, int *k_out, void *workspace,
                       size_t workspace_bytes, srcnn_stream_t stream);

/* ------------------------------------------------------------------ training: batch assembly
 * The per-iteration half of the reference's data loader (lib/roi_data_layer/minibatch.py, roibatchLoader.py:72-110,
 * lib/model/utils/blob.py), for a whole batch of at most SRCNN_LOADER_MAX_BATCH slots per launch.  The per-slot descriptions
 * are HOST arrays and travel in the kernels' argument blocks: nothing is uploaded, nothing is read back.  Both kernels write
 * every output element exactly once (pass uninitialised buffers) and use no atomics.
 *
 * srcnn_gt_batch.  `table`: the roidb packed once into device memory, SRCNN_GT_COLS float32 per object:
 *     [0..3] left box, [4..7] right box, [8..11] merge box (x1 y1 x2 y2, unscaled), [12..14] dim w h l, [15] sin(alpha),
 *     [16] cos(alpha) (taken on the host at packing time, as minibatch.py:68-69 takes them on every call), [17..22] kpts, [23] class.
 * Slot b describes rows [row_begin, row_begin + n) of it, the image's float32 im_scale and its blob width im_width;
 * keys[b * key_stride + c] is the uint32 shuffle key of the slot's row c (device memory, n <= key_stride).  Per row, float32,
 * each operation rounded once:  box = table box * im_scale, x1 = min(x1, im_width), column 4 = class (three box sets);
 * dim_orien = (w, h, l, sin, cos) as stored;  kpt = table kpt * im_scale, replaced by -1 where kpt < 0 or kpt > im_width - 1.
 * Row c goes to output row rank(c) = #{d : (key[d], d) < (key[c], c)} (srcnn_proposal_targets' convention: equal keys rank
 * by index) -- np.random.shuffle as a sort by key; only ranks < min(n, K) are kept (truncation AFTER the shuffle,
 * roibatchLoader.py:83-107), every other output row is zero.  Outputs: gt_left / gt_right / gt_merge / gt_dim_orien (B, K, 5),
 * gt_kpts (B, K, 6), num_boxes (B) int64 = min(n, K).  One workgroup per slot ranks its keys in LDS: n is at most
 * SRCNN_GT_MAX_ROWS, a larger entry is refused.
 *
 * srcnn_preprocess_train.  Slot b: the decoded uint8 RGB left / right images (H, W, 3) (device memory, or page-locked host
 * memory read where it is), `flipped`, and `scale` (target size / short side, double).  Writes out_left / out_right, float32
 * (B, 3, Hmax, Wmax): per pixel RGB -> BGR, minus PIXEL_MEANS (in double, stored as float32), cv2.resize(fx = fy = scale,
 * INTER_LINEAR) exactly as srcnn_preprocess does it, output size OH = cvRound(H * scale), OW = cvRound(W * scale); columns >=
 * min(OW, max_size) (blob.py:59-61) and rows >= OH of a slot are zero (blob.py:20-37).  flipped != 0 (minibatch.py:116-119): the
 * left output is the RIGHT source read mirrored (column W - 1 - x) and the right output the left source mirrored; the mirror
 * applies to the source index, before the mean and the resize.  Every slot needs OH <= Hmax and min(OW, max_size) <= Wmax;
 * the outputs must be 16-byte aligned (a thread stores four consecutive floats of the flat blob) and a blob has fewer than 2^31
 * elements.
 *
 * Errors (SRCNN_ERR_ARG, before any launch): a null array / output / image, B outside 1..SRCNN_LOADER_MAX_BATCH, K <= 0, a
 * negative or out-of-table row range, n > SRCNN_GT_MAX_ROWS or > key_stride, a non-positive or non-finite scale, a null table
 * or keys when any slot has rows, a resized image larger than (Hmax, Wmax), misaligned outputs, a blob of 2^31 elements or more. */
#define SRCNN_LOADER_MAX_BATCH 16
#define SRCNN_GT_COLS 24
#define SRCNN_GT_MAX_ROWS 512
typedef struct srcnn_gt_slot {
    int row_begin, n;            /* rows [row_begin, row_begin + n) of the table */
    float im_scale;              /* float32(target size / short side) */
    float im_width;              /* the image's blob width: min(OW, max_size) */
} srcnn_gt_slot;
typedef struct srcnn_train_image {
    const unsigned char *left, *right;   /* decoded uint8 RGB (H, W, 3) */
    int H, W;
    int flipped;
    double scale;
} srcnn_train_image;
SRCNN_API int srcnn_gt_batch(const float *table, int table_rows, const srcnn_gt_slot *slots_host, int B, const unsigned *keys,
                   int key_stride, int K, float *gt_left, float *gt_right, float *gt_merge, float *gt_dim_orien, float *gt_kpts,
                   long long *num_boxes, srcnn_stream_t stream);
SRCNN_API int srcnn_preprocess_train(const srcnn_train_image *slots_host, int B, int Hmax, int Wmax, int max_size, float *out_left,
                           float *out_right, srcnn_stream_t stream);

/* ------------------------------------------------------------------ result visualisation
 * The picture the reference's demo.py:225-333 / test_net.py:231-339 show, drawn on the device from one image's detection record
 * (see srcnn_pack_detections) with no host read of a detection: the left image over the right image with the 2-D boxes
 * (net_utils.vis_detections), the projected 3-D wireframes on the left image (vis_3d_utils.vis_single_box_in_img) and, to the
 * right of both, a bird's-eye view of the lidar points with the 3-D boxes (vis_lidar_in_bev, vis_box_in_bev).  Everything up to
 * the integer pixel coordinates follows the reference -- which objects are drawn, their end points, the integer conversions,
 * colours, thicknesses, panel sizes and layout.  The RASTERISATION RULE below is this project's own definition: OpenCV's
 * cv2.line is not available to compare with, so pixel equality with OpenCV is NOT claimed.
 *
 * srcnn_render_overlay.  left / right: uint8 RGB (H, W, 3); rec: (max_det + 1, SRCNN_REC_COLS); p2_host: the 3x4 P2, 12 host
 * doubles, row-major; bev_plane: uint8 (y_max, x_max) gray plane as srcnn_bev_lidar writes it, or NULL = all white (255); panel:
 * uint8 RGB (2 H, W + x_max, 3) -- rows [0, H) x columns [0, W) the left image, rows [H, 2 H) the right image, columns
 * [W, W + x_max) the bird's-eye view (x_max == 0: no such columns; otherwise y_max must equal 2 H, as the reference's
 * np.concatenate needs).  res, x_max, y_max, x_off, y_off are the reference's float64 host values for width = 2 H:
 * res = 70.0 / width, x_max = int(40 / res), y_max = int(70 / res), x_off = int(floor(-20 / res)), y_off = int(floor(70 / res)) - 1.
 * With count = the record's row 0 column 0 (clamped to [0, max_det]) and row r the r-th detection:
 *   2-D boxes (layer 1): rows r < min(100, count) with score > vis_thresh: the left box on the left image and the right box on
 *     the right image, each four segments between the corners (rint(x1), rint(y1)), (rint(x2), rint(y2)), rint = float32
 *     round-half-even; RGB (204, 0, 0), thickness 1.
 *   wireframes (layer 2): rows r < count with alignment status (column 25) > 0 and score > vis_thresh; in float64, with
 *     (x, y, z, theta) = columns 27-30, (w, h, l) = columns 9-11, c = cos(theta), s = sin(theta): corner(a, b, d) =
 *     (x + (c a + s d) / 2, y + b / 2, z + (-s a + c d) / 2) for (a, b, d) = (-w, 0, -l), (-w, 0, l), (w, 0, l), (w, 0, -l) and the same
 *     four with b = -2 h; pixel = (trunc(u / n), trunc(v / n)) with (u, v, n) = P2[:, 0:3] . corner, each sum left to right.  A
 *     box with ANY corner at z < 0 is skipped whole.  Edges 0-1 1-2 2-3 0-3, 4-5 5-6 6-7 7-4, 4-0 5-1 6-2 7-3; RGB (0, 200, 0),
 *     thickness 1, on the left image.
 *   bird's-eye boxes (layer 4): the same rows; points 0-3 = the four corners with b = 0, point 4 = (x + s t, y, z + c t) with
 *     t = l * 2 / 3; pixel = (trunc(X / res) - x_off, trunc(-Z / res) + y_off); edges 0-1 1-2 2-3 0-3 1-4 2-4; RGB (0, 200, 0),
 *     thickness 2.
 * `layers`: the sum of the layers to draw (7 = all).  Every coordinate is clamped to [-2^30, 2^30] (NaN -> -2^30) before its
 * conversion to an integer, and all line arithmetic is 64-bit: a corner near z -> 0+ projects arbitrarily far away.
 * Draw order, later wins: image pixels, 2-D boxes in record order, wireframes in record order; on the bird's-eye view the plane,
 * then the boxes in record order.  An object drawn on one of the three targets never spills into another.
 *
 * RASTERISATION RULE.  A segment p0 -> p1 has adx = |x1 - x0|, ady = |y1 - y0|, sx = sign(x1 - x0), sy = sign(y1 - y0).  If
 * adx >= ady (x-major) its pixels are x = x0 + sx i, y = y0 + sy ((2 i ady + adx) / (2 adx)) for i = 0..adx, the division
 * rounding down; a zero-length segment is the single pixel p0; the y-major case (adx < ady) is the same with x and y exchanged.
 * Thickness t stamps, at each such pixel, the offsets dx, dy in [-(t / 2), (t - 1) / 2] (integer division).  Pixels outside the
 * target rectangle are dropped.  The rule is a closed-form membership test: the kernel is a gather -- a thread owns pixels,
 * walks the segments whose bounding box meets its tile and keeps the last one that covers the pixel -- so every panel byte is
 * written exactly once, without atomics, and the panel does not depend on the launch geometry (`rows_per_thread`: 1, 2, 4 or
 * 8 pixel rows per thread, 0 = the default; a tile is 64 x 4 rows_per_thread pixels).
 * workspace: srcnn_overlay_workspace_bytes(max_det) bytes, the segment list (26 slots per record row).
 *
 * srcnn_bev_lidar.  kitti_utils.get_point_cloud without its image crop + vis_3d_utils.vis_lidar_in_bev:53-66.  points: n_points
 * x (x, y, z, intensity) float32, 16-byte aligned; velo_to_cam2_host: rows 0-2 of the reference's float64 product
 * T(t_cam2_cam0) . pad(R0_rect) . pad(Tr_velo_to_cam), 12 host doubles.  Sets the whole (y_max, x_max) plane to 255, then per
 * point, float64: X = m00 x + m01 y + m02 z + m03 (left to right), Z likewise from row 2; kept when 0 < Z < 70 and -20 < X < 20;
 * x_img = trunc(X / res) - x_off, y_img = trunc(-Z / res) + y_off, each clamped from ABOVE only (x_max - 1, y_max - 1) as the
 * reference does; plane[y_img, x_img] = 100.  A negative index, which numpy would wrap to the other end of the plane, is
 * skipped: after the filter trunc(X / res) >= trunc(-20 / res) >= x_off and trunc(-Z / res) >= -floor(70 / res), so none occurs
 * for the geometry above.  Every store writes the same value, so plain stores are race-free in outcome.  n_points == 0 leaves the
 * plane white: what the reference shows without a lidar file (its single point at the origin is filtered out).
 *
 * Errors (SRCNN_ERR_ARG, before any HIP call): a null pointer (left, right, rec, p2_host, panel, workspace; plane,
 * velo_to_cam2_host, points when n_points > 0), H or W <= 0 or > 32768, max_det < 0 or > 4096, rec_cols != SRCNN_REC_COLS,
 * x_max < 0 or > 65536, |x_off| or |y_off| > SRCNN_OVERLAY_MAX_OFFSET (2^20: with the clamp and the panel sizes above every end
 * point stays inside 32 bits), x_max > 0 with y_max != 2 H, x_max or y_max <= 0 (srcnn_bev_lidar), a non-finite or non-positive res,
 * layers outside 0..7, rows_per_thread not one of 0, 1, 2, 4, 8, a non-finite vis_thresh, n_points < 0, misaligned points, a
 * panel (plane) that overlaps one of the inputs; SRCNN_ERR_WORKSPACE: a workspace smaller than srcnn_overlay_workspace_bytes. */
#define SRCNN_OVERLAY_SLOTS_PER_ROW 26
#define SRCNN_OVERLAY_MAX_OFFSET 1048576
#define SRCNN_OVERLAY_BOXES 1
#define SRCNN_OVERLAY_WIREFRAMES 2
#define SRCNN_OVERLAY_BEV_BOXES 4
SRCNN_API size_t srcnn_overlay_workspace_bytes(int max_det);
SRCNN_API int srcnn_render_overlay(const unsigned char *left, const unsigned char *right, int H, int W, const float *rec,
                         int max_det, int rec_cols, const double *p2_host, float vis_thresh, const unsigned char *bev_plane,
                         double res, int x_max, int y_max, int x_off, int y_off, int layers, int rows_per_thread,
                         unsigned char *panel, void *workspace, size_t workspace_bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_bev_lidar(const float *points, int n_points, const double *velo_to_cam2_host, double res, int x_max, int y_max,
                    int x_off, int y_off, unsigned char *plane, srcnn_stream_t stream);

/* ------------------------------------------------------------------ recorded launch programs
 * The forward is a fixed list of ~230 asynchronous launches over fixed buffers (one list per input size and buffer set).
 * Between srcnn_program_begin and srcnn_program_end every srcnn_* call made BY THE CALLING THREAD records its kernel
 * launches / memsets (function, geometry, stream, by-value arguments) into the program instead of launching them;
 * srcnn_program_run then re-issues the whole list from C on the streams it was recorded with, the main stream replaced by
 * the one given -- no Python frame, descriptor filling or plan lookup per launch.  Dependencies between streams are
 * recorded explicitly: record_event (returns an event id >= 0) on the producing stream, wait_event on the consuming one.
 * The caller keeps every buffer a recorded launch points at alive and unchanged in address (activations, weights,
 * workspaces).  Unlike a hipGraph the side-stream branches stay real concurrent streams at replay. */
SRCNN_API void *srcnn_program_create(void);
SRCNN_API void srcnn_program_destroy(void *prog);
SRCNN_API int srcnn_program_begin(void *prog, srcnn_stream_t main_stream);
SRCNN_API int srcnn_program_end(void *prog);
SRCNN_API int srcnn_program_recording(void);                        /* 1 while the calling thread records */
SRCNN_API int srcnn_program_record_event(void *prog, srcnn_stream_t stream);
SRCNN_API int srcnn_program_wait_event(void *prog, srcnn_stream_t stream, int event_id);
SRCNN_API int srcnn_program_size(void *prog);                       /* recorded nodes */
SRCNN_API int srcnn_program_run(void *prog, srcnn_stream_t main_stream);

/* ------------------------------------------------------------------ streams with their own hardware queue
 * HIP folds the streams of a process onto GPU_MAX_HW_QUEUES (default 4) hardware queues, least-used queue first.  Streams that
 * share a queue execute in submission order and an event wait of one of them holds up everything queued behind it -- with
 * several forwards in flight (one main stream + two side streams each) a side stream of forward A that waits for A's trunk
 * stalls the main stream of forward B that happens to share its queue (profiles/queue_mapping_r04.txt).  A stream created
 * here owns a hardware queue of its own (created with an all-ones CU mask: masked streams are never pooled), so that the
 * placement of the forwards' streams is the caller's decision, not an accident of creation order.
 * dedicated_queue = 0 gives an ordinary non-blocking stream from the shared pool. */
SRCNN_API int srcnn_stream_create(int dedicated_queue, srcnn_stream_t *stream);
/* The same with a caller-chosen CU mask (bit b of word b / 32 enables compute unit b of the device's enumeration; `words`
 * 32-bit words, at least one bit set in them): the kernels of this stream run on those CUs only.  The serving regime gives each
 * of S forwards in flight its own 1/S of every XCD's CUs (stereo_rcnn_amd/streams.py: partition_masks) -- a forward then never
 * shares a CU with another forward's kernels, and its launches meet a device of 256/S CUs that their tile counts fill. */
SRCNN_API int srcnn_stream_create_cu_mask(int words, const unsigned *mask, srcnn_stream_t *stream);
SRCNN_API int srcnn_stream_destroy(srcnn_stream_t stream);
/* Diagnostics: launches `blocks` one-wave workgroups on `stream`; block b writes its XCC_ID register to xcc[b] and its HW_ID
 * register (CU / shader-array / shader-engine fields) to hw_id[b] (device int arrays of `blocks` entries).  Shows where a
 * (masked) stream's workgroups actually run. */
SRCNN_API int srcnn_probe_placement(int blocks, int *xcc, int *hw_id, srcnn_stream_t stream);

/* ------------------------------------------------------------------ profiling hooks
 * When enabled, every conv-engine launch is bracketed by hipEvents on its stream; the
 * accumulated kernel time / algorithmic flops / launch count are read back with
 * srcnn_prof_read (which synchronises those events). Used by bench.py for `roofline`. */
SRCNN_API int srcnn_prof_enable(int on);
SRCNN_API int srcnn_prof_read(double *conv_ms, double *conv_flops, long long *conv_launches);
/* Per-launch form: elapsed ms of each recorded conv launch, in launch order, into ms[0..max) (same synchronisation);
 * returns the number of launches recorded (which may exceed max) or a negative error.  Does not reset the recording --
 * srcnn_prof_read / srcnn_prof_enable do.  Used by bench.py / tools/layer_table.py for the per-layer roofline table. */
SRCNN_API int srcnn_prof_read_launches(float *ms, int max);

/* ------------------------------------------------------------------ KITTI object evaluation
 * The device side of stereo_rcnn_amd/kitti_eval.py, a restatement of the KITTI object devkit's evaluation
 * (evaluate_object_3d_offline: cleanData / computeStatistics / eval_class).  A whole split is one ragged batch:
 * frame f owns detection rows [det_off[f], det_off[f+1]), ground-truth rows [gt_off[f], gt_off[f+1]) (DontCare rows
 * excluded) and don't-care rows [dc_off[f], dc_off[f+1]), each row SRCNN_KITTI_COLS doubles
 * [x1 y1 x2 y2 h w l x y z ry alpha score] (score unused for ground truth, only x1..y2 used for don't-care rows).
 * Overlap matrices are laid out per frame, ground-truth (or don't-care) major: frame f's det j x gt i overlap is
 * ov_*[pair_off[f] + i * n_det(f) + j] with pair_off[f+1] - pair_off[f] = n_gt(f) * n_det(f), and its det j x
 * don't-care k overlap is ov_dc[dcpair_off[f] + k * n_det(f) + j].  Everything is float64 with no "+1".
 * LIMIT: at most SRCNN_KITTI_MAX_DET detections per frame (max_det_per_frame is the caller's count of the largest
 * frame); a larger count returns SRCNN_ERR_ARG before anything is launched.  No workspace is needed. */
#define SRCNN_KITTI_COLS 13
#define SRCNN_KITTI_MAX_DET 4096
#define SRCNN_KITTI_SLOTS 41
typedef struct srcnn_kitti_split {
    int n_frames;
    int max_det_per_frame;
    const int *det_off, *gt_off, *dc_off;    /* (n_frames + 1) row offsets */
    const long long *pair_off, *dcpair_off;  /* (n_frames + 1) offsets into ov_img / ov_bev / ov_3d and ov_dc */
    const double *det, *gt, *dc;             /* rows of SRCNN_KITTI_COLS doubles */
    double *ov_img;                          /* 2-D IoU */
    double *ov_bev;                          /* rotated-rectangle IoU in the x-z plane */
    double *ov_3d;                           /* BEV intersection x height overlap (y is the bottom face), over the union volume */
    double *ov_dc;                           /* 2-D intersection over the DETECTION's area (devkit criterion 0) */
} srcnn_kitti_split;
/* Fills ov_img, ov_bev, ov_3d and ov_dc of every frame (one workgroup per frame).  Degenerate geometry (identical or
 * nested boxes, shared edges, zero extent, no contact) gives finite values; an empty union gives 0. */
SRCNN_API int srcnn_kitti_overlaps(const srcnn_kitti_split *split, srcnn_stream_t stream);
/* One match pass of computeStatistics over every (configuration c, threshold slot t, frame f): one wavefront per item,
 * detections across the lanes (64-wide chunks), every greedy choice a cross-lane reduction.  A configuration is a
 * (class, difficulty) flag set, a metric (0 image, 1 BEV, 2 3-D) and that metric's minimum overlap (strict >).
 * compute_fp = 0 (pass 1, n_slots must be 1): gt_score[c * n_gt_total + g] = the score of the detection ground truth g
 *   is a true positive with, -inf otherwise.
 * compute_fp = 1 (pass 2): detections scoring below thresholds[c * n_slots + t] are left out; tp / fp / fn (int) and
 *   similarity (double: sum over the frame's true positives, in ground-truth order, of (1 + cos(alpha_gt - alpha_det)) / 2;
 *   -1 when tp + fp == 0; 0 for the BEV and 3-D metrics) go to index (c * n_slots + t) * n_frames + f.  Slots
 *   t >= cfg_n_thresh[c] get zeros.  Results are deterministic: no atomics, fixed reduction order. */
typedef struct srcnn_kitti_match_desc {
    int n_cfg, n_slots, compute_fp;
    int n_gt_total, n_det_total;             /* gt_off[n_frames], det_off[n_frames] */
    const int *cfg_flags;                    /* (n_cfg) row of ign_gt / ign_det to use */
    const int *cfg_metric;                   /* (n_cfg) 0 / 1 / 2 */
    const double *cfg_min_overlap;           /* (n_cfg) */
    const int *cfg_n_thresh;                 /* (n_cfg) pass 2: thresholds in use, <= n_slots */
    const double *thresholds;                /* (n_cfg, n_slots) pass 2 */
    const signed char *ign_gt;               /* (flag sets, n_gt_total): cleanData's ignored_gt, 0 / 1 / -1 */
    const signed char *ign_det;              /* (flag sets, n_det_total): ignored_det, 0 / 1 / -1 */
    double *gt_score;                        /* pass 1 output */
    int *tp, *fp, *fn;                       /* pass 2 outputs */
    double *similarity;
} srcnn_kitti_match_desc;
SRCNN_API int srcnn_kitti_match(const srcnn_kitti_split *split, const srcnn_kitti_match_desc *match, srcnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SRCNN_HIP_H */
