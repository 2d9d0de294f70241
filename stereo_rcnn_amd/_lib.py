"""ctypes binding of libsrcnn_hip.so (the C-ABI drop-in boundary, include/srcnn_hip.h).

The reference binds its native ops with cffi (`torch.utils.ffi`,
lib/model/nms/_ext/nms/__init__.py:2-15); cffi is not in this image, ctypes gives the
same contract.  There is NO fallback: if the HIP library is missing or fails to load,
importing any operator raises (the product path never routes through the CPU oracle).
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRCNN_LIB_PATH") or os.path.join(_HERE, "libsrcnn_hip.so")   # override: A/B builds of the library (dev)

FMT_F32, FMT_SPLIT16 = 0, 1     # SRCNN_FMT_* (include/srcnn_hip.h)
REC_COLS = 32                   # SRCNN_REC_COLS: detection record row (include/srcnn_hip.h lists the columns)
LOSS_ROWS_PER_WG = 1024         # SRCNN_LOSS_ROWS_PER_WG: rows of one stage-1 workgroup of the loss kernels (one workspace partial each)
CE_MAX_COLS = 256               # SRCNN_CE_MAX_COLS
CE_MEAN_KEPT, CE_WEIGHTED = 0, 1    # SRCNN_CE_*
TARGETS_MAX_GT = 64             # SRCNN_TARGETS_MAX_GT
TARGETS_MAX_ROIS = 4096         # SRCNN_TARGETS_MAX_ROIS: proposals + ground-truth boxes of one image
TARGETS_MAX_BATCH_ROIS = 1024   # SRCNN_TARGETS_MAX_BATCH_ROIS: rois_per_image
OPT_CHUNK = 4096                # SRCNN_OPT_CHUNK: elements of one chunk of the optimiser kernels (one norm partial each)
OPT_TENSORS_PER_LAUNCH = 64     # SRCNN_OPT_TENSORS_PER_LAUNCH: tensors one launch of the optimiser kernels carries in its arguments
LOADER_MAX_BATCH = 16           # SRCNN_LOADER_MAX_BATCH: batch slots one launch of the batch assembly kernels carries in its arguments
GT_COLS = 24                    # SRCNN_GT_COLS: floats of one object row of the ground-truth table (include/srcnn_hip.h lists the columns)
GT_MAX_ROWS = 512               # SRCNN_GT_MAX_ROWS: objects of one roidb entry srcnn_gt_batch ranks
PREP_LAYERS_PER_LAUNCH = 16     # SRCNN_PREP_LAYERS_PER_LAUNCH: layers one launch of the weight preparation kernels carries in its arguments
PREP_CONV, PREP_SHORTCUT, PREP_STEM, PREP_DECONV2X2 = 0, 1, 2, 3     # SRCNN_PREP_*: the forms of srcnn_prep_weights
OVERLAY_SLOTS_PER_ROW = 26      # SRCNN_OVERLAY_SLOTS_PER_ROW: segments srcnn_render_overlay keeps per record row (8 + 12 + 6)
OVERLAY_BOXES, OVERLAY_WIREFRAMES, OVERLAY_BEV_BOXES = 1, 2, 4      # SRCNN_OVERLAY_*: the layers of srcnn_render_overlay

c_int, c_float, c_double, c_void_p, c_size_t = (ctypes.c_int, ctypes.c_float, ctypes.c_double,
                                                ctypes.c_void_p, ctypes.c_size_t)


class ConvDesc(ctypes.Structure):
    """struct srcnn_conv_desc (include/srcnn_hip.h)."""
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("residual", c_void_p), ("y", c_void_p),
                ("B", c_int), ("H", c_int), ("W", c_int), ("Cin", c_int), ("x_cstride", c_int),
                ("OH", c_int), ("OW", c_int), ("Cout", c_int),
                ("KH", c_int), ("KW", c_int), ("stride", c_int), ("pad", c_int),
                ("y_cstride", c_int), ("y_coffset", c_int), ("res_cstride", c_int),
                ("relu", c_int), ("mode", c_int),
                ("precision", c_int), ("w_lo", c_void_p), ("w_inv_scale", c_float),
                ("tile_mr", c_int), ("tile_nr", c_int), ("splits", c_int),
                ("x_format", c_int), ("y_format", c_int), ("res_format", c_int),
                ("tile_waves", c_int), ("tile_stages", c_int), ("layer_tag", c_int),
                ("m_limit", c_void_p), ("m_limit_mul", c_int),
                ("x2", c_void_p), ("Cin2", c_int), ("H2", c_int), ("W2", c_int), ("x2_cstride", c_int), ("stride2", c_int),
                ("head_w", c_void_p), ("head_bias", c_void_p), ("head_y", c_void_p), ("head_cout", c_int), ("head_scale", c_float),
                ("head_wf", c_void_p), ("head_rows", c_int), ("head_parts", c_int), ("head_plane", ctypes.c_longlong),
                ("up_top", c_void_p), ("up_format", c_int), ("up_H", c_int), ("up_W", c_int)]


class ConvBwdDesc(ctypes.Structure):
    """struct srcnn_conv_bwd_desc (include/srcnn_hip.h)."""
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("y", c_void_p), ("dy", c_void_p),
                ("dx", c_void_p), ("dw", c_void_p), ("db", c_void_p), ("g_out", c_void_p),
                ("B", c_int), ("H", c_int), ("W", c_int), ("Cin", c_int), ("x_cstride", c_int),
                ("OH", c_int), ("OW", c_int), ("Cout", c_int),
                ("KH", c_int), ("KW", c_int), ("stride", c_int), ("pad", c_int),
                ("y_cstride", c_int), ("y_coffset", c_int), ("relu", c_int),
                ("mode", c_int), ("precision", c_int), ("x_format", c_int), ("y_format", c_int),
                ("tile_mr", c_int), ("tile_nr", c_int), ("splits", c_int),
                ("head_w", c_void_p), ("head_wf", c_void_p), ("x2", c_void_p), ("up_top", c_void_p)]


class ConvFwdF16x3Desc(ctypes.Structure):
    """struct srcnn_conv_fwd_f16x3_desc (include/srcnn_hip.h)."""
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("residual", c_void_p), ("y", c_void_p),
                ("B", c_int), ("H", c_int), ("W", c_int), ("Cin", c_int), ("x_cstride", c_int),
                ("OH", c_int), ("OW", c_int), ("Cout", c_int),
                ("KH", c_int), ("KW", c_int), ("stride", c_int), ("pad", c_int),
                ("y_cstride", c_int), ("y_coffset", c_int), ("relu", c_int),
                ("x_format", c_int), ("y_format", c_int),
                ("tile_mr", c_int), ("tile_nr", c_int)]


class KittiSplit(ctypes.Structure):
    """struct srcnn_kitti_split (include/srcnn_hip.h): a ragged batch of frames, device pointers."""
    _fields_ = [("n_frames", c_int), ("max_det_per_frame", c_int),
                ("det_off", c_void_p), ("gt_off", c_void_p), ("dc_off", c_void_p),
                ("pair_off", c_void_p), ("dcpair_off", c_void_p),
                ("det", c_void_p), ("gt", c_void_p), ("dc", c_void_p),
                ("ov_img", c_void_p), ("ov_bev", c_void_p), ("ov_3d", c_void_p), ("ov_dc", c_void_p)]


class KittiMatchDesc(ctypes.Structure):
    """struct srcnn_kitti_match_desc (include/srcnn_hip.h): one match pass, device pointers."""
    _fields_ = [("n_cfg", c_int), ("n_slots", c_int), ("compute_fp", c_int), ("n_gt_total", c_int), ("n_det_total", c_int),
                ("cfg_flags", c_void_p), ("cfg_metric", c_void_p), ("cfg_min_overlap", c_void_p), ("cfg_n_thresh", c_void_p),
                ("thresholds", c_void_p), ("ign_gt", c_void_p), ("ign_det", c_void_p),
                ("gt_score", c_void_p), ("tp", c_void_p), ("fp", c_void_p), ("fn", c_void_p), ("similarity", c_void_p)]


class AnchorTargetParams(ctypes.Structure):
    """struct srcnn_anchor_target_params (include/srcnn_hip.h)."""
    _fields_ = [("negative_overlap", c_float), ("positive_overlap", c_float), ("clobber_positives", c_int),
                ("batch_size", c_int), ("num_fg", c_int), ("inside_weight", c_float)]


class ProposalTargetParams(ctypes.Structure):
    """struct srcnn_proposal_target_params (include/srcnn_hip.h)."""
    _fields_ = [("fg_thresh", c_float), ("bg_thresh_hi", c_float), ("bg_thresh_lo", c_float),
                ("rois_per_image", c_int), ("fg_rois_per_image", c_int), ("kpts_grid", c_int),
                ("bbox_means", c_float * 4), ("bbox_stds", c_float * 4), ("dim_means", c_float * 5), ("dim_stds", c_float * 5),
                ("inside_weights", c_float * 4)]


class GtSlot(ctypes.Structure):
    """struct srcnn_gt_slot (include/srcnn_hip.h)."""
    _fields_ = [("row_begin", c_int), ("n", c_int), ("im_scale", c_float), ("im_width", c_float)]


class TrainImage(ctypes.Structure):
    """struct srcnn_train_image (include/srcnn_hip.h)."""
    _fields_ = [("left", c_void_p), ("right", c_void_p), ("H", c_int), ("W", c_int), ("flipped", c_int), ("scale", c_double)]


class PrepLayer(ctypes.Structure):
    """struct srcnn_prep_layer (include/srcnn_hip.h)."""
    _fields_ = [("form", c_int), ("n_src", c_int), ("kh", c_int), ("kw", c_int), ("cin", c_int), ("cin2", c_int),
                ("cout", c_int * 3), ("frag_rows", c_int), ("alias_of", c_int), ("pad_", c_int),
                ("w", c_void_p * 3), ("b", c_void_p * 3),
                ("bn_g", c_void_p * 2), ("bn_b", c_void_p * 2), ("bn_m", c_void_p * 2), ("bn_v", c_void_p * 2),
                ("dst_w", c_void_p), ("dst_b", c_void_p), ("dst_hi", c_void_p), ("dst_lo", c_void_p), ("dst_frag", c_void_p)]


_SIGNATURES = {
    # name: (restype, argtypes)
    "srcnn_version": (c_int, []),
    "srcnn_last_error": (ctypes.c_char_p, []),
    "srcnn_nms_workspace_bytes": (c_size_t, [c_int]),
    "srcnn_nms": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_size_t, c_void_p]),
    "srcnn_nms_batched_workspace_bytes": (c_size_t, [c_int, c_int]),
    "srcnn_nms_batched": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                                  c_void_p, c_size_t, c_void_p]),
    "nms_cuda": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "roi_align_forward_cuda": (c_int, [c_int, c_int, c_float, c_void_p, c_int, c_int, c_int, c_int,
                                       c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "srcnn_pyramid_roi_align": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                        c_int, c_float, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p]),
    "srcnn_pool2x2_s1": (c_int, [c_void_p, ctypes.c_longlong, c_int, c_int, c_void_p, c_int, c_void_p]),
    "roi_align_backward_cuda": (c_int, [c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int,
                                        c_int, c_void_p]),
    "srcnn_pool2x2_s1_backward": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_int, c_int, c_void_p, c_int, c_void_p]),
    "srcnn_pyramid_roi_align_backward": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float,
                                                 ctypes.POINTER(c_void_p), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int,
                                                 c_int, c_void_p, c_void_p]),
    "srcnn_act_convert": (c_int, [c_void_p, c_int, c_void_p, c_int, ctypes.c_longlong, c_int, c_void_p]),
    "srcnn_gather_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "srcnn_decode_kept_kpts": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                       c_void_p]),
    "srcnn_conv2d_workspace_bytes": (c_size_t, [ctypes.POINTER(ConvDesc)]),
    "srcnn_conv2d": (c_int, [ctypes.POINTER(ConvDesc), c_void_p, c_size_t, c_void_p]),
    "srcnn_conv2d_chain_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "srcnn_conv2d_chain": (c_int, [ctypes.POINTER(ConvDesc), c_int, c_void_p]),
    "srcnn_conv2d_group": (c_int, [ctypes.POINTER(ConvDesc), c_int, c_void_p]),
    "srcnn_conv2d_backward_workspace_bytes": (c_size_t, [ctypes.POINTER(ConvBwdDesc)]),
    "srcnn_conv2d_backward": (c_int, [ctypes.POINTER(ConvBwdDesc), c_void_p, c_size_t, c_void_p]),
    "srcnn_conv2d_backward_f16x3_workspace_bytes": (c_size_t, [ctypes.POINTER(ConvBwdDesc)]),
    "srcnn_conv2d_backward_f16x3": (c_int, [ctypes.POINTER(ConvBwdDesc), c_void_p, c_size_t, c_void_p]),
    "srcnn_conv2d_forward_f16x3_workspace_bytes": (c_size_t, [ctypes.POINTER(ConvFwdF16x3Desc)]),
    "srcnn_conv2d_forward_f16x3": (c_int, [ctypes.POINTER(ConvFwdF16x3Desc), c_void_p, c_size_t, c_void_p]),
    "srcnn_conv2d_forward_f16x3_maxima": (c_int, [ctypes.POINTER(ConvFwdF16x3Desc), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "srcnn_conv2d_backward_f16x3_maxima": (c_int, [ctypes.POINTER(ConvBwdDesc), c_void_p, c_void_p, c_size_t, c_void_p]),
    "srcnn_absmax": (c_int, [c_void_p, ctypes.c_longlong, c_int, ctypes.c_longlong, c_void_p, c_void_p]),
    "srcnn_upsample_add_backward": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "srcnn_subsample2_backward": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "srcnn_pixel_shuffle2": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "srcnn_range_flag_read": (c_int, [c_int]),
    "srcnn_range_flag_device_word": (c_void_p, []),
    "srcnn_range_flag_bind": (c_int, [c_void_p]),
    "srcnn_preprocess": (c_int, [c_void_p, c_int, c_int, c_double, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]),
    "srcnn_stem_pack": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "srcnn_stem_pack_pair": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "srcnn_maxpool3x3s2_ceil": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "srcnn_upsample_add": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                   c_int, c_void_p]),
    "srcnn_subsample2": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "srcnn_nhwc_to_nchw": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "srcnn_nchw_to_nhwc": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "srcnn_rpn_score": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "srcnn_rpn_score_levels": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_int), c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "srcnn_rpn_score_parts": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(c_int),
                                      c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "srcnn_proposal_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "srcnn_proposal_workspace_layout": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_size_t), c_int]),
    "srcnn_proposal_layer": (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(c_int), c_int, c_void_p,
                                     c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                     c_void_p]),
    "srcnn_softmax_rows": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "srcnn_box_head_tail": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "srcnn_kpts_tail": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "srcnn_decode_detections": (c_int, [c_void_p] * 8 + [c_int, c_int, c_int] + [c_void_p] * 4 + [c_void_p]),
    "srcnn_class_nms_workspace_bytes": (c_size_t, [c_int]),
    "srcnn_class_nms": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_float, c_void_p, c_void_p,
                                c_void_p, c_size_t, c_void_p]),
    "srcnn_pack_detections": (c_int, [c_void_p] * 7 + [c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "srcnn_dense_align_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "srcnn_dense_align_workspace_layout": (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_size_t), c_int]),
    "srcnn_dense_align": (c_int, [c_void_p, c_void_p, c_int, c_int, c_double, c_double, c_double, c_double, c_double,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                  c_size_t, c_void_p]),
    "srcnn_box3d_workspace_bytes": (c_size_t, [c_int, c_int]),
    "srcnn_infer_boundary": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "srcnn_solve_4dof": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_double, c_double, c_double, c_double, c_float,
                                 c_void_p, c_void_p]),
    "srcnn_solve_4dof_scalar": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_double, c_double, c_double, c_double, c_float,
                                        c_void_p, c_void_p]),
    "srcnn_solve_3dof_scalar": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_double, c_double, c_double, c_double, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    "srcnn_align_inputs": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "srcnn_solve_3dof": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_double, c_double, c_double, c_double, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "srcnn_solve_4dof_records_host": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_double, c_double, c_double, c_double,
                                              c_float, c_void_p, c_int]),
    "srcnn_solve_3dof_records_host": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_double, c_double, c_double, c_double,
                                              c_void_p, c_void_p, c_void_p, c_int]),
    "srcnn_solve_4dof_host": (c_int, [c_int, c_int, c_double, c_double, c_double, c_double, c_double, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "srcnn_solve_3dof_host": (c_int, [c_int, c_int, c_double, c_double, c_double, c_double, c_double, c_void_p, c_void_p,
                                      c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "srcnn_solver_evaluate_host": (c_int, [c_int, c_int, c_double, c_double, c_double, c_double, c_double, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "srcnn_program_create": (c_void_p, []),
    "srcnn_program_destroy": (None, [c_void_p]),
    "srcnn_program_begin": (c_int, [c_void_p, c_void_p]),
    "srcnn_program_end": (c_int, [c_void_p]),
    "srcnn_program_recording": (c_int, []),
    "srcnn_program_record_event": (c_int, [c_void_p, c_void_p]),
    "srcnn_program_wait_event": (c_int, [c_void_p, c_void_p, c_int]),
    "srcnn_program_size": (c_int, [c_void_p]),
    "srcnn_program_run": (c_int, [c_void_p, c_void_p]),
    "srcnn_stream_create": (c_int, [c_int, ctypes.POINTER(c_void_p)]),
    "srcnn_stream_create_cu_mask": (c_int, [c_int, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(c_void_p)]),
    "srcnn_stream_destroy": (c_int, [c_void_p]),
    "srcnn_probe_placement": (c_int, [c_int, c_void_p, c_void_p, c_void_p]),
    "srcnn_prof_enable": (c_int, [c_int]),
    "srcnn_prof_read_launches": (c_int, [ctypes.POINTER(ctypes.c_float), c_int]),
    "srcnn_prof_read": (c_int, [ctypes.POINTER(c_double), ctypes.POINTER(c_double),
                                ctypes.POINTER(ctypes.c_longlong)]),
    "srcnn_kitti_overlaps": (c_int, [ctypes.POINTER(KittiSplit), c_void_p]),
    "srcnn_kitti_match": (c_int, [ctypes.POINTER(KittiSplit), ctypes.POINTER(KittiMatchDesc), c_void_p]),
    "srcnn_loss_workspace_bytes": (c_size_t, [ctypes.c_longlong]),
    "srcnn_cross_entropy": (c_int, [c_void_p, ctypes.c_longlong, c_int, ctypes.c_longlong, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    "srcnn_cross_entropy_backward": (c_int, [c_void_p, ctypes.c_longlong, c_int, ctypes.c_longlong, c_void_p, c_void_p, c_int, c_void_p,
                                             c_void_p, c_void_p, ctypes.c_longlong, c_void_p]),
    "srcnn_smooth_l1": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, ctypes.c_longlong, c_int, c_float,
                                c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "srcnn_smooth_l1_backward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, ctypes.c_longlong, c_int,
                                         c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "srcnn_anchor_targets_workspace_bytes": (c_size_t, [c_int, c_int]),
    "srcnn_anchor_targets": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     ctypes.POINTER(AnchorTargetParams)] + [c_void_p] * 6 + [c_void_p, c_size_t, c_void_p]),
    "srcnn_proposal_targets_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "srcnn_proposal_targets": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                       c_void_p, ctypes.POINTER(ProposalTargetParams)] + [c_void_p] * 12
                               + [c_void_p, c_size_t, c_void_p]),
    "srcnn_grad_norm_workspace_bytes": (c_size_t, [c_int, ctypes.POINTER(ctypes.c_longlong)]),
    "srcnn_grad_norm": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(ctypes.c_longlong), c_int, c_float, c_void_p, c_void_p, c_size_t,
                                c_void_p]),
    "srcnn_grad_scale": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(ctypes.c_longlong), c_int, c_void_p, c_void_p]),
    "srcnn_sgd_step": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(ctypes.c_longlong),
                               ctypes.POINTER(c_float), ctypes.POINTER(c_float), ctypes.POINTER(c_int), c_int, c_float, c_int, c_void_p,
                               c_void_p]),
    "srcnn_prep_weights_workspace_bytes": (c_size_t, [c_int]),
    "srcnn_prep_weights": (c_int, [ctypes.POINTER(PrepLayer), c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "srcnn_gt_batch": (c_int, [c_void_p, c_int, ctypes.POINTER(GtSlot), c_int, c_void_p, c_int, c_int] + [c_void_p] * 6 + [c_void_p]),
    "srcnn_preprocess_train": (c_int, [ctypes.POINTER(TrainImage), c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "srcnn_overlay_workspace_bytes": (c_size_t, [c_int]),
    "srcnn_render_overlay": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, ctypes.POINTER(c_double), c_float, c_void_p,
                                     c_double, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "srcnn_bev_lidar": (c_int, [c_void_p, c_int, ctypes.POINTER(c_double), c_double, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
}

_lib = None


def declared_symbols():
    return sorted(_SIGNATURES)


def lib():
    """Load the HIP library (once).  Raises if it is absent: no CPU/eager fallback exists."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libsrcnn_hip.so not found at %s - build it with `python -m stereo_rcnn_amd.csrc.build` "
                "(or __graft_entry__.build()). The product path has no fallback." % LIB_PATH)
        from . import streams
        streams.hip_may_start()            # the hardware-queue count HIP will start with is decided no later than here
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what="srcnn call"):
    if rc != 0:
        msg = lib().srcnn_last_error()
        raise RuntimeError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))


def ptr(t):
    """Device pointer of a contiguous CUDA(HIP) tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda, "libsrcnn_hip operates on device memory only"
    assert t.is_contiguous(), "tensor must be contiguous"
    return t.data_ptr()


def int_array(values, ctype=c_int):
    """C array of integers for a library call."""
    values = [int(v) for v in values]
    return (ctype * len(values))(*values)


def ptr_array(tensors_or_ints):
    """C array of device pointers for a library call: tensors (their data_ptr) or addresses."""
    ptrs = [t if isinstance(t, int) else t.data_ptr() for t in tensors_or_ints]
    return (c_void_p * len(ptrs))(*ptrs)


def stream():
    """Handle of torch's current HIP stream: every launch goes where torch's allocator expects it."""
    return torch.cuda.current_stream().cuda_stream


class Workspace(object):
    """Grow-only device scratch owned by the caller side (one per device)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        nbytes = max(int(nbytes), 256)
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self.buf


_workspaces = {}
_recording_refs = None      # while a launch program records: every workspace handed out (the program keeps them alive)


def workspace(nbytes, device, key="default"):
    # one scratch buffer per (device, purpose, stream): forwards in flight on different streams never share scratch
    k = (str(device), key, torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0)
    if k not in _workspaces:
        _workspaces[k] = Workspace()
    buf = _workspaces[k].get(nbytes, device)
    if _recording_refs is not None:
        _recording_refs.append(buf)
    return buf
