"""Inference configuration (`cfg`) with the reference's names (lib/model/utils/config.py).

Only the values the inference hot path reads are kept; line numbers refer to the
reference file.  `cfg` is attribute- and key-addressable like the reference's easydict
(`cfg.TEST.NMS`, `cfg['TEST'].RPN_NMS_THRESH`).
"""
import numpy as np


class _Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


cfg = _Cfg()
cfg.TRAIN = _Cfg()
cfg.TEST = _Cfg()
cfg.RESNET = _Cfg()

cfg.TRAIN.LEARNING_RATE = 0.001                   # :22
cfg.TRAIN.MOMENTUM = 0.9                          # :25
cfg.TRAIN.WEIGHT_DECAY = 0.0001                   # :28
cfg.TRAIN.DOUBLE_BIAS = False                     # :40
cfg.TRAIN.BIAS_DECAY = False                      # :46
cfg.TRAIN.TRUNCATED = False                       # :43
cfg.TRAIN.SCALES = (600,)                         # :49
cfg.TRAIN.MAX_SIZE = 2484                         # :52
cfg.TRAIN.BATCH_SIZE = 512                        # :55  rois per image of the proposal target layer
cfg.TRAIN.FG_FRACTION = 0.25                      # :58
cfg.TRAIN.FG_THRESH = 0.5                         # :61
cfg.TRAIN.BG_THRESH_HI = 0.5                      # :65
cfg.TRAIN.BG_THRESH_LO = 0.0                      # :66
cfg.TRAIN.BBOX_NORMALIZE_TARGETS = True           # :69
cfg.TRAIN.BBOX_INSIDE_WEIGHTS = (1.0, 1.0, 1.0, 1.0)       # :72
cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED = True        # :76
cfg.TRAIN.DIM_NORMALIZE_TARGETS_PRECOMPUTED = True         # :80
cfg.TRAIN.RPN_POSITIVE_OVERLAP = 0.7              # :86
cfg.TRAIN.RPN_NEGATIVE_OVERLAP = 0.3              # :88
cfg.TRAIN.RPN_CLOBBER_POSITIVES = False           # :90
cfg.TRAIN.RPN_FG_FRACTION = 0.5                   # :92
cfg.TRAIN.RPN_BATCHSIZE = 512                     # :94
cfg.TRAIN.RPN_NMS_THRESH = 0.7                    # :96
cfg.TRAIN.RPN_PRE_NMS_TOP_N = 12000               # :98
cfg.TRAIN.RPN_POST_NMS_TOP_N = 2000               # :100
cfg.TRAIN.RPN_MIN_SIZE = 8                        # :102
cfg.TRAIN.RPN_BBOX_INSIDE_WEIGHTS = (1.0, 1.0, 1.0, 1.0)   # :104
cfg.TRAIN.RPN_POSITIVE_WEIGHT = -1.0              # :108
cfg.MAX_NUM_GT_BOXES = 30                         # :207
cfg.TRAIN.BBOX_NORMALIZE_MEANS = (0.0, 0.0, 0.0, 0.0)      # :77
cfg.TRAIN.BBOX_NORMALIZE_STDS = (0.1, 0.1, 0.2, 0.2)       # :78
cfg.TRAIN.DIM_NORMALIZE_MEANS = (1.6, 1.5, 4.0, 0.0, 0.0)  # :81
cfg.TRAIN.DIM_NORMALIZE_STDS = (0.5, 0.5, 0.5, 0.5, 0.5)   # :82
cfg.TEST.SCALES = (600,)                          # :117
cfg.TEST.MAX_SIZE = 2484                          # :120
cfg.TEST.NMS = 0.3                                # :124
cfg.TEST.RPN_NMS_THRESH = 0.7                     # :127
cfg.TEST.RPN_PRE_NMS_TOP_N = 6000                 # :129
cfg.TEST.RPN_POST_NMS_TOP_N = 300                 # :132
cfg.TEST.RPN_MIN_SIZE = 16                        # :135 (filter is commented out, proposal_layer.py:90)
cfg.PIXEL_MEANS = np.array([[[102.9801, 115.9465, 122.7717]]])   # :170
cfg.KPTS_GRID = 28                                # :173
cfg.RNG_SEED = 3                                  # :178
cfg.USE_GPU_NMS = True                            # :196
cfg.POOLING_SIZE = 7                              # :204
cfg.ANCHOR_RATIOS = [0.5, 1, 2]                   # :210
cfg.FEAT_STRIDE = [16, ]                          # :213
cfg.FPN_ANCHOR_SCALES = [32, 64, 128, 256, 512]   # :216
cfg.FPN_FEAT_STRIDES = [4, 8, 16, 32, 64]         # :219
cfg.FPN_ANCHOR_STRIDE = 1                         # :222
cfg.RESNET.FIXED_BLOCKS = 1
