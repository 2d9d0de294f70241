"""Host-side driver of the HIP convolution engine and NHWC helpers.

Thin Python over the C ABI (include/srcnn_hip.h): weight re-layout / frozen-BN folding
at load time, and one function per native op that fills the C descriptor and launches on
torch's current stream.  No arithmetic happens here.
"""
import ctypes
import os as _os

import torch

from . import _lib


class ConvW(object):
    """A convolution prepared for the engine: weight (Cout, KH, KW, Cin) K-contiguous, bias."""

    def __init__(self, weight, bias, kh, kw, stride, pad, relu, mode=0, cin2=0, stride2=1):
        self.weight = weight.contiguous()
        self.bias = None if bias is None else bias.contiguous()
        self.cout = int(weight.shape[0])
        # cin2 > 0 (1x1 only): the last cin2 columns of K belong to a SECOND input sampled with stride2 (prep_conv_shortcut)
        self.cin2, self.stride2 = int(cin2), int(stride2)
        self.cin = int(weight.numel() // (weight.shape[0] * kh * kw)) - self.cin2
        self.kh, self.kw, self.stride, self.pad, self.relu, self.mode = kh, kw, stride, pad, int(relu), mode
        self.alg_k = self.cin * kh * kw + self.cin2      # algorithmic K (the stem pads 147 -> 224; see prep_stem)
        self.w_hi = self.w_lo = None         # f16x3 engine operands (see split_f16x3)
        self.inv_scale = 1.0

    def split_f16x3(self):
        """Error-compensated split for the f16 MFMA engine (csrc/conv_f16x3.hip):
        w * 2^k = hi + lo with hi = f16(w 2^k), lo = f16(w 2^k - hi); k puts max|w| near 2^14 so
        that lo stays out of the f16 subnormal range.  Exact power-of-two scaling, undone in the epilogue."""
        if self.w_hi is None:
            import math
            m = float(self.weight.abs().max())
            k = math.floor(math.log2(16384.0 / m)) if m > 0 else 0
            ws = self.weight * (2.0 ** k)
            self.w_hi = ws.half()
            self.w_lo = (ws - self.w_hi.float()).half().contiguous()
            self.w_hi = self.w_hi.contiguous()
            self.inv_scale = 2.0 ** (-k)
        return self


def fold_bn(w, bn, eps=1e-5):
    """Frozen BN (resnet.py:300-309: always eval) folded into the preceding bias-free conv.
    Done in float64, stored float32:  w' = w * g/sqrt(v+eps),  b' = beta - mean * g/sqrt(v+eps)."""
    s = bn['weight'].double() / torch.sqrt(bn['running_var'].double() + eps)
    wf = (w.double() * s.view(-1, 1, 1, 1)).float()
    bf = (bn['bias'].double() - bn['running_mean'].double() * s).float()
    return wf, bf


def prep_conv(w, b, stride=1, pad=0, relu=False, bn=None, device='cuda'):
    """nn.Conv2d weight (Cout, Cin, KH, KW) -> engine layout (Cout, KH, KW, Cin)."""
    if bn is not None:
        w, b = fold_bn(w, bn)
    kh, kw = int(w.shape[2]), int(w.shape[3])
    wt = w.permute(0, 2, 3, 1).contiguous().to(device)
    return ConvW(wt, None if b is None else b.to(device), kh, kw, stride, pad, relu)


def prep_conv_shortcut(w3, bn3, wd, bnd, stride2, device='cuda'):
    """The last 1x1 conv of a bottleneck block and the block's projection shortcut (resnet.py:86-100:
    out = relu(bn3(conv3(t)) + bn_d(downsample(x)))) as ONE GEMM over K = [channels of t | channels of x]: both frozen BNs
    folded, weights concatenated along K, biases added.  The shortcut's result is then never written nor read back as a
    residual, and its launch is gone (srcnn_conv_desc.x2)."""
    w3f, b3 = fold_bn(w3, bn3)
    wdf, bd = fold_bn(wd, bnd)
    assert w3f.shape[2:] == (1, 1) and wdf.shape[2:] == (1, 1) and w3f.shape[0] == wdf.shape[0]
    wt = torch.cat((w3f[:, :, 0, 0], wdf[:, :, 0, 0]), 1).contiguous().view(w3f.shape[0], 1, 1, -1).to(device)
    return ConvW(wt, (b3.double() + bd.double()).float().to(device), 1, 1, 1, 0, True, cin2=int(wdf.shape[1]), stride2=stride2)


def prep_stem(w, bn, device='cuda'):
    """7x7/2 stem (resnet.py:109) as 7 row-taps of 32 floats = 8 pixels x NHWC4 (see srcnn_stem_pack)."""
    wf, bf = fold_bn(w, bn)
    cout = wf.shape[0]
    wt = torch.zeros(cout, 7, 8, 4, device=wf.device)
    wt[:, :, :7, :3] = wf.permute(0, 2, 3, 1)          # (co, kh, kw, c)
    cw = ConvW(wt.view(cout, 7, 1, 32).to(device), bf.to(device), 7, 1, 2, 0, True)
    cw.alg_k = 3 * 7 * 7
    return cw


def prep_deconv2x2(w, b, relu=True, device='cuda'):
    """nn.ConvTranspose2d(k=2, s=2) weight (Cin, Cout, 2, 2) -> GEMM rows ordered (i, j, co)."""
    cin, cout = int(w.shape[0]), int(w.shape[1])
    wt = w.permute(2, 3, 1, 0).contiguous().view(4 * cout, 1, 1, cin)
    return ConvW(wt.to(device), b.to(device), 1, 1, 1, 0, relu, mode=1)


def prep_linear_stack(ws, bs, device='cuda'):
    """Several nn.Linear(in, out_i) sharing the input -> one (sum out_i, 1, 1, in) conv."""
    w = torch.cat([x for x in ws], 0)
    b = torch.cat([x for x in bs], 0)
    return ConvW(w.view(w.shape[0], 1, 1, w.shape[1]).to(device), b.to(device), 1, 1, 1, 0, False)


def head_fragments(hcw):
    """The weights of a narrow 1x1 head (ConvW (N2, 1, 1, C)) for the MFMA-form fused head (srcnn_conv_desc.head_wf): split into
    hi / lo f16 like any weight of the f16x3 engine, rows zero-padded to a multiple of 8, and laid out in the order the kernel's
    lanes read them: [C / 16 steps][hi, lo][k group 0, 1][rows][8 halves], element (s, g, n, i) = W[n][16 s + 8 g + i].
    Returns (tensor, rows); cached on the ConvW."""
    if getattr(hcw, '_frag', None) is None:
        assert hcw.kh == 1 and hcw.kw == 1 and hcw.cin % 16 == 0 and hcw.cout <= 24
        hcw.split_f16x3()
        n2, C = hcw.cout, hcw.cin
        rows = -(-n2 // 8) * 8
        f = torch.zeros((2, rows, C), dtype=torch.float16, device=hcw.w_hi.device)
        f[0, :n2] = hcw.w_hi.view(n2, C)
        f[1, :n2] = hcw.w_lo.view(n2, C)
        f = f.view(2, rows, C // 16, 2, 8).permute(2, 0, 3, 1, 4).contiguous()        # (step, hi/lo, k group, row, 8)
        hcw._frag = (f, rows)
    return hcw._frag


class PrepSpec(object):
    """One layer of srcnn_prep_weights (include/srcnn_hip.h, "weight preparation"): the sources in nn.Module layout (float32
    contiguous device tensors) and the destination tensors, which the call overwrites where they are.
    form: _lib.PREP_*; ws / bs: the source weights and biases (bs None or a list with None entries); bns: one frozen-BN dict
    (weight, bias, running_mean, running_var) per folded source.  alias_of: index of an earlier spec of the same call whose
    dst_w / dst_b this layer shares (it then writes only its own hi / lo / fragments)."""

    def __init__(self, form, ws, bs=None, bns=(), dst_w=None, dst_b=None, dst_hi=None, dst_lo=None, dst_frag=None, frag_rows=0,
                 alias_of=-1):
        self.form, self.ws, self.bs, self.bns = form, list(ws), list(bs) if bs is not None else [None] * len(ws), list(bns)
        self.dst_w, self.dst_b, self.dst_hi, self.dst_lo, self.dst_frag, self.frag_rows = dst_w, dst_b, dst_hi, dst_lo, dst_frag, frag_rows
        self.alias_of = alias_of

    @classmethod
    def for_convw(cls, form, cw, ws, bs=None, bns=(), alias_of=-1):
        """Into the tensors a ConvW already holds: weight, bias, and -- where they exist -- w_hi / w_lo and the fused head's fragments."""
        frag, rows = getattr(cw, '_frag', None) or (None, 0)
        return cls(form, ws, bs, bns, cw.weight, cw.bias, cw.w_hi, cw.w_lo, frag, rows, alias_of)

    def fill(self, d):
        w0 = self.ws[0]
        d.form, d.n_src, d.alias_of, d.frag_rows = self.form, len(self.ws), self.alias_of, self.frag_rows
        if self.form == _lib.PREP_DECONV2X2:
            d.cin, d.cout[0], d.kh, d.kw = int(w0.shape[0]), int(w0.shape[1]), int(w0.shape[2]), int(w0.shape[3])
        else:
            d.cin = int(w0.shape[1])
            d.kh, d.kw = (int(w0.shape[2]), int(w0.shape[3])) if w0.dim() == 4 else (1, 1)
            if self.form == _lib.PREP_SHORTCUT:
                d.cin2 = int(self.ws[1].shape[1])
            for i, w in enumerate(self.ws):
                d.cout[i] = int(w.shape[0])
                assert self.form == _lib.PREP_SHORTCUT or tuple(w.shape[1:]) == tuple(w0.shape[1:]), "sources of one layer share Cin and the kernel size"
        for i, (w, b) in enumerate(zip(self.ws, self.bs)):
            d.w[i], d.b[i] = _prep_src(w, int(w.numel())), _prep_src(b, d.cout[i])
        for i, bn in enumerate(self.bns):
            if bn is not None:
                d.bn_g[i], d.bn_b[i], d.bn_m[i], d.bn_v[i] = (_prep_src(bn[k], d.cout[i]) for k in ('weight', 'bias', 'running_mean', 'running_var'))
        rows = 4 * d.cout[0] if self.form == _lib.PREP_DECONV2X2 else (sum(d.cout[:len(self.ws)]) if self.form == _lib.PREP_CONV else d.cout[0])
        row_len = 224 if self.form == _lib.PREP_STEM else (d.cin + d.cin2) * (d.kh * d.kw if self.form == _lib.PREP_CONV else 1)
        n_bias = d.cout[0] if self.form == _lib.PREP_DECONV2X2 else rows
        for name, t, dt, n in (('dst_w', self.dst_w, torch.float32, rows * row_len), ('dst_b', self.dst_b, torch.float32, n_bias),
                               ('dst_hi', self.dst_hi, torch.float16, rows * row_len), ('dst_lo', self.dst_lo, torch.float16, rows * row_len),
                               ('dst_frag', self.dst_frag, torch.float16, 2 * self.frag_rows * row_len)):
            if t is not None:
                assert t.is_cuda and t.is_contiguous() and t.dtype == dt and t.numel() == n, \
                    "prep_weights_into: %s must be a contiguous %s device tensor of %d elements" % (name, dt, n)
                setattr(d, name, t.data_ptr())


def _prep_src(t, numel):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == numel, \
        "prep_weights_into: sources are contiguous float32 device tensors of the layer's sizes"
    return t.data_ptr()


def prep_weights_into(specs, k_out=None):
    """srcnn_prep_weights over a list of PrepSpec on torch's current stream: BN fold, re-layout, max |w|, hi / lo split and head
    fragments of every layer, written into the specs' destination tensors.  No host read.  Returns k_out, the device int32 vector of
    the layers' power-of-two exponents k (inv_scale = 2^-k)."""
    L = _lib.lib()
    n = len(specs)
    dev = specs[0].dst_w.device
    if k_out is None:
        k_out = torch.empty((n,), dtype=torch.int32, device=dev)
    assert k_out.is_cuda and k_out.dtype == torch.int32 and k_out.numel() == n and k_out.is_contiguous()
    descs = (_lib.PrepLayer * n)()
    for d, s in zip(descs, specs):
        s.fill(d)
    with torch.cuda.device(dev):
        ws = _lib.workspace(L.srcnn_prep_weights_workspace_bytes(n), dev, "prep_weights")
        _lib.check(L.srcnn_prep_weights(descs, n, k_out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()), "srcnn_prep_weights")
    return k_out


def conv_out_hw(h, w, k_h, k_w, stride, pad):
    return (h + 2 * pad - k_h) // stride + 1, (w + 2 * pad - k_w) // stride + 1


class FlopCounter(object):
    """Algorithmic conv FLOPs (2*M*N*K with the true K) of the launches issued while enabled, and their COMPULSORY bytes:
    every operand element the launch needs read once and every result written once, at the 4 bytes per element both activation
    formats and both weight forms (fp32, or hi + lo f16) occupy -- input pixels x Cin (only the sampled pixels of a strided
    1x1), weights Cout x K, residual and output M x Cout."""
    enabled = False
    flops = 0.0
    launches = 0
    bytes = 0.0
    rows = None          # list: one dict per launch (name, M, N, K, flops, bytes, plan) while enabled; see layer_table.py


# ---- SPLIT16 range guard (include/srcnn_hip.h: srcnn_range_flag_read): layers are tagged by name so that a tripped flag
# can be reported as the layer that produced the out-of-range activation
TAG_NAMES = {9001: 'upsample_add', 9002: 'input conversion to SPLIT16 (stem_pack / act_convert)',
             9003: 'maxpool3x3s2_ceil (an F32 input beyond the SPLIT16 range)'}
_TAG_IDS = {}


def layer_tag(name):
    if name is None:
        return 0
    t = _TAG_IDS.get(name)
    if t is None:
        t = _TAG_IDS[name] = len(_TAG_IDS) + 1
        TAG_NAMES[t + 1] = name                 # the flag holds tag + 1
    return t


class Split16RangeError(RuntimeError):
    """An activation left the range the SPLIT16 format can hold (|v| > 65504 or NaN): the f16x3 results of that forward are
    not valid; re-run it with precision 'f32'."""


def range_flag(reset=True):
    """(flag, layer name): flag 0 = every SPLIT16 tensor written since the last reset was in range.  Synchronises the device."""
    v = _lib.lib().srcnn_range_flag_read(1 if reset else 0)
    if v < 0:
        _lib.check(v, "srcnn_range_flag_read")
    return v, (TAG_NAMES.get(v, 'layer tag %d' % (v - 1)) if v else None)


PRECISION = 'f32'     # default engine: 'f32' (exact fp32 MFMA) or 'f16x3' (3-term split on the f16 MFMA)

# ---- per-shape launch-plan autotuning ("measure, don't guess"): every distinct conv shape is timed
# once on the device it runs on over the legal (tile, split-K) plans; the winner is cached.
AUTOTUNE = True
_TUNED = {}
_TUNE_LOG = {}       # key -> [(plan, ms)] of the last tuning run (dev tools print it)
# (tile_mr, tile_nr, waves, stages): workgroup tile (64*mr) x (64*nr), wavefronts, LDS ring depth
_CANDIDATES = [(2, 2, 4, 2), (2, 1, 4, 2), (1, 2, 4, 2), (1, 1, 4, 2)]
# extra variants of the SPLIT16 engine (csrc/conv_f16s.hip): 8-wave tiles and deeper DMA rings
# ((4, 4, 8, 2) = 256x256 on 8 waves of 64x128: 25 % fewer LDS fragment bytes per MFMA than the 64x64 per-wave tiles)
_CANDIDATES_F16S = [(4, 4, 8, 2), (4, 2, 8, 3), (2, 2, 8, 4), (2, 2, 8, 2), (2, 1, 4, 3), (1, 2, 4, 3), (1, 1, 4, 4)]


# Largest LDS footprint (KB per workgroup) a tuned plan may have.  Isolated-launch timing always favours the deepest ring /
# biggest tile (up to 144 KB: one workgroup per CU, nothing else fits beside it); with several pairs in flight a smaller
# footprint lets workgroups of OTHER launches share the CU and fill the matrix pipe's idle slots (profiles/lds_cap_r03.txt).
MAX_LDS_KB = int(_os.environ.get('SRCNN_MAX_LDS_KB', '160'))


ACT_SCALES = _os.environ.get('SRCNN_ACT_SCALES', '1') != '0'    # per-tensor power-of-two SPLIT16 activation scales (plan.calibrate)
LIMIT_TUNE_ROIS = 64          # row-limited launches (the lazy keypoint head) are tuned for this many units below the limit
RPN_PAIR_LAUNCH = _os.environ.get('SRCNN_RPN_PAIR', '1') != '0'     # A/B switch of the one-launch stereo RPN conv (conv mode 2)
# A/B switch: the projection shortcut of a layer's first block computed inside that block's conv3 (prep_conv_shortcut)
SHORTCUT_FUSION = _os.environ.get('SRCNN_SHORTCUT_FUSION', '1') != '0'
# A/B switches: the keypoint branch's 6-channel classifier computed inside the epilogue of the deconvolution -- '1' / 'valu' = round
# 4's fp32-FMA + DPP form (conv2d(head=...), srcnn_conv_desc.head_w), 'mfma' = as a second GEMM on the matrix pipe (conv2d(head2=...),
# srcnn_conv_desc.head_wf: the form the RPN head needs; for this 6-channel head on a K = 256 launch it is 10 % slower alone --
# 183 vs 166 us: the weight slice's load and four of eight waves computing -- and equal in the mix, profiles/kpts_head_form_r05.txt),
# '0' = two launches; and the stereo RPN's 24-channel head computed inside the RPN conv's epilogue as per-(eye, N tile) partial sums
KPTS_HEAD_FUSION = _os.environ.get('SRCNN_KPTS_HEAD_FUSION', '1')
KPTS_HEAD_FUSION = {'0': False, '1': 'valu'}.get(KPTS_HEAD_FUSION, KPTS_HEAD_FUSION)
RPN_HEAD_FUSION = _os.environ.get('SRCNN_RPN_HEAD_FUSION', '1') != '0'
# the five pyramid levels of the stereo RPN (shared RPN_Conv + head weights, stereo_rpn.py:73-95) in grouped launches
# (srcnn_conv2d_group): 'all' = one launch for P2..P6 behind the last smoothing conv, 'small' = P3..P6 in one launch (76 + 20 + 6 + 292
# tiles of 256x256: launches that cannot fill 256 CUs on their own) and P2 by itself, '0' = one launch per level.  Bit-identical.
RPN_GROUP = _os.environ.get('SRCNN_RPN_GROUP', 'small')
RPN_GROUP_TILE = tuple(int(c) for c in _os.environ.get('SRCNN_RPN_GROUP_TILE', '4482'))       # (tile_mr, tile_nr, waves, stages): 4482 or 2282
# A/B switch: the FPN top-down addition (_upsample_add) computed inside the lateral 1x1 conv's epilogue (conv2d(up=...),
# srcnn_conv_desc.up_top) whenever the lateral is launched inline behind its top map -- i.e. with several forwards in flight; a
# lone forward keeps the laterals on a side stream, early, and the separate srcnn_upsample_add.  Bit-identical either way.
# Built, tested, and NOT the default: three launches and 0.4 GB of traffic per pair fewer, and 0.2-0.4 % SLOWER four in flight
# (155.5 / 155.2 against 155.8 / 155.8 pairs/s, same box, profiles/upsample_fusion_ab_r05.txt) -- the mix is not short of HBM
# bandwidth, and the four bilinear taps lengthen the epilogue of a launch whose workgroups hold the matrix pipe's LDS.
UPSAMPLE_FUSION = _os.environ.get('SRCNN_UPSAMPLE_FUSION', '0') != '0'

# ---- chained bottleneck launches (csrc/conv_chain.hip: srcnn_conv2d_chain): [conv2 -> conv3 -> conv1 of the next block] as ONE launch
# whose workgroups keep their rows through the three convolutions.  BOTTLENECK_CHAIN: '0' (default) = off, '1' = on, 'auto' = on while
# several forwards are in flight.  Built, bit-identical (tests/test_conv_chain_gpu.py), measured, and NOT the default: the headline
# step is the same with and without it (profiles/chain_ab_r06.txt: 6.35-6.39 ms off, 6.35-6.41 ms with layer1 / layer2 / layer3
# chained on their best tiles, at 3, 4, 6 and 8 forwards in flight) -- the intermediates come back through the fabric all the
# same (a layer3 block's weights alone are 4.4 MB, the XCD's whole L2), and the package power limit prices the step by its
# MFMA work, which a chain does not change.  It removes 46 launches per forward.
BOTTLENECK_CHAIN = _os.environ.get('SRCNN_BOTTLENECK_CHAIN', '0')
# planes of the bottleneck (64, 128, 256, 512) -> (tile_mr, waves, stages, narrow nr, wide nr) or None = that layer keeps its
# separate launches.  layer4 (M = 2394: 10 workgroups of 256 rows) stays unchained.
CHAIN_TILES = {64: (2, 4, 2, 1, 1), 128: (4, 8, 3, 2, 2), 256: (4, 8, 3, 2, 2), 512: None}
CHAIN_MIN_WGS = 32        # a chain launch with fewer workgroups than this is not worth its latency


# ---- what the tuner minimises.  'isolated': the latency of the launch alone on the chip (the right objective for one pair at a
# time).  'concurrent': the time per launch while TUNE_STREAMS copies of the launch run on as many HIP streams -- the regime of
# the headline benchmark and of pipeline.detect_3d_stream, where several batch-1 forwards are in flight and a plan is worth
# what it costs in CU-time, not in latency: a 150-workgroup plan that leaves 106 CUs to the neighbours beats a split-K plan
# that is 10 % faster alone but occupies the whole chip and needs a reduction launch (profiles/tune_objective_r04.txt).
# The two plan sets live side by side in _TUNED (the mode is part of the key).
TUNE_MODE = _os.environ.get('SRCNN_TUNE_MODE', 'isolated')
TUNE_STREAMS = int(_os.environ.get('SRCNN_TUNE_STREAMS', '3'))
_tune_side_streams = {}
_tune_flag = None          # scratch word that takes the range-guard reports of the tuner's trial launches (_tune)

# Measurement hook (mix_table.py): [(compiled regex, n)] -- a conv launch whose layer name matches is issued n MORE times right
# behind itself (same arguments: the output is simply rewritten).  The step-time increase per extra launch is that layer's
# marginal cost INSIDE the several-forwards-in-flight mix, which no per-launch timing can give.  Empty in production.
REPEAT = []

# Measurement hook (tools/skip_probe.py): names of NON-conv stages of the forward that Plan leaves out while it records / runs
# ('maxpool', 'upsample_add', 'subsample', 'rpn_scores', 'proposals', 'roi_align', 'box_tail', 'kpts_tail') -- the buffers they would
# have written keep the previous frame's contents, so the step still runs on valid data; the step-time difference is what the
# stage costs INSIDE the several-forwards-in-flight mix.  Empty in production.
DEBUG_SKIP = frozenset()

# Bumped by whoever rewrites _TUNED under a model that already recorded launch programs (tune.tune_throughput, load_plans):
# every Plan compares it in run() and re-records.  KEY_HITS: while a dict, conv2d counts the launches per plan key.
PLAN_EPOCH = 0
KEY_HITS = None


def set_tune_mode(mode, streams=None):
    """'isolated' or 'concurrent' (see above).  Plans recorded into launch programs under the other mode are dropped by
    Plan.run (the mode is part of its epoch)."""
    global TUNE_MODE, TUNE_STREAMS
    assert mode in ('isolated', 'concurrent')
    TUNE_MODE = mode
    if streams is not None:
        TUNE_STREAMS = int(streams)


def tune_mode_key():
    return ('conc', TUNE_STREAMS) if TUNE_MODE == 'concurrent' and TUNE_STREAMS > 1 else ()


def set_plan(key, plan):
    """Overwrite the tuned plan of one shape key; recorded launch programs are re-recorded on their next run."""
    global PLAN_EPOCH
    _TUNED[tuple(key)] = tuple(plan)
    PLAN_EPOCH += 1


def plan_lds_kb(mr, nr, waves, stages):
    return stages * 128 * 64 * (mr + nr) // 1024


def save_plans(path):
    """Write the tuned plans (shape key -> plan) as JSON: a later process on the same GPU model can skip the tuning launches."""
    import json
    with open(path, 'w') as f:
        json.dump([[list(k), list(v)] for k, v in _TUNED.items()], f)


def load_plans(path):
    """Adopt plans written by save_plans(); shapes not in the file are still tuned on first use.  Returns the count."""
    import json
    with open(path) as f:
        rows = json.load(f)
    global PLAN_EPOCH
    for k, v in rows:
        _TUNED[tuple(k)] = tuple(v)
    PLAN_EPOCH += 1
    return len(rows)


def _shape_key(cw, B, H, W, OH, OW, x_cstride, precision, fmts=(0, 0, 0)):
    return (precision, B, H, W, OH, OW, cw.cin, cw.cout, cw.kh, cw.kw, cw.stride, cw.pad, cw.mode, x_cstride) + tuple(fmts)


def _set_plan(d, plan):
    d.tile_mr, d.tile_nr, d.tile_waves, d.tile_stages, d.splits = plan


def _candidate_plans(d, only=None):
    """The plans (mr, nr, waves, stages, splits) _tune times for the launch d describes, in trial order.
    only: the (mr, nr, waves, stages) tiles to choose from, unsplit (launches with an MFMA-form fused head).  Of the shape rules
    below they obey their own alone -- no 256-row tile for fewer than four of them, but never an empty choice -- and the LDS cap."""
    M = d.B * d.OH * d.OW
    if only is not None:
        tiles = [t for t in only if not (t[0] >= 4 and M < 256 * 4)] or list(only)[-1:]
        return [tuple(t) + (1,) for t in tiles if plan_lds_kb(*t) <= MAX_LDS_KB]
    nkt = (d.KH * d.KW * d.Cin + d.Cin2) // 32
    fused_in = d.x2 or d.up_top            # a second input / the top-down addition: never split-K, never the 256x256 tile
    tiles = list(_CANDIDATES)
    if d.precision == 1 and d.x_format == 1:
        tiles = _CANDIDATES_F16S + tiles
    cands = []
    for mr, nr, waves, stages in tiles:
        if plan_lds_kb(mr, nr, waves, stages) > MAX_LDS_KB:
            continue
        if nr == 2 and d.Cout <= 64:
            continue
        # the 256x256 tile: not with a second input (register budget); few fat workgroups lose the latency contest of this tuner on the
        # small-M layers but can win the several-in-flight step (tune.tune_throughput takes its candidates from this log)
        if nr == 4 and (d.Cout <= 128 or M < 256 * 8 or fused_in):
            continue
        if mr >= 2 and M <= 64 * (mr // 2):
            continue
        blocks = -(-M // (64 * mr)) * -(-d.Cout // (64 * nr))
        cands.append((mr, nr, waves, stages, 1))
        if d.mode != 1 and not fused_in:
            cands += [(mr, nr, waves, stages, s) for s in (2, 3, 4, 6, 8, 12, 16)
                      if blocks * s <= 4096 and nkt // s >= 4 and blocks < 1024]
    return cands


def _tune(d, key, device, only=None):
    """Times each candidate plan with HIP events on the current stream: three interleaved passes, then a play-off.
    only: see _candidate_plans."""
    L = _lib.lib()
    cands = _candidate_plans(d, only)
    log = _TUNE_LOG.setdefault(key, [])
    del log[:]
    st = _lib.stream()
    # the trial launches may run on whatever the buffers hold (a tensor last written in the other activation format reads as
    # NaNs): their range-guard reports go to a scratch word, not to the forward's
    global _tune_flag
    if _tune_flag is None or _tune_flag.device != device:
        _tune_flag = torch.zeros(1, dtype=torch.int32, device=device)
    bound = L.srcnn_range_flag_device_word()
    L.srcnn_range_flag_bind(_tune_flag.data_ptr())
    try:
        return _tune_candidates(d, key, device, cands, log, L, st)
    finally:
        L.srcnn_range_flag_bind(bound)


def _tune_candidates(d, key, device, cands, log, L, st):
    conc = tune_mode_key()
    if conc:
        pool = _tune_side_streams.setdefault(str(device), [])
        while len(pool) < TUNE_STREAMS:
            pool.append(torch.cuda.Stream(device=device))
        side = pool[:TUNE_STREAMS]

    def timed_isolated(plan, launches):
        _set_plan(d, plan)
        ws = _lib.workspace(L.srcnn_conv2d_workspace_bytes(ctypes.byref(d)), device, "conv")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            _lib.check(L.srcnn_conv2d(ctypes.byref(d), ws.data_ptr(), ws.numel(), st), "srcnn_conv2d(tune)")
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / launches

    def timed_concurrent(plan, launches):
        """time per launch with the same launch running on TUNE_STREAMS streams at once (every stream its own split-K scratch;
        the copies read the same operands and write the same values to the same output)"""
        _set_plan(d, plan)
        need = L.srcnn_conv2d_workspace_bytes(ctypes.byref(d))
        wss = []
        for s in side:
            with torch.cuda.stream(s):
                wss.append(_lib.workspace(need, device, "conv"))
        cur = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        for s in side:
            s.wait_event(e0)
        for _ in range(launches):
            for s, ws in zip(side, wss):
                _lib.check(L.srcnn_conv2d(ctypes.byref(d), ws.data_ptr(), ws.numel(), s.cuda_stream), "srcnn_conv2d(tune)")
        for s in side:
            cur.wait_stream(s)
        e1.record(cur)
        e1.synchronize()
        return e0.elapsed_time(e1) / (launches * len(side))

    timed = timed_concurrent if conc else timed_isolated

    # three passes over all candidates (a transient -- clock ramp, a neighbour's kernel -- then hits every plan once, not
    # one plan always), minimum per plan; the first launch of a plan is a warm-up
    best_of = {}
    for rnd in range(3):
        for plan in cands:
            if rnd == 0:
                timed(plan, 1)
            t = timed(plan, 2)
            if plan not in best_of or t < best_of[plan]:
                best_of[plan] = t
    # play-off between the three fastest
    finalists = sorted(best_of, key=best_of.get)[:3]
    for plan in finalists * 3:
        best_of[plan] = min(best_of[plan], timed(plan, 3))
    for plan in cands:
        log.append((plan, best_of[plan]))
    best = min(finalists, key=best_of.get)
    _TUNED[key] = best
    return best


def conv_cost(cw, B, H, W, OH, OW, residual=False, up=None, head=False, head2=None, first_in_chain=True, grouped=False):
    """What FlopCounter books for one convolution: (flops, bytes, M, N, K).  A pure function of the shape and the options conv2d
    takes (residual / head: whether there is one; up, head2: conv2d's tuples).  Algorithmic flops 2 M N K with the true K, and
    compulsory bytes at 4 per element (see FlopCounter), by these rules:
    - a 1x1 convolution reads only the pixels it samples (M of them, whatever its stride); any other kernel reads the whole input;
    - a later phase of a chain (first_in_chain=False) reads what its workgroup has just written: its input is not counted.  Its
      weights, second input, residual and output are;
    - a fused head adds its own flops, and its output replaces y (not written): 6 channels per tap for the fp32-FMA head; for the
      MFMA head its channels per tap, once (final) or once per 256 conv channels (partial sums);
    - a deconvolution (mode 1) is 4 taps of Cout / 4 channels each;
    - a problem of a grouped launch is counted as the plain convolution the RPN levels are: one input, one tap per pixel, no
      top-down addition."""
    M = B * OH * OW
    taps = 4 if cw.mode == 1 and not grouped else 1
    px_in = M if (cw.kh == 1 and cw.kw == 1) else B * H * W
    flops = 2.0 * M * cw.cout * cw.alg_k
    nbytes = 4.0 * ((px_in * cw.cin if first_in_chain else 0) + (0 if grouped else M * cw.cin2) + cw.cout * cw.alg_k
                    + M * cw.cout * (2 if residual else 1) + (B * up[1] * up[2] * cw.cout if up is not None and not grouped else 0))
    if head2 is not None:
        hn = head2[0].cout
        flops += 2.0 * M * hn * cw.cout
        nbytes += 4.0 * M * (taps * hn * (max(1, cw.cout // 256) if head2[2] else 1) - cw.cout)
    if head:
        flops += 2.0 * M * taps * 6 * (cw.cout // taps)
        nbytes += 4.0 * M * (taps * 6 - cw.cout)
    return flops, nbytes, M, cw.cout, cw.alg_k


def _book(name, flops, nbytes, M, N, K, plan, **extra):
    """Books one launch into FlopCounter: the totals, and its row (extra: the 'chain' / 'group' key of a fused launch)."""
    if FlopCounter.enabled:
        FlopCounter.flops += flops
        FlopCounter.bytes += nbytes
        FlopCounter.launches += 1
        if FlopCounter.rows is not None:
            FlopCounter.rows.append(dict({'name': name, 'M': M, 'N': N, 'K': K, 'flops': flops, 'bytes': nbytes, 'plan': plan}, **extra))


def _plan_key(cw, d, precision, lim):
    """The _TUNED key of the launch d describes (lim: m_limit_mul of a row-limited launch, else None).  A launch with an MFMA-form
    head is keyed by the head's rows alone."""
    if d.head_wf:
        opts = ('head2', d.head_rows)
    else:
        opts = ((('lim', lim) if lim is not None else ()) + (('x2', cw.cin2, cw.stride2, d.H2, d.W2) if d.x2 else ())
                + (('up',) if d.up_top else ()))
    return _shape_key(cw, d.B, d.H, d.W, d.OH, d.OW, d.x_cstride, precision, (d.x_format, d.y_format, d.res_format) + opts + tune_mode_key())


def _choose_plan(d, cw, precision, device, plan=None, lim=None):
    """The plan (tile_mr, tile_nr, waves, stages, splits) for the launch the filled descriptor d describes; (0, 0, 0, 0, 0) leaves the
    choice to the library's heuristic.  plan: the caller's explicit plan, if any (tests, tools, fused launches).  lim: m_limit_mul of
    a row-limited launch -- the limit itself is not in d yet, the tuner puts its own there."""
    if d.up_top and plan is not None and tuple(plan) != (0, 0, 0, 0, 0):
        # the addition lives in the conv kernel's epilogue of every tile but 256x256 and the 4-wave 256x128 / 128x256 (the tiles
        # with the vector epilogue only: conv_f16s_plan_ok), never in the split-K reduction: an explicit plan is rewritten here
        # (not silently replaced by the library's heuristic), so that the returned plan is the one that ran
        big = tuple(plan[:2]) == (4, 4) or (tuple(plan[:3]) in ((4, 2, 4), (2, 4, 4)))
        plan = ((4, 2, 8, 3) if big else tuple(plan[:4])) + (1,)
    if d.head_w:                          # the fp32-FMA fused head lives in the 256x256 tile, whatever was asked for
        return (4, 4, 8, 2, 1)
    if plan is not None:                  # explicit
        return tuple(plan)
    if not AUTOTUNE:
        return (0, 0, 0, 0, 0)
    if d.head_wf and not d.head_parts:    # final MFMA head: the 256x256 tile owns the pixel's channels -- nothing to tune
        return (4, 4, 8, 2, 1)
    key = _plan_key(cw, d, precision, lim)
    if KEY_HITS is not None:
        KEY_HITS[key] = KEY_HITS.get(key, 0) + 1
    plan = _TUNED.get(key)
    if plan is not None:
        return plan
    # never time inside a graph capture / program recording; warm-up runs tune first
    recording = torch.cuda.is_current_stream_capturing() or _lib.lib().srcnn_program_recording()
    if d.head_wf:                         # partial MFMA head: the 256x256 or the 128x128 8-wave tile
        if recording:
            return (4, 4, 8, 2, 1) if d.B * d.OH * d.OW >= 2048 else (2, 2, 8, 2, 1)
        return _tune(d, key, device, only=[(4, 4, 8, 2), (2, 2, 8, 2)])
    if recording:
        return (0, 0, 0, 0, 0)
    if lim is not None:
        # a launch with a device-side row limit is tuned WITH a typical limit (LIMIT_TUNE_ROIS of its units): what is fastest for
        # the whole shape (the biggest tile, one round of CUs) is not what is fastest for a fifth of it
        typical = torch.tensor([LIMIT_TUNE_ROIS], dtype=torch.int32, device=device)
        d.m_limit, d.m_limit_mul = typical.data_ptr(), int(lim)
    plan = _tune(d, key, device)
    d.m_limit, d.m_limit_mul = None, 0
    return plan


def _issue(launch, what, name):
    """Issues a launch -- launch() calls the library and returns its status -- and the extra copies REPEAT asks for."""
    _lib.check(launch(), what)
    if REPEAT and name:
        for rx, n in REPEAT:
            if rx.match(name):
                for _ in range(n):
                    _lib.check(launch(), what + "(repeat)")


def conv2d(cw, x, B, H, W, y, OH, OW, x_cstride=None, y_cstride=None, y_coffset=0, residual=None,
           res_cstride=None, x_offset_elems=0, relu=None, precision=None, x_fmt=0, y_fmt=0, res_fmt=0, plan=None, name=None,
           in_shift=0, out_shift=0, m_limit=None, m_limit_mul=0, x2=None, H2=0, W2=0, x2_cstride=None, head=None, head2=None, up=None,
           desc_only=False):
    """Launch the conv engine.  x / y / residual are device tensors (any shape; raw NHWC memory).
    *_fmt: _lib.FMT_F32 or _lib.FMT_SPLIT16 (f16x3 engine only; see include/srcnn_hip.h).
    in_shift / out_shift (f16x3 engine): the input tensor holds its values x 2^in_shift, the output (and the residual, which
    must carry the output's scale) is to be stored x 2^out_shift -- per-tensor power-of-two activation scales that keep
    SPLIT16 tensors in the middle of the f16 range (model/stereo_rcnn/plan.py: calibrate).  Exact: the factor goes into the
    epilogue's power-of-two rescale and a pre-scaled copy of the bias; ReLU commutes with it.
    m_limit (device int32 tensor) / m_limit_mul: only rows m < m_limit[0] * m_limit_mul are needed (srcnn_conv_desc.m_limit).
    x2 / H2 / W2 (weights from prep_conv_shortcut): the second input (B, H2, W2, cin2) SPLIT16, stored with the SAME scale as x.
    head = (cw_head, y_head) (f16x3 SPLIT16 engine): a 6-channel 1x1 conv applied to the activated output pixels inside this
    launch's epilogue (srcnn_conv_desc.head_w); y_head (pixels, 6) float32 receives it, y is not written (may be None).
    head2 = (cw_head, y_head, parts) (f16x3 SPLIT16 engine): the MFMA form of such a head (srcnn_conv_desc.head_wf), up to 24
    channels.  parts = 0: final (256-channel pixels; bias added; y_head (pixels, n) float32); parts > 0: y_head (parts, pixels, n)
    float32 receives one plane of partial sums per (eye, N tile) of the launch -- the caller adds them and the bias.
    up = (top, TH, TW, top_fmt) (f16x3 SPLIT16 engine): the FPN top-down addition inside this launch (srcnn_conv_desc.up_top):
    y = bilinear_align_corners(top (B, TH, TW, cout) -> (OH, OW)) + (conv + bias), top stored with the OUTPUT's scale; bit-identical
    to conv2d (float32 y) followed by upsample_add.
    desc_only (with an explicit plan): nothing is launched or counted; returns the filled descriptor (conv_chain / conv_group).
    Returns the plan the launch ran with: (tile_mr, tile_nr, waves, stages, splits)."""
    L = _lib.lib()
    d = _lib.ConvDesc()
    d.x = x.data_ptr() + 4 * x_offset_elems
    precision = PRECISION if precision is None else precision
    if precision == 'f16x3':
        cw.split_f16x3()
        d.w, d.w_lo, d.w_inv_scale, d.precision = cw.w_hi.data_ptr(), cw.w_lo.data_ptr(), cw.inv_scale * 2.0 ** (out_shift - in_shift), 1
    else:
        assert in_shift == 0 and out_shift == 0, "activation scales belong to the f16x3 engine's SPLIT16 tensors"
        d.w, d.w_lo, d.w_inv_scale, d.precision = cw.weight.data_ptr(), None, 1.0, 0
    bias = cw.bias
    if bias is not None and out_shift:
        cache = cw.__dict__.setdefault('_bias_shifted', {})
        bias = cache.get(out_shift)
        if bias is None:
            bias = cache[out_shift] = (cw.bias * 2.0 ** out_shift).contiguous()
    d.bias = bias.data_ptr() if bias is not None else None
    d.residual = residual.data_ptr() if residual is not None else None
    d.y = y.data_ptr() if y is not None else None
    if head is not None:
        hcw, hy = head
        assert precision == 'f16x3' and x_fmt == _lib.FMT_SPLIT16 and hcw.cout == 6 and hcw.kh == 1 and hcw.kw == 1 and hcw.bias is not None
        assert hy.dtype == torch.float32 and hy.is_contiguous()
        d.head_w, d.head_bias, d.head_y = hcw.weight.data_ptr(), hcw.bias.data_ptr(), hy.data_ptr()
        d.head_cout, d.head_scale = 6, 2.0 ** -out_shift
        y_fmt = _lib.FMT_F32
    if head2 is not None:
        hcw, hy, parts = head2
        assert head is None and precision == 'f16x3' and x_fmt == _lib.FMT_SPLIT16 and hcw.kh == 1 and hcw.kw == 1
        assert hy.dtype == torch.float32 and hy.is_contiguous()
        frag, rows = head_fragments(hcw)
        d.head_wf, d.head_rows, d.head_cout, d.head_parts = frag.data_ptr(), rows, hcw.cout, int(parts)
        d.head_plane = hy.numel() // parts if parts else 0
        d.head_bias = hcw.bias.data_ptr() if (hcw.bias is not None and not parts) else None
        d.head_y, d.head_scale = hy.data_ptr(), hcw.inv_scale * 2.0 ** -out_shift
        y_fmt = _lib.FMT_F32
    d.B, d.H, d.W, d.Cin = B, H, W, cw.cin
    d.x_cstride = cw.cin if x_cstride is None else x_cstride
    d.OH, d.OW, d.Cout = OH, OW, cw.cout
    d.KH, d.KW, d.stride, d.pad = cw.kh, cw.kw, cw.stride, cw.pad
    cq = cw.cout // 4 if cw.mode == 1 else cw.cout
    d.y_cstride = cq if y_cstride is None else y_cstride
    d.y_coffset = y_coffset
    d.res_cstride = cw.cout if res_cstride is None else res_cstride
    d.relu = cw.relu if relu is None else int(relu)
    d.mode = cw.mode
    d.x_format, d.y_format, d.res_format = x_fmt, y_fmt, res_fmt
    d.layer_tag = layer_tag(name)
    assert (x2 is not None) == (cw.cin2 > 0), "weights from prep_conv_shortcut need the second input, and only they take one"
    if x2 is not None:
        assert precision == 'f16x3' and x_fmt == _lib.FMT_SPLIT16, "the second input belongs to the SPLIT16 engine"
        d.x2, d.Cin2, d.H2, d.W2, d.stride2 = x2.data_ptr(), cw.cin2, H2, W2, cw.stride2
        d.x2_cstride = cw.cin2 if x2_cstride is None else x2_cstride
    if up is not None:
        top, th, tw, top_fmt = up
        assert precision == 'f16x3' and x_fmt == _lib.FMT_SPLIT16 and residual is None and head is None and head2 is None and cw.mode == 0
        d.up_top, d.up_format, d.up_H, d.up_W = top.data_ptr(), int(top_fmt), int(th), int(tw)
    if desc_only:
        assert plan is not None and head is None and m_limit is None
    _set_plan(d, _choose_plan(d, cw, precision, x.device, plan, m_limit_mul if m_limit is not None else None))
    if desc_only:
        return d
    if m_limit is not None:               # after the plan: the tuner times the launch with a typical limit (_choose_plan)
        assert m_limit.is_cuda and m_limit.dtype == torch.int32 and m_limit_mul > 0
        d.m_limit, d.m_limit_mul = m_limit.data_ptr(), int(m_limit_mul)
    used = (d.tile_mr, d.tile_nr, d.tile_waves, d.tile_stages, d.splits)
    _book(name or 'conv %dx%d %d->%d' % (cw.kh, cw.kw, cw.cin, cw.cout),
          *conv_cost(cw, B, H, W, OH, OW, residual is not None, up, head is not None, head2), plan=used)
    ws = _lib.workspace(L.srcnn_conv2d_workspace_bytes(ctypes.byref(d)), x.device, "conv")
    _issue(lambda: L.srcnn_conv2d(ctypes.byref(d), ws.data_ptr(), ws.numel(), _lib.stream()), "srcnn_conv2d", name)
    return used


def resolved_plan(d):
    """The plan (tile_mr, tile_nr, waves, stages, splits) the library launches for the filled descriptor d (srcnn_conv2d_plan).
    It differs from the plan d asks for where the library does not implement that one for this convolution and answers with its
    heuristic plan; a zero plan resolves to the heuristic plan itself.  Nothing is launched."""
    out = (ctypes.c_int * 5)()
    _lib.check(_lib.lib().srcnn_conv2d_plan(ctypes.byref(d), out), "srcnn_conv2d_plan")
    return tuple(out)


def _fill_train_geometry(d, cw, B, H, W, OH, OW, x_cstride, y_cstride, y_coffset, relu, tile):
    """The fields srcnn_conv_bwd_desc and srcnn_conv_fwd_f16x3_desc share, from a ConvW and the call's strides."""
    d.B, d.H, d.W, d.Cin = B, H, W, cw.cin
    d.x_cstride = cw.cin if x_cstride is None else x_cstride
    d.OH, d.OW, d.Cout = OH, OW, cw.cout
    d.KH, d.KW, d.stride, d.pad = cw.kh, cw.kw, cw.stride, cw.pad
    d.y_cstride = cw.cout if y_cstride is None else y_cstride
    d.y_coffset = y_coffset
    d.relu = cw.relu if relu is None else int(relu)
    if tile is not None:
        d.tile_mr, d.tile_nr = int(tile[0]), int(tile[1])


def conv2d_backward(cw, x, B, H, W, y, dy, OH, OW, want=('dx', 'dw', 'db'), splits=0, x_cstride=None, y_cstride=None, y_coffset=0,
                    relu=None, g_out=None, out=None, tile=None, precision='f32', x_amax=None, prepared=None):
    """Gradients of conv2d(cw, x, ..., precision='f32') (srcnn_conv2d_backward; include/srcnn_hip.h states the sums' orders).
    precision: 'f32', that exact fp32 backward, or 'f16x3', srcnn_conv2d_backward_f16x3 -- the same gradients by the 3 x f16 split
    with per-tensor power-of-two scales found on the device; the one asked for runs, never the other in its place.
    x (B, H, W, *) and dy / y (B, OH, OW, *) are raw NHWC device tensors with the forward's strides; y is the saved forward output
    (needed when relu, else may be None); relu defaults to cw.relu.  want: which of 'dx' (like x: pixel stride x_cstride), 'dw'
    (Cout, KH, KW, Cin) and 'db' (Cout) to compute -- the others are neither computed nor allocated.  g_out: optional dense
    (B, OH, OW, Cout) tensor that receives the masked gradient dy * [y > 0] (the residual branch's gradient).  out: {name: tensor}
    to write into instead of fresh tensors (every element is overwritten).  splits: K slices of the weight gradient (0 = the
    library's choice); tile: (tile_mr, tile_nr).  x_amax (precision 'f16x3' only): a 1-element int32 device tensor holding the float
    bits of max |x| over channels [0, Cin) of all B H W pixels (absmax, or a forward's y_amax): the weight gradient's max |x| pass
    is then not launched (srcnn_conv2d_backward_f16x3_maxima); the gradients keep their bits.  prepared (precision 'f16x3' only):
    the PreparedW prepare_train_weights made from cw.weight: neither the max |w| pass nor the re-layout + split is launched
    (srcnn_conv2d_backward_f16x3_prepared); the gradients keep their bits.  Returns {name: tensor} for the names in want."""
    L = _lib.lib()
    if precision not in ('f32', 'f16x3'):
        raise ValueError("conv2d_backward: precision must be 'f32' or 'f16x3' (got %r)" % (precision,))
    if x_amax is not None and precision != 'f16x3':
        raise ValueError("conv2d_backward: x_amax belongs to precision 'f16x3'")
    entry = 'srcnn_conv2d_backward' if precision == 'f32' else 'srcnn_conv2d_backward_f16x3'
    assert cw.mode == 0 and cw.cin2 == 0, "only plain convolutions have a backward"
    unknown = set(want) - {'dx', 'dw', 'db'}
    assert not unknown, unknown
    d = _lib.ConvBwdDesc()
    xcs = cw.cin if x_cstride is None else x_cstride
    res = dict(out or {})
    if 'dx' in want and 'dx' not in res:
        res['dx'] = torch.empty((B, H, W, xcs), dtype=torch.float32, device=dy.device)
    if 'dw' in want and 'dw' not in res:
        res['dw'] = torch.empty((cw.cout, cw.kh, cw.kw, cw.cin), dtype=torch.float32, device=dy.device)
    if 'db' in want and 'db' not in res:
        res['db'] = torch.empty((cw.cout,), dtype=torch.float32, device=dy.device)
    res = {k: res[k] for k in want}
    d.x = x.data_ptr() if x is not None else None
    d.w = cw.weight.data_ptr()
    d.y = y.data_ptr() if y is not None else None
    d.dy = dy.data_ptr()
    d.dx, d.dw, d.db = (res[k].data_ptr() if k in res else None for k in ('dx', 'dw', 'db'))
    d.g_out = g_out.data_ptr() if g_out is not None else None
    _fill_train_geometry(d, cw, B, H, W, OH, OW, xcs, y_cstride, y_coffset, relu, tile)
    d.splits = int(splits)
    d.precision = 0 if precision == 'f32' else 1
    nbytes = getattr(L, entry + '_workspace_bytes')(ctypes.byref(d))
    ws = _lib.workspace(nbytes, dy.device, "conv_backward")
    if prepared is not None:
        if precision != 'f16x3':
            raise ValueError("conv2d_backward: prepared belongs to precision 'f16x3'")
        _check_prepared(prepared, cw)
        if x_amax is None and 'dw' in want:
            F16X3_MAXIMA['scans'] += 1
        _lib.check(L.srcnn_conv2d_backward_f16x3_prepared(ctypes.byref(d), None if x_amax is None else _amax_ptr(x_amax),
                                                          _amax_ptr(prepared.word), prepared.wt_hi.data_ptr(), prepared.wt_lo.data_ptr(),
                                                          prepared.plane_bytes, ws.data_ptr(), ws.numel(), _lib.stream()),
                   entry + '_prepared')
    elif x_amax is not None:
        _lib.check(L.srcnn_conv2d_backward_f16x3_maxima(ctypes.byref(d), _amax_ptr(x_amax), ws.data_ptr(), ws.numel(), _lib.stream()),
                   entry + '_maxima')
    else:
        if precision == 'f16x3' and 'dw' in want:
            F16X3_MAXIMA['scans'] += 1
        _lib.check(getattr(L, entry)(ctypes.byref(d), ws.data_ptr(), ws.numel(), _lib.stream()), entry)
    return res


# The f16x3 training calls' max |x|: host counters of the passes over an activation that were issued ('scans': inside a call that
# was given no word, or by absmax) and of the calls that needed max |x| and were served by a word older than themselves ('reused',
# counted by the owner of the words -- autograd's record -- since only it knows where a word came from).
F16X3_MAXIMA = {'scans': 0, 'reused': 0}


def reset_f16x3_maxima():
    F16X3_MAXIMA['scans'] = F16X3_MAXIMA['reused'] = 0


def _amax_ptr(word):
    assert word.is_cuda and word.dtype == torch.int32 and word.numel() == 1, "a max word is a 1-element int32 device tensor"
    return word.data_ptr()


def absmax(x, cin=None, x_cstride=None):
    """max |x| over channels [0, cin) of every pixel of x (..., x_cstride) (srcnn_absmax; defaults: x's last dimension for both) as
    a fresh 1-element int32 device tensor holding the float's bits -- the word conv2d_train_f16x3 and conv2d_backward(precision=
    'f16x3') take as x_amax.  Floats behind cin are not read; NaNs are dropped; an all-zero x gives 0.  Nothing is read by the host."""
    xcs = int(x.shape[-1]) if x_cstride is None else int(x_cstride)
    cin = xcs if cin is None else int(cin)
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() % xcs == 0
    word = torch.empty(1, dtype=torch.int32, device=x.device)
    F16X3_MAXIMA['scans'] += 1
    _lib.check(_lib.lib().srcnn_absmax(x.data_ptr(), x.numel() // xcs, cin, xcs, word.data_ptr(), _lib.stream()), "srcnn_absmax")
    return word


class PreparedW(object):
    """One layer of prepare_train_weights: `weight`, the fp32 (Cout, KH, KW, Cin) tensor the planes were made from (detached); `word`,
    a 1-element int32 view holding the float bits of max |w|; the forward planes w_hi / w_lo (Cp, KH KW, Cin) and the backward planes
    wt_hi / wt_lo (Cin, KH KW, Cp), float16, Cp = Cout rounded up to 32; plane_bytes, the bytes of each.  Valid until the weight
    changes: it is not a cache, whoever changes the weight prepares again."""
    __slots__ = ('weight', 'word', 'w_hi', 'w_lo', 'wt_hi', 'wt_lo', 'plane_bytes')

    def __init__(self, weight, word, w_hi, w_lo, wt_hi, wt_lo):
        self.weight, self.word, self.w_hi, self.w_lo, self.wt_hi, self.wt_lo = weight, word, w_hi, w_lo, wt_hi, wt_lo
        self.plane_bytes = w_hi.numel() * 2


def _check_prepared(prepared, cw):
    if prepared.weight.data_ptr() != cw.weight.data_ptr() or tuple(prepared.weight.shape) != (cw.cout, cw.kh, cw.kw, cw.cin):
        raise ValueError("prepared: the planes were not made from this weight tensor (%s at %#x)"
                         % (tuple(prepared.weight.shape), prepared.weight.data_ptr()))


def prepare_train_weights(weights, workspace=None):
    """max |w| and the f16x3 hi / lo planes of a LIST of weights in one srcnn_train_weights_prepare call (csrc/train_weights.hip): a
    fixed, small number of launches whatever the list's length, nothing read by the host.  weights: contiguous float32 device
    tensors (Cout, KH, KW, Cin) in the engine's layout, BN already folded, Cin a multiple of 32 -- what conv2d_train_f16x3 and
    conv2d_backward take as cw.weight.  Returns one PreparedW per weight for their `prepared=`.  The words of the whole list are one
    int32 tensor and the planes one float16 tensor, carved at 256-byte steps.  workspace: a uint8 device tensor of at least
    srcnn_train_weights_workspace_bytes(len(weights)) bytes for the call's table (default: the shared grow-only scratch)."""
    L = _lib.lib()
    weights = [w.detach() for w in weights]
    if not weights:
        raise ValueError("prepare_train_weights: an empty list")
    dev = weights[0].device
    sizes = []
    for w in weights:
        assert w.is_cuda and w.dtype == torch.float32 and w.dim() == 4 and w.is_contiguous(), "contiguous float32 (Cout, KH, KW, Cin) device tensors"
        cout, kh, kw, cin = (int(v) for v in w.shape)
        sizes.append(-(-((cout + 31) // 32 * 32 * kh * kw * cin) // 128) * 128)          # halves of one plane, rounded up to 256 bytes
    words = torch.empty(64 * len(weights), dtype=torch.int32, device=dev)               # one word per 256 bytes: no two layers share a line
    planes = torch.empty(4 * sum(sizes), dtype=torch.float16, device=dev)
    descs = (_lib.TrainWeightDesc * len(weights))()
    out, off = [], 0
    for i, (w, n) in enumerate(zip(weights, sizes)):
        cout, kh, kw, cin = (int(v) for v in w.shape)
        numel = (cout + 31) // 32 * 32 * kh * kw * cin
        p = PreparedW(w, words[64 * i:64 * i + 1], *(planes[off + j * n:off + j * n + numel] for j in range(4)))
        off += 4 * n
        d = descs[i]
        d.w, d.w_amax = w.data_ptr(), p.word.data_ptr()
        d.w_hi, d.w_lo, d.wt_hi, d.wt_lo = p.w_hi.data_ptr(), p.w_lo.data_ptr(), p.wt_hi.data_ptr(), p.wt_lo.data_ptr()
        d.Cout, d.KH, d.KW, d.Cin = cout, kh, kw, cin
        out.append(p)
    nbytes = L.srcnn_train_weights_workspace_bytes(len(weights))
    ws = _lib.workspace(nbytes, dev, "train_weights") if workspace is None else workspace
    _lib.check(L.srcnn_train_weights_prepare(descs, len(weights), ws.data_ptr(), ws.numel(), _lib.stream()), "srcnn_train_weights_prepare")
    return out


class FoldSpec(object):
    """One layer of fold_train_weights: kind, 'conv' (parts (rows, Cin, KH, KW) -> (Cout, KH, KW, Cin)), 'linear' ((rows, K) ->
    (Cout, 1, 1, K)) or 'deconv2x2' ((Cin, Cout, 2, 2) -> (4 Cout, 1, 1, Cin), row order (i, j, co)); parts, one to three
    (weight, bias or None) pairs concatenated along the output rows; bn, the frozen BatchNorm's dict ('weight', 'bias',
    'running_mean', 'running_var') or None.  The tensors are the PARAMETERS as the modules hold them: contiguous float32 on the
    device.  shape: the folded weight's; has_b: whether a folded bias exists."""
    __slots__ = ('kind', 'parts', 'bn', 'shape', 'has_b')
    KINDS = ('conv', 'linear', 'deconv2x2')

    def __init__(self, kind, parts, bn=None):
        if kind not in self.KINDS:
            raise ValueError("FoldSpec: kind must be one of %s (got %r)" % (', '.join(self.KINDS), kind))
        parts = tuple((w, b) for w, b in parts)
        if not parts:
            raise ValueError("FoldSpec: no parts")
        for t in [w for w, _ in parts] + [b for _, b in parts if b is not None] + list((bn or {}).values()):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "contiguous float32 device tensors"
        w0 = parts[0][0]
        assert all(w.dim() == w0.dim() and w.shape[1:] == w0.shape[1:] for w, _ in parts), "the parts differ in more than their rows"
        assert w0.dim() == (2 if kind == 'linear' else 4), "conv / deconv2x2 weights are 4-d, linear weights 2-d"
        rows = sum(int(w.shape[0]) for w, _ in parts)
        if kind == 'deconv2x2':
            self.shape = (4 * int(w0.shape[1]), 1, 1, int(w0.shape[0]))
        elif kind == 'linear':
            self.shape = (rows, 1, 1, int(w0.shape[1]))
        else:
            self.shape = (rows, int(w0.shape[2]), int(w0.shape[3]), int(w0.shape[1]))
        self.kind, self.parts, self.bn = kind, parts, bn
        self.has_b = bn is not None or parts[0][1] is not None


def _fold_descs(specs):
    specs = list(specs)
    if not specs:
        raise ValueError("fold_train_weights: an empty list")
    descs = (_lib.TrainFoldDesc * len(specs))()
    for d, s in zip(descs, specs):
        d.kind = FoldSpec.KINDS.index(s.kind)                   # _lib.TRAIN_FOLD_CONV, _LINEAR, _DECONV2X2: 0, 1, 2
        d.n_parts = len(s.parts)
        for p, (w, b) in enumerate(s.parts[:3]):
            d.w[p], d.bias[p], d.rows[p] = w.data_ptr(), None if b is None else b.data_ptr(), int(w.shape[1 if s.kind == 'deconv2x2' else 0])
        if s.bn is not None:
            d.bn_weight, d.bn_bias = s.bn['weight'].data_ptr(), s.bn['bias'].data_ptr()
            d.bn_mean, d.bn_var = s.bn['running_mean'].data_ptr(), s.bn['running_var'].data_ptr()
        rows, d.KH, d.KW, d.Cin = s.shape
        d.Cout = rows // 4 if s.kind == 'deconv2x2' else rows
        if s.kind == 'deconv2x2':
            d.KH = d.KW = 2
    return specs, descs


def fold_train_weights(specs, workspace=None):
    """Every layer's folded weight in the engine's layout and its folded bias in ONE srcnn_train_weights_fold call
    (csrc/train_fold.hip, include/srcnn_hip.h): what autograd.fold_conv / fold_linear / fold_deconv2x2 + .contiguous() (and
    torch.cat for several parts) compute, bit for bit, in a fixed number of launches.  specs: FoldSpec's.  Returns [(w, b or None)],
    fresh tensors without a graph (autograd.fold_all is the differentiable form).  workspace: prepare_train_weights's, of
    srcnn_train_fold_workspace_bytes(len(specs)) bytes."""
    L = _lib.lib()
    specs, descs = _fold_descs(specs)
    dev = specs[0].parts[0][0].device
    out = []
    for d, s in zip(descs, specs):
        w = torch.empty(s.shape, dtype=torch.float32, device=dev)
        b = torch.empty(s.shape[0], dtype=torch.float32, device=dev) if s.has_b else None
        d.dst_w, d.dst_b = w.data_ptr(), None if b is None else b.data_ptr()
        out.append((w, b))
    ws = _lib.workspace(L.srcnn_train_fold_workspace_bytes(len(specs)), dev, "train_fold") if workspace is None else workspace
    _lib.check(L.srcnn_train_weights_fold(descs, len(specs), ws.data_ptr(), ws.numel(), _lib.stream()), "srcnn_train_weights_fold")
    return out


def fold_train_weights_backward(specs, dws, dbs, workspace=None):
    """The adjoint of fold_train_weights in ONE srcnn_train_weights_fold_backward call.  dws / dbs: per layer the gradient of the
    folded weight / bias (contiguous float32, the folded tensor's shape) or None.  Returns per layer ([dw of each part], [db of each
    part]) in the parameters' own shapes, contiguous; None where nothing arrived (a None dw: every part's weight; a None db, or a layer
    without a convolution bias: every part's bias -- a frozen BN's tensors receive nothing).  A deconvolution's db is refused: its
    bias stays the caller's bias.repeat(4) (include/srcnn_hip.h, "frozen-BN fold")."""
    L = _lib.lib()
    specs, descs = _fold_descs(specs)
    dws, dbs = list(dws), list(dbs)
    assert len(dws) == len(specs) and len(dbs) == len(specs), "one dw and one db (or None) per layer"
    dev = specs[0].parts[0][0].device
    out = []
    for d, s, dw, db in zip(descs, specs, dws, dbs):
        for g, shape in ((dw, s.shape), (db, s.shape[:1])):
            assert g is None or (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == tuple(shape)), \
                "contiguous float32 device gradients of the folded tensors' shapes"
        gws = [None if dw is None else torch.empty_like(w) for w, _ in s.parts]
        gbs = [None if db is None or b is None else torch.empty_like(b) for _, b in s.parts]
        for p in range(min(len(s.parts), 3)):
            d.grad_w[p] = None if gws[p] is None else gws[p].data_ptr()
            d.grad_b[p] = None if gbs[p] is None else gbs[p].data_ptr()
        out.append((gws, gbs))
    ptrs = lambda gs: (_lib.c_void_p * len(gs))(*[None if g is None else g.data_ptr() for g in gs])
    ws = _lib.workspace(L.srcnn_train_fold_workspace_bytes(len(specs)), dev, "train_fold_backward") if workspace is None else workspace
    _lib.check(L.srcnn_train_weights_fold_backward(descs, len(specs), ptrs(dws), ptrs(dbs), ws.data_ptr(), ws.numel(), _lib.stream()),
               "srcnn_train_weights_fold_backward")
    return out


def conv2d_train_f16x3(cw, x, B, H, W, y, OH, OW, residual=None, x_cstride=None, y_cstride=None, y_coffset=0, relu=None, tile=None,
                       x_amax=None, y_amax=None, prepared=None):
    """The training forward on the f16 matrix pipe (srcnn_conv2d_forward_f16x3): y = relu?(conv(x, w) + bias + residual) by the 3 x f16
    split with one power-of-two scale for x and one for w, both found on the device inside the call -- the scheme of
    conv2d_backward(precision='f16x3').  cw: an engine.ConvW holding the plain fp32 weights (Cout, KH, KW, Cin) (BN folded) and
    bias, mode 0; no prepared planes, no host-side exponent.  x (B, H, W, *) and y (B, OH, OW, *) are raw NHWC float32 device
    tensors; residual dense (B, OH, OW, Cout).  tile: (tile_mr, tile_nr).  It is not conv2d(precision='f16x3'), the inference
    engine, and never runs in its place or lets it run in its own.
    x_amax / y_amax: 1-element int32 device tensors (float bits), never slices of the shared workspace.  x_amax, when given, is
    max |x| over channels [0, Cin) of all B H W pixels and replaces the call's own pass over x; y_amax, when given, is overwritten
    with max |y| over exactly what the call stores (srcnn_conv2d_forward_f16x3_maxima).  prepared: the PreparedW
    prepare_train_weights made from cw.weight -- the call then launches neither its max |w| pass nor its weight split
    (srcnn_conv2d_forward_f16x3_prepared).  y keeps its bits either way."""
    L = _lib.lib()
    assert cw.mode == 0 and cw.cin2 == 0, "only plain convolutions have a training forward"
    d = _lib.ConvFwdF16x3Desc()
    d.x, d.w, d.y = x.data_ptr(), cw.weight.data_ptr(), y.data_ptr()
    d.bias = cw.bias.data_ptr() if cw.bias is not None else None
    d.residual = residual.data_ptr() if residual is not None else None
    _fill_train_geometry(d, cw, B, H, W, OH, OW, x_cstride, y_cstride, y_coffset, relu, tile)
    ws = _lib.workspace(L.srcnn_conv2d_forward_f16x3_workspace_bytes(ctypes.byref(d)), x.device, "conv_forward_f16x3")
    if x_amax is None:
        F16X3_MAXIMA['scans'] += 1
    if prepared is not None:
        _check_prepared(prepared, cw)
        _lib.check(L.srcnn_conv2d_forward_f16x3_prepared(ctypes.byref(d), None if x_amax is None else _amax_ptr(x_amax),
                                                         None if y_amax is None else _amax_ptr(y_amax), _amax_ptr(prepared.word),
                                                         prepared.w_hi.data_ptr(), prepared.w_lo.data_ptr(), prepared.plane_bytes,
                                                         ws.data_ptr(), ws.numel(), _lib.stream()), "srcnn_conv2d_forward_f16x3_prepared")
    elif x_amax is None and y_amax is None:
        _lib.check(L.srcnn_conv2d_forward_f16x3(ctypes.byref(d), ws.data_ptr(), ws.numel(), _lib.stream()), "srcnn_conv2d_forward_f16x3")
    else:
        _lib.check(L.srcnn_conv2d_forward_f16x3_maxima(ctypes.byref(d), None if x_amax is None else _amax_ptr(x_amax),
                                                       None if y_amax is None else _amax_ptr(y_amax), ws.data_ptr(), ws.numel(),
                                                       _lib.stream()), "srcnn_conv2d_forward_f16x3_maxima")
    return y


def chain_enabled():
    if BOTTLENECK_CHAIN == 'auto':
        from . import streams
        return streams.pairs_in_flight() > 1
    return BOTTLENECK_CHAIN not in ('0', '', 'off')


def chain_tile(planes, M):
    """The chain tile of a bottleneck with `planes` channels and M output rows, or None."""
    t = CHAIN_TILES.get(planes)
    if t is None or -(-M // (64 * t[0])) < CHAIN_MIN_WGS:
        return None
    return t


def _fused_descs(problems, plan_of, chained):
    """The descriptors of a chained / grouped launch of problems = [(args, kwargs)] as for conv2d, each on the tile plan_of(its ConvW),
    with what FlopCounter books for it: (descs, default name, flops, bytes, [(name, M, N, K) per problem])."""
    descs = (_lib.ConvDesc * len(problems))()
    flops = nbytes = 0.0
    rows = []
    for i, (args, kw) in enumerate(problems):
        cw, B, H, W, OH, OW = args[0], args[2], args[3], args[4], args[6], args[7]
        kw = dict(kw)
        pname = kw.pop('name', None)
        d = conv2d(*args, plan=plan_of(cw), desc_only=True, name=pname, **kw)
        ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(d), ctypes.sizeof(d))
        fl, by, M, N, K = conv_cost(cw, B, H, W, OH, OW, kw.get('residual') is not None, head2=kw.get('head2'),
                                    first_in_chain=not (chained and i), grouped=not chained)
        flops += fl
        nbytes += by
        rows.append((pname, M, N, K))
    return descs, '+'.join(str(r[0]) for r in rows), flops, nbytes, rows


def conv_chain(phases, tile, name=None):
    """ONE launch for up to three convolutions over the same rows (srcnn_conv2d_chain): phases = [(args, kwargs)] exactly as they
    would be passed to conv2d, in order; phase i > 0 must be a 1x1 / stride 1 convolution of phase i-1's output.  tile = (tile_mr,
    waves, stages, narrow nr, wide nr): a phase runs on the wide N tile when its Cout fills it (Cout >= 64 * wide nr), else on the
    narrow one.  Results are bit-identical to the separate launches with the same tiles."""
    L = _lib.lib()
    mr, waves, stages, na, nb = tile
    descs, joined, flops, nbytes, rows = _fused_descs(phases, lambda cw: (mr, nb if cw.cout >= 64 * nb else na, waves, stages, 1), True)
    _book(name or joined, flops, nbytes, rows[0][1], max(r[2] for r in rows), sum(r[3] for r in rows), (mr, nb, waves, stages, 1), chain=rows)
    _issue(lambda: L.srcnn_conv2d_chain(descs, len(phases), _lib.stream()), "srcnn_conv2d_chain", name)
    return tile


def conv_group(problems, tile, name=None):
    """ONE launch for up to five independent convolutions that share a tile (srcnn_conv2d_group): problems = [(args, kwargs)] as
    for conv2d; tile = (tile_mr, tile_nr, waves, stages).  Each result is bit-identical to its own launch with that tile."""
    L = _lib.lib()
    plan = tuple(tile) + (1,)
    descs, joined, flops, nbytes, rows = _fused_descs(problems, lambda cw: plan, False)
    _book(name or joined, flops, nbytes, sum(r[1] for r in rows), rows[0][2], rows[0][3], plan, group=rows)
    _issue(lambda: L.srcnn_conv2d_group(descs, len(problems), _lib.stream()), "srcnn_conv2d_group", name)
    return plan


def preprocess_size(H, W, target_short=600):
    """(OH, OW, im_scale) of the reference's resize: im_scale = target / short side (demo.py:113-114), output size as
    cv2.resize derives it from fx/fy: cvRound(H*s), cvRound(W*s) -- Python's round() is the same ties-to-even."""
    scale = float(target_short) / float(min(H, W))
    return int(round(H * scale)), int(round(W * scale)), scale


def preprocess(img_rgb_u8, target_short=600, max_size=2484, packed=None, packed_fmt=0, planar=True):
    """A0 on the device: uint8 RGB (H, W, 3) device tensor -> (1, 3, OH, OW) float32 network input and im_scale
    (demo.py:103-129: RGB->BGR, -PIXEL_MEANS, cv2.resize INTER_LINEAR so that the short side is `target_short`;
    bit-equal to the OpenCV restatement oracle/preprocess.py).  `packed`: optional pre-allocated stem input buffer
    ((OH+6) x (OW+8) x 4 floats, see srcnn_stem_pack) written in the same pass in `packed_fmt` (the fused form);
    planar=False skips the float32 planes (detector-only callers that feed the stem through `packed`)."""
    assert img_rgb_u8.is_cuda and img_rgb_u8.dtype == torch.uint8 and img_rgb_u8.dim() == 3
    img = img_rgb_u8.contiguous()
    H, W = int(img.shape[0]), int(img.shape[1])
    OH, OW, scale = preprocess_size(H, W, target_short)
    out = torch.empty((1, 3, OH, OW), dtype=torch.float32, device=img.device) if planar else None
    _lib.check(_lib.lib().srcnn_preprocess(img.data_ptr(), H, W, scale, out.data_ptr() if planar else None, OH, OW,
                                           packed.data_ptr() if packed is not None else None, packed_fmt, _lib.stream()),
               "srcnn_preprocess")
    if planar and OW > max_size:                       # blob.py:59-61 (inert for KITTI)
        out = out[:, :, :, :max_size].contiguous()
    return out, scale


def preprocess_train(pairs, flipped, scales, max_size=2484, device=None, out=None):
    """The image blobs of a training batch in one launch (minibatch._get_image_blob + blob.im_list_to_blob; csrc/loader.hip).
    pairs: per slot (left, right) uint8 RGB (H, W, 3) tensors -- on the device, or page-locked host tensors the kernel reads where
    they are (then give `device`); flipped: per slot; scales: per slot the Python float target / short side.  Returns
    (im_left, im_right) float32 (B, 3, Hmax, Wmax), zero-padded to the batch maximum, and the per-slot (OH, OWc): each image's
    own resized height and its width after the max_size crop.  Bit-equal to oracle/preprocess.py per image.  `out`: the two
    (B, 3, Hmax, Wmax) tensors to write into (every element is written)."""
    B = len(pairs)
    assert B == len(flipped) == len(scales) and 0 < B <= _lib.LOADER_MAX_BATCH
    slots, sizes = (_lib.TrainImage * B)(), []
    for b, ((l, r), f, s) in enumerate(zip(pairs, flipped, scales)):
        assert l.dtype == torch.uint8 and l.dim() == 3 and l.shape[2] == 3 and tuple(l.shape) == tuple(r.shape)
        assert l.is_contiguous() and r.is_contiguous() and (l.is_cuda or l.is_pinned()) and (r.is_cuda or r.is_pinned())
        if l.is_cuda:
            device = l.device
        H, W = int(l.shape[0]), int(l.shape[1])
        slots[b] = _lib.TrainImage(l.data_ptr(), r.data_ptr(), H, W, int(bool(f)), float(s))
        sizes.append((int(round(H * float(s))), min(int(round(W * float(s))), int(max_size))))
    assert device is not None, "page-locked host images: say which device reads them"
    Hmax, Wmax = max(s[0] for s in sizes), max(s[1] for s in sizes)
    if out is None:
        out = (torch.empty((B, 3, Hmax, Wmax), dtype=torch.float32, device=device),      # the kernel writes every element
               torch.empty((B, 3, Hmax, Wmax), dtype=torch.float32, device=device))
    out_l, out_r = out
    assert all(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (B, 3, Hmax, Wmax) for t in out)
    _lib.check(_lib.lib().srcnn_preprocess_train(slots, B, Hmax, Wmax, int(max_size), out_l.data_ptr(), out_r.data_ptr(), _lib.stream()),
               "srcnn_preprocess_train")
    return out_l, out_r, sizes


def gt_batch(table, slots, keys, K, out=None):
    """The ground-truth tensors of a training batch in one launch (minibatch.py:47-82, roibatchLoader.py:72-110; csrc/loader.hip).
    table: (rows, GT_COLS) float32 device tensor (data.pack_gt_table); slots: per batch slot (row_begin, n, im_scale, im_width);
    keys: (B, key_stride) device tensor of uint32 shuffle keys, the words held in a 4-byte integer dtype (data.keys_to_words).
    Returns [gt_boxes_left, gt_boxes_right, gt_boxes_merge (B, K, 5), gt_dim_orien (B, K, 5), gt_kpts (B, K, 6), num_boxes (B) int64];
    `out`: the same six tensors to write into (every element is written)."""
    B = len(slots)
    assert 0 < B <= _lib.LOADER_MAX_BATCH
    assert table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2 and table.shape[1] == _lib.GT_COLS
    assert keys.is_cuda and keys.is_contiguous() and keys.element_size() == 4 and keys.dim() == 2 and keys.shape[0] == B
    dev = table.device
    if out is None:
        out = [torch.empty((B, K, c), dtype=torch.float32, device=dev) for c in (5, 5, 5, 5, 6)]
        out.append(torch.empty((B,), dtype=torch.int64, device=dev))
    arr = (_lib.GtSlot * B)(*[_lib.GtSlot(int(s[0]), int(s[1]), float(s[2]), float(s[3])) for s in slots])
    _lib.check(_lib.lib().srcnn_gt_batch(table.data_ptr(), int(table.shape[0]), arr, B, keys.data_ptr(), int(keys.shape[1]), int(K),
                                         *[t.data_ptr() for t in out], _lib.stream()), "srcnn_gt_batch")
    return out


def bev_geometry(H):
    """The bird's-eye view's geometry for an image of H rows, in Python float64 as the reference takes it (demo.py:229 passes
    width = 2 H; vis_3d_utils.py:44, 56-60): (res, x_max, y_max, x_off, y_off)."""
    import math
    width = 2 * int(H)
    res = 70.0 / width
    return res, int(40 / res), int(70 / res), int(math.floor(-20 / res)), int(math.floor(70 / res)) - 1


def _device_u8(t, what):
    if not t.is_cuda:
        raise NotImplementedError("%s on %s: the overlay kernels run on the GPU only" % (what, t.device))
    assert t.dtype == torch.uint8 and t.is_contiguous(), "%s must be a contiguous uint8 tensor" % what


def bev_lidar(points, velo_to_cam2, H, out=None):
    """The gray bird's-eye plane of a lidar cloud (kitti_utils.get_point_cloud + vis_3d_utils.vis_lidar_in_bev; csrc/overlay.hip).
    points: (N, 4) float32 device tensor (x, y, z, intensity), N may be 0; velo_to_cam2: the 3x4 (or 4x4) float64 velodyne ->
    camera-2 matrix (kitti_utils.velo_to_cam2); H: the image height the plane stands beside.  Returns the (y_max, x_max) uint8
    plane: 255, 100 where a point falls."""
    import numpy as np
    if not points.is_cuda:
        raise NotImplementedError("bev_lidar on %s: the overlay kernels run on the GPU only" % points.device)
    assert points.dtype == torch.float32 and points.is_contiguous() and points.dim() == 2 and points.shape[1] == 4
    res, x_max, y_max, x_off, y_off = bev_geometry(H)
    if out is None:
        out = torch.empty((y_max, x_max), dtype=torch.uint8, device=points.device)
    _device_u8(out, "bev_lidar plane")
    assert tuple(out.shape) == (y_max, x_max)
    m = (_lib.c_double * 12)(*[float(v) for v in np.asarray(velo_to_cam2, np.float64)[:3].reshape(-1)])
    n = int(points.shape[0])
    _lib.check(_lib.lib().srcnn_bev_lidar(points.data_ptr() if n else None, n, m, res, x_max, y_max, x_off, y_off, out.data_ptr(),
                                          _lib.stream()), "srcnn_bev_lidar")
    return out


def render_overlay(left_u8, right_u8, record, p2, vis_thresh=0.7, bev_plane=None, bev=True, layers=7, rows_per_thread=0, out=None):
    """The result picture of one pair, drawn on the device from its detection record (demo.py:225-333; csrc/overlay.hip,
    include/srcnn_hip.h "result visualisation" states the drawing model and the rasterisation rule).  left_u8 / right_u8: uint8 RGB
    (H, W, 3) device tensors; record: (max_det + 1, REC_COLS) float32 device tensor; p2: the 3x4 P2; bev_plane: bev_lidar's
    plane or None = white; bev=False: no bird's-eye columns (the panel is (2 H, W, 3)).  Returns the uint8 RGB panel
    (2 H, W + x_max, 3).  Raises ValueError where the reference's int(70 / res) is not 2 H: the reference's np.concatenate fails there."""
    import numpy as np
    for t, what in ((left_u8, "render_overlay left image"), (right_u8, "render_overlay right image")):
        _device_u8(t, what)
    if not record.is_cuda:
        raise NotImplementedError("render_overlay on %s: the overlay kernels run on the GPU only" % record.device)
    assert left_u8.dim() == 3 and left_u8.shape[2] == 3 and tuple(left_u8.shape) == tuple(right_u8.shape)
    assert record.dtype == torch.float32 and record.is_contiguous() and record.dim() == 2 and record.shape[1] == _lib.REC_COLS
    assert record.shape[0] >= 1
    H, W = int(left_u8.shape[0]), int(left_u8.shape[1])
    res, x_max, y_max, x_off, y_off = bev_geometry(H)
    if not bev:
        x_max, bev_plane = 0, None
    elif y_max != 2 * H:
        raise ValueError("int(70 / res) = %d is not 2 H = %d: the bird's-eye view cannot stand beside the two images" % (y_max, 2 * H))
    if bev_plane is not None:
        _device_u8(bev_plane, "render_overlay bev plane")
        assert tuple(bev_plane.shape) == (y_max, x_max)
    dev = left_u8.device
    if out is None:
        out = torch.empty((2 * H, W + x_max, 3), dtype=torch.uint8, device=dev)          # the kernel writes every byte
    _device_u8(out, "render_overlay panel")
    assert tuple(out.shape) == (2 * H, W + x_max, 3)
    max_det = int(record.shape[0]) - 1
    L = _lib.lib()
    ws = _lib.workspace(L.srcnn_overlay_workspace_bytes(max_det), dev, "overlay")
    p = (_lib.c_double * 12)(*[float(v) for v in np.asarray(p2, np.float64).reshape(-1)[:12]])
    _lib.check(L.srcnn_render_overlay(left_u8.data_ptr(), right_u8.data_ptr(), H, W, record.data_ptr(), max_det, _lib.REC_COLS, p,
                                      float(vis_thresh), bev_plane.data_ptr() if bev_plane is not None else None, res, x_max, y_max,
                                      x_off, y_off, int(layers), int(rows_per_thread), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _lib.stream()), "srcnn_render_overlay")
    return out


def stem_pack(im_nchw, out, batch_offset=0, out_fmt=0):
    """NCHW image -> zero-bordered NHWC4 for the stem conv; out_fmt FMT_SPLIT16 writes the same buffer in the layout the
    DMA conv engine reads (pass x_fmt=FMT_SPLIT16 to conv2d)."""
    B, C, H, W = im_nchw.shape
    assert C == 3
    L = _lib.lib()
    off = batch_offset * (H + 6) * (W + 8) * 4 * 4
    _lib.check(L.srcnn_stem_pack(_lib.ptr(im_nchw), B, H, W, out.data_ptr() + off, out_fmt, _lib.stream()),
               "srcnn_stem_pack")


def stem_pack_pair(left_nchw, right_nchw, out, out_fmt=0):
    """Both eyes of a stereo batch in one launch: out (2B, H+6, W+8, 4) = lefts, then rights."""
    B, C, H, W = left_nchw.shape
    assert C == 3 and tuple(right_nchw.shape) == tuple(left_nchw.shape)
    _lib.check(_lib.lib().srcnn_stem_pack_pair(_lib.ptr(left_nchw), _lib.ptr(right_nchw), B, H, W, out.data_ptr(), out_fmt, _lib.stream()),
               "srcnn_stem_pack_pair")


def maxpool3x3s2_ceil(x, B, H, W, C, y, OH, OW, y_fmt=0):
    _lib.check(_lib.lib().srcnn_maxpool3x3s2_ceil(x.data_ptr(), B, H, W, C, y.data_ptr(), OH, OW, y_fmt,
                                                  _lib.stream()), "srcnn_maxpool3x3s2_ceil")


def upsample_add(top, TH, TW, lateral, B, H, W, C, y, top_fmt=0, y_fmt=0):
    _lib.check(_lib.lib().srcnn_upsample_add(top.data_ptr(), TH, TW, lateral.data_ptr(), B, H, W, C, y.data_ptr(),
                                             top_fmt, y_fmt, _lib.stream()), "srcnn_upsample_add")


def act_convert(x, x_fmt, y_fmt):
    """NHWC activation tensor (.., C) F32 <-> SPLIT16 (same shape / byte size; the SPLIT16 tensor is an
    opaque float32-typed buffer)."""
    C = int(x.shape[-1])
    pixels = x.numel() // C
    y = torch.empty_like(x)
    _lib.check(_lib.lib().srcnn_act_convert(_lib.ptr(x), x_fmt, y.data_ptr(), y_fmt, pixels, C, _lib.stream()),
               "srcnn_act_convert")
    return y


def pyramid_roi_align(maps, hw, C, im_height, rois, n_rois, A, out, cstride, coffset, x_fmt=0, y_fmt=0, limit=None):
    """ROIAlign over the four pyramid levels P2..P5 (level routing, lattice sampling, 2x2 average; srcnn_pyramid_roi_align): maps =
    the levels' NHWC maps (tensors or device addresses) of sizes hw = [(h, w)] and C channels, rois (n_rois, 5) -> A x A x C per roi
    into channels [coffset, coffset + C) of `out` rows of cstride channels.  limit: device int32 row limit, or None."""
    _lib.check(_lib.lib().srcnn_pyramid_roi_align(_lib.ptr_array(maps), _lib.int_array(h for h, _ in hw), _lib.int_array(w for _, w in hw), C,
                                                  im_height, rois.data_ptr(), n_rois, A, out.data_ptr(), cstride, coffset, x_fmt, y_fmt,
                                                  None if limit is None else limit.data_ptr(), _lib.stream()), "srcnn_pyramid_roi_align")


def subsample2(x, B, H, W, C, y, OH, OW):
    _lib.check(_lib.lib().srcnn_subsample2(x.data_ptr(), B, H, W, C, y.data_ptr(), OH, OW, _lib.stream()),
               "srcnn_subsample2")


def nhwc_to_nchw(x_nhwc):
    """(B,H,W,C) contiguous -> new (B,C,H,W) contiguous tensor (API-edge helper)."""
    B, H, W, C = x_nhwc.shape
    y = torch.empty((B, C, H, W), dtype=x_nhwc.dtype, device=x_nhwc.device)
    _lib.check(_lib.lib().srcnn_nhwc_to_nchw(_lib.ptr(x_nhwc), B, H, W, C, y.data_ptr(), _lib.stream()),
               "srcnn_nhwc_to_nchw")
    return y


def nchw_to_nhwc(x_nchw):
    B, C, H, W = x_nchw.shape
    y = torch.empty((B, H, W, C), dtype=x_nchw.dtype, device=x_nchw.device)
    _lib.check(_lib.lib().srcnn_nchw_to_nhwc(_lib.ptr(x_nchw), B, C, H, W, y.data_ptr(), _lib.stream()),
               "srcnn_nchw_to_nhwc")
    return y
