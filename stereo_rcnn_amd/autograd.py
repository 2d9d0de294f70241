"""Differentiable convolution, linear, FPN top-down and deconvolution layers on the exact-fp32 HIP engine.

Every learnable layer of the network goes through the conv engine (the ResNet and FPN convs, RPN_Conv and its heads, RCNN_top,
the linear heads, the keypoint tower).  These functions are that engine with a backward: the forward is `engine.conv2d(...,
precision='f32')`, the backward `engine.conv2d_backward` (srcnn_conv2d_backward: dx, dw, db on the fp32 MFMA; include/srcnn_hip.h
states the sums and their order) or, with backward_precision='f16x3', srcnn_conv2d_backward_f16x3 (the same gradients by the
error-compensated 3 x f16 split).  forward_precision='f16x3' runs the forward as `engine.conv2d_train_f16x3`
(srcnn_conv2d_forward_f16x3): the same split with the scales of x and w found on the device inside the call, so no exponent is
read by the host; the two precisions are independent, and the backward reads the saved x, w and the forward's own y (the ReLU
mask) whichever engine wrote it.  Tensors are NCHW at the edge and NHWC inside, like the ROIAlign modules.  Nothing here waits for
the device.  CPU tensors raise NotImplementedError, as the project's other ops.

conv2d_nhwc is the same convolution NHWC to NHWC: a graph of many layers (stereo_rcnn_amd.training) stays in the engine's layout
and pays no transpose per layer.  upsample_add, subsample2 and conv_transpose2x2 are the three remaining differentiable operators
of the reference's training branch (_upsample_add, MaxPool2d(1, stride 2), ConvTranspose2d(k=2, s=2) + ReLU) over the adjoint
kernels of csrc/train_ops.hip; they are NHWC on both sides.

reuse_maxima (default True; it matters only where a precision is 'f16x3').  The f16x3 calls scale x by a power of two found from
max |x|, and without help every call scans its input for it: the forward, the weight gradient over the same saved x again, and
every further consumer of that tensor likewise.  With reuse_maxima a convolution whose forward is f16x3 has its epilogue leave
max |y| in a device word (engine.conv2d_train_f16x3's y_amax), which is recorded for the tensor it returns; a convolution looks
its input up in that record and hands the word on as x_amax, and a tensor the record does not know is scanned once
(engine.absmax) and recorded, so that its second consumer hits.  The word used for x is kept on ctx and given to the f16x3
backward.  When only the backward is f16x3 the scan therefore moves to the forward -- the same one pass for a tensor with one
consumer, one pass instead of two for a block input that feeds conv1 and downsample -- and it is issued only where a weight
gradient will want it (grad mode on and the weight requires grad).  A maximum does not depend on who computed it: every result
keeps its bits.  engine.F16X3_MAXIMA counts the passes issued and the calls served by an older word.

'auto' (either precision).  choose_engine(direction, M, N, K) names the engine per call from the call's GEMM size -- a closed-form
rule fitted to the measured table in stereo_rcnn_amd/train_engine_table.py -- and the call then runs exactly as if that engine had
been asked for: a layer resolved to fp32 neither scans nor records a maximum, and the next f16x3 consumer of its output scans once.
An explicit 'f32' or 'f16x3' is never replaced.

prepared=.  max |w| and the hi / lo planes of a weight are functions of the weight alone.  engine.prepare_train_weights computes
them for a list of folded weights in one call (csrc/train_weights.hip); a PreparedLayer carries one layer's folded weight (still in
the graph), bias and planes, and a function given it launches no pass over the weight in either direction.  The bits do not change.
Nothing here caches across optimiser steps: optim.SGD writes parameters through raw pointers, which no version counter sees, so
whoever steps prepares again (stereo_rcnn_amd.training.TrainWeights).

fold_all.  fold_conv / fold_linear / fold_deconv2x2 are torch operators per layer (a float64 fold, a permute().contiguous(), a
torch.cat) with their autograd nodes.  fold_all(specs) is the same for a whole list of layers as ONE node over two library calls
(csrc/train_fold.hip: the fold and its adjoint, include/srcnn_hip.h), with the same bits in both directions;
TrainWeights.prepare(device_fold=True) uses it.
"""
import collections
import weakref

import torch

from . import _lib, engine


class Precision(collections.namedtuple('Precision', 'forward backward reuse_maxima')):
    """The public functions' three precision keywords as one immutable value, validated here and nowhere else (forward first)."""
    __slots__ = ()

    def __new__(cls, forward='f32', backward='f32', reuse_maxima=True):
        for name, value in (('forward', forward), ('backward', backward)):
            if value not in ('f32', 'f16x3', 'auto'):
                raise ValueError("%s_precision must be 'f32' or 'f16x3' (got %r), or 'auto' for choose_engine's pick per layer" % (name, value))
        return super().__new__(cls, forward, backward, bool(reuse_maxima))

    def without_graph(self):
        return self._replace(forward='f32')         # layers without a graph (the frozen stages) stay on the fp32 forward

    def resolved(self, M, N, K):
        """'auto' replaced by choose_engine's answer for one call's GEMM, each direction on its own; an explicit engine stays."""
        if 'auto' not in (self.forward, self.backward):
            return self
        return self._replace(forward=choose_engine('forward', M, N, K) if self.forward == 'auto' else self.forward,
                             backward=choose_engine('backward', M, N, K) if self.backward == 'auto' else self.backward)


# choose_engine's thresholds, fitted to profiles/train_engine_table.txt (train_engine_table.ROWS holds its rows; the table times
# the f16x3 calls with maxima handed over and weights prepared, so a layer's f16x3 time carries no preparation).
# tests/test_auto_precision_cpu.py holds the rule to every row outside the +-3 % band.
# Forward: every measured layer of 4750 rows and more wins (0.41 .. 0.94, one at 1.02) and every layer of 1197 rows and fewer
# loses (1.05 .. 2.03): below a few thousand rows the call streams its weights once whatever the engine, and the split adds work.
AUTO_FORWARD_MIN_M = 2400
# Backward: it wins wherever M is small or moderate (0.43 .. 0.97 up to 4750 rows: the weight gradient's long K = M is where the
# f16 pipe pays), and at large M only where a pixel carries enough products: the mask pass, the staged gradient and the split of
# both wgrad operands cost per pixel, the gain grows with N K per pixel.  Measured at M >= 18675: N K <= 65536 loses (1.06 .. 1.24),
# N K >= 131072 wins (0.61 .. 0.81).  M N K >= AUTO_BACKWARD_MIN_NK * M states N K >= 98304 in the rule's own terms.
AUTO_BACKWARD_MIN_M = 64
AUTO_BACKWARD_LARGE_M = 8192
AUTO_BACKWARD_MIN_NK = 98304


def choose_engine(direction, M, N, K):
    """The engine 'auto' stands for in one convolution call: 'f16x3' or 'f32'.  direction: 'forward' (y) or 'backward' (dx, dw,
    db); M = B OH OW output pixels, N = Cout, K = KH KW Cin.  A pure closed-form rule over M and M N K (the thresholds above):
      forward   f16x3 iff M >= AUTO_FORWARD_MIN_M;
      backward  f16x3 iff M >= AUTO_BACKWARD_MIN_M and (M < AUTO_BACKWARD_LARGE_M or M N K >= AUTO_BACKWARD_MIN_NK * M).
    A degenerate M = 1 is fp32 in both directions."""
    if direction not in ('forward', 'backward'):
        raise ValueError("direction must be 'forward' or 'backward' (got %r)" % (direction,))
    M, N, K = int(M), int(N), int(K)
    if direction == 'forward':
        return 'f16x3' if M >= AUTO_FORWARD_MIN_M else 'f32'
    return 'f16x3' if M >= AUTO_BACKWARD_MIN_M and (M < AUTO_BACKWARD_LARGE_M or M * N * K >= AUTO_BACKWARD_MIN_NK * M) else 'f32'


class PreparedLayer(collections.namedtuple('PreparedLayer', 'w b planes')):
    """One layer as stereo_rcnn_amd.training.TrainWeights prepares it: w, the folded weight in the engine's layout (Cout, KH, KW,
    Cin), contiguous and still inside the graph (its gradient flows on to the parameter as it does from the weight a call folds
    itself); b, the folded bias or None; planes, the engine.PreparedW made from w.  A function given `prepared=` uses w and b in
    place of its weight / bias / bn arguments."""
    __slots__ = ()


# The engines of the calls of one forward, in call order: [(M, N, K, forward, backward)], appended to while it is a list
# (record_engines); _REPLAY: an iterator of (forward, backward) that replaces the precisions of the calls one by one (replay_engines).
_DECISIONS = None
_REPLAY = None


class record_engines(object):
    """with record_engines() as log: ... -- log receives (M, N, K, forward engine, backward engine) of every convolution call."""

    def __enter__(self):
        global _DECISIONS
        self.outer, _DECISIONS = _DECISIONS, []
        return _DECISIONS

    def __exit__(self, *exc):
        global _DECISIONS
        _DECISIONS = self.outer


class replay_engines(object):
    """with replay_engines(engines): ... -- the i-th convolution call runs on engines[i] = (forward, backward), both explicit,
    whatever its own precision keywords say: a recorded 'auto' run, forced layer by layer."""

    def __init__(self, engines):
        self.engines = [(f, b) for f, b in engines]

    def __enter__(self):
        global _REPLAY
        self.outer, _REPLAY = _REPLAY, iter(self.engines)

    def __exit__(self, *exc):
        global _REPLAY
        _REPLAY = self.outer


def _bn_scale_shift(bn, eps=1e-5):
    """engine.fold_bn's factors in float64: y = conv(x, w) * scale + shift."""
    s = bn['weight'].detach().double() / torch.sqrt(bn['running_var'].detach().double() + eps)
    return s, bn['bias'].detach().double() - bn['running_mean'].detach().double() * s


# id(tensor) -> (weak reference, _version, word): max |t| over all of t, recorded for that very tensor object at that version.
# Tensor identity survives Function.apply in this torch for both the inputs forward() sees and the output apply() returns
# (tests/test_f16x3_maxima_abi_cpu.py checks it); the record is nevertheless written on what apply() returned.
_MAXIMA = {}


def _record_maximum(t, word):
    key = id(t)
    _MAXIMA[key] = (weakref.ref(t, lambda _, key=key: _MAXIMA.pop(key, None)), t._version, word)


def _known_maximum(t):
    """The recorded word of max |t|, or None: a hit needs the very object the word was recorded for, unmodified since.  A view, a
    slice, a torch.cat result or a tensor changed in place is another object or another version: a miss.  What torch's version
    counter does not see -- a write through `.data`, or an engine call that fills an existing tensor through its raw pointer -- the
    record does not see either: the tensors recorded here are the fresh outputs of this module's functions and their inputs, and a
    caller that rewrites such a tensor behind torch's back passes reuse_maxima=False."""
    hit = _MAXIMA.get(id(t))
    if hit is None or hit[0]() is not t or hit[1] != t._version:
        return None
    return hit[2]


def _conv_nhwc(x, weight, bias, residual, stride, pad, relu, prec, prepared=None):
    """_Conv2dNHWC.apply with the record of maxima around it.  x is contiguous (B, H, W, Cin): the convolution reads the tensor's
    full channel range (Cin = its last dimension = its pixel stride), which is what a recorded word covers.  'auto' is resolved
    here, per call; what follows sees two explicit engines, so a layer resolved to fp32 neither scans nor records a maximum.
    prepared: an engine.PreparedW made from `weight`, or None."""
    cout, kh, kw, cin = (int(v) for v in weight.shape)
    OH, OW = engine.conv_out_hw(int(x.shape[1]), int(x.shape[2]), kh, kw, stride, pad)
    M, K = int(x.shape[0]) * OH * OW, kh * kw * cin
    prec = prec.resolved(M, cout, K)
    if _REPLAY is not None:
        prec = Precision(*next(_REPLAY), reuse_maxima=prec.reuse_maxima).resolved(M, cout, K)
    if _DECISIONS is not None:
        _DECISIONS.append((M, cout, K, prec.forward, prec.backward))
    x_word = y_word = None
    fresh = False
    f16_fwd = prec.forward == 'f16x3'
    f16_dw = prec.backward == 'f16x3' and torch.is_grad_enabled() and weight.requires_grad
    if prec.reuse_maxima and x.is_cuda and (f16_fwd or f16_dw):
        x_word = _known_maximum(x)
        if x_word is None:
            x_word = engine.absmax(x.detach())
            _record_maximum(x, x_word)
            fresh = True
        if f16_fwd:
            y_word = torch.empty(1, dtype=torch.int32, device=x.device)
    y = _Conv2dNHWC.apply(x, weight, bias, residual, stride, pad, relu, prec, x_word, y_word, fresh, prepared)
    if y_word is not None:
        _record_maximum(y, y_word)
    return y


class _Conv2dNHWC(torch.autograd.Function):
    """x (B, H, W, Cin), weight (Cout, KH, KW, Cin) engine layout and already BN-folded, bias (Cout) or None, residual
    (B, OH, OW, Cout) or None; all contiguous float32 on the device."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, stride, pad, relu, prec=Precision(), x_word=None, y_word=None, x_word_fresh=False,
                prepared=None):
        """prec: a Precision without 'auto'; x_word: the word of max |x| or None; y_word: a word to receive max |y| (f16x3 forward)
        or None; x_word_fresh: x_word was scanned for this call, so its first use is not a scan avoided; prepared: the
        engine.PreparedW of `weight` or None -- the f16x3 calls of either direction then skip their own pass over the weights, a
        layer on the fp32 engine ignores it."""
        ctx.backward_precision = prec.backward
        ctx.prepared = prepared
        B, H, W, cin = (int(v) for v in x.shape)
        cout, kh, kw = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        cw = engine.ConvW(weight.detach(), None if bias is None else bias.detach(), kh, kw, stride, pad, relu)
        OH, OW = engine.conv_out_hw(H, W, kh, kw, stride, pad)
        y = torch.empty((B, OH, OW, cout), dtype=torch.float32, device=x.device)
        res = None if residual is None else residual.detach()
        if prec.forward == 'f16x3':
            engine.conv2d_train_f16x3(cw, x.detach(), B, H, W, y, OH, OW, residual=res, x_amax=x_word, y_amax=y_word, prepared=prepared)
            if x_word is not None:
                engine.F16X3_MAXIMA['reused'] += 0 if x_word_fresh else 1
                x_word_fresh = False
        else:
            engine.conv2d(cw, x.detach(), B, H, W, y, OH, OW, residual=res, precision='f32', plan=(0, 0, 0, 0, 0))
        ctx.save_for_backward(x, weight, y if relu else None)
        ctx.x_word, ctx.x_word_fresh = x_word, x_word_fresh
        ctx.geom = (B, H, W, OH, OW, kh, kw, stride, pad, bool(relu), bias is not None, residual is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        B, H, W, OH, OW, kh, kw, stride, pad, relu, has_bias, has_res = ctx.geom
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        need_b, need_r = need_b and has_bias, need_r and has_res
        dy = dy.contiguous()
        want = tuple(k for k, n in (('dx', need_x), ('dw', need_w), ('db', need_b)) if n)
        # the residual branch's gradient is the masked gradient itself; without a ReLU that is dy
        g_out = torch.empty_like(dy) if (need_r and relu) else None
        res = {}
        if want or g_out is not None:
            cw = engine.ConvW(weight, None, kh, kw, stride, pad, relu)
            f16 = ctx.backward_precision == 'f16x3'
            x_word = ctx.x_word if f16 else None
            res = engine.conv2d_backward(cw, x, B, H, W, y, dy, OH, OW, want=want, g_out=g_out, precision=ctx.backward_precision,
                                         x_amax=x_word, prepared=ctx.prepared if f16 else None)
            if x_word is not None and need_w and not ctx.x_word_fresh:
                engine.F16X3_MAXIMA['reused'] += 1
        return (res.get('dx'), res.get('dw'), res.get('db'), (g_out if relu else dy) if need_r else None) + (None,) * 8


def _check(x, weight):
    if not (x.is_cuda and weight.is_cuda):
        raise NotImplementedError
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TypeError("float32 tensors only")


class _ToNHWC(torch.autograd.Function):
    """(B, C, H, W) -> (B, H, W, C) through the library's layout kernels, both directions."""

    @staticmethod
    def forward(ctx, x):
        return engine.nchw_to_nhwc(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return engine.nhwc_to_nchw(g.contiguous())


class _ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return engine.nhwc_to_nchw(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return engine.nchw_to_nhwc(g.contiguous())


def _fold(weight_eng, bias, bn):
    """Frozen BatchNorm (the reference's set_bn_fix freezes every BN: it gets no gradient) folded as engine.fold_bn folds it --
    in float64, stored float32 -- but inside the graph: d(w * scale) / dw = scale, so the gradient with respect to the UNFOLDED
    weight is dw_folded * scale[n], and a conv bias under a BN receives db * scale[n]."""
    if bn is None:
        return weight_eng, bias
    scale, shift = _bn_scale_shift(bn)
    w = (weight_eng.double() * scale.view(-1, 1, 1, 1)).float()
    b = shift.float() if bias is None else (bias.double() * scale + shift).float()
    return w, b


def _folded(prepared, fold):
    """(w, b, planes) of a public function's layer: the PreparedLayer's, or fold()'s own w (made contiguous) and b without planes."""
    if prepared is not None:
        return prepared.w, prepared.b, prepared.planes
    w, b = fold()
    return w.contiguous(), b, None


def fold_conv(weight, bias=None, bn=None):
    """conv2d's / conv2d_nhwc's folded weight and bias: weight (Cout, Cin, KH, KW) -> (Cout, KH, KW, Cin) with the frozen BN in."""
    return _fold(weight.permute(0, 2, 3, 1), bias, bn)


def fold_linear(weight, bias=None):
    """linear's: weight (out, K) -> (out, 1, 1, K)."""
    return weight.contiguous().view(int(weight.shape[0]), 1, 1, int(weight.shape[1])), bias


def fold_deconv2x2(weight, bias=None):
    """conv_transpose2x2's: weight (Cin, Cout, 2, 2) -> (4 Cout, 1, 1, Cin) in row order (i, j, co), the bias four times."""
    cin, cout = int(weight.shape[0]), int(weight.shape[1])
    return weight.permute(2, 3, 1, 0).reshape(4 * cout, 1, 1, cin), None if bias is None else bias.repeat(4)


def fold_spec(spec):
    """One engine.FoldSpec folded by the eager operators above: its parts' weights (and biases) concatenated along the rows, then
    fold_conv / fold_linear / fold_deconv2x2 by its kind.  Returns (w, b or None), w in the folded shape spec.shape (a view
    wherever the fold is one), both inside the graph.  fold_all is the same for a whole list on the device."""
    ws, bs = [w for w, _ in spec.parts], [b for _, b in spec.parts]
    w = ws[0] if len(ws) == 1 else torch.cat(ws, 0)
    b = None if bs[0] is None else bs[0] if len(bs) == 1 else torch.cat(bs, 0)
    if spec.kind == 'conv':
        return fold_conv(w, b, spec.bn)
    return fold_linear(w, b) if spec.kind == 'linear' else fold_deconv2x2(w, b)


class _FoldAll(torch.autograd.Function):
    """fold_all's node: inputs, per layer and part, the weight and (where there is one) the bias, then every frozen BN tensor;
    outputs, per layer, the folded w and (where there is one) the folded b.  A b that is a BN's shift alone depends on no
    parameter: it is marked non-differentiable."""

    @staticmethod
    def forward(ctx, specs, *tensors):
        ctx.set_materialize_grads(False)
        ctx.specs, ctx.n_inputs = specs, len(tensors)
        flat, constant = [], []
        for s, (w, b) in zip(specs, engine.fold_train_weights(specs)):
            flat.append(w)
            if b is not None:
                flat.append(b)
                if s.parts[0][1] is None:
                    constant.append(b)
        ctx.mark_non_differentiable(*constant)
        return tuple(flat)

    @staticmethod
    def backward(ctx, *grads):
        grads = iter(grads)
        dws, dbs = [], []
        for s in ctx.specs:
            dw, db = next(grads), next(grads) if s.has_b else None
            dws.append(None if dw is None else dw.contiguous())
            dbs.append(None if db is None or s.parts[0][1] is None else db.contiguous())
        out = [None]                                            # specs
        if any(g is not None for g in dws + dbs):
            for s, (gws, gbs) in zip(ctx.specs, engine.fold_train_weights_backward(ctx.specs, dws, dbs)):
                for (_, b), gw, gb in zip(s.parts, gws, gbs):
                    out += [gw] if b is None else [gw, gb]
        return tuple(out) + (None,) * (1 + ctx.n_inputs - len(out))        # no gradient at all / the frozen BN tensors


def fold_all(specs):
    """fold_conv / fold_linear / fold_deconv2x2 + .contiguous() of a whole list of layers as ONE graph node over two library calls
    (engine.fold_train_weights forward, engine.fold_train_weights_backward for all gradients at once; csrc/train_fold.hip).
    specs: engine.FoldSpec's over the PARAMETERS.  Returns [(w, b or None)] per layer: contiguous, in the engine's layout, inside
    the graph, with the bits of the eager folds; so are the gradients that reach the parameters.  A parameter none of whose
    folded tensors received a gradient gets None; the frozen BN tensors get None.  The one operator left to torch is a
    deconvolution's bias: b = bias.repeat(4), whose adjoint is a four-term float sum in an order torch does not document."""
    specs = list(specs)
    inner, tensors, bns = [], [], []
    for s in specs:
        deconv_bias = s.kind == 'deconv2x2' and s.parts[0][1] is not None
        inner.append(engine.FoldSpec(s.kind, [(s.parts[0][0], None)]) if deconv_bias else s)
        for w, b in inner[-1].parts:
            tensors += [w] if b is None else [w, b]
        bns += [] if s.bn is None else [s.bn[k] for k in ('weight', 'bias', 'running_mean', 'running_var')]
    flat = iter(_FoldAll.apply(inner, *(tensors + bns)))
    out = []
    for s, i in zip(specs, inner):
        w = next(flat)
        b = next(flat) if i.has_b else (s.parts[0][1].repeat(4) if s.has_b else None)
        out.append((w, b))
    return out


def conv2d(x, weight, bias=None, stride=1, padding=0, relu=False, residual=None, bn=None, backward_precision='f32', forward_precision='f32',
           reuse_maxima=True, prepared=None):
    """relu?(bn?(conv2d(x, weight) + bias) + residual) on the exact-fp32 engine, differentiable with respect to x, weight, bias
    and residual.  x (B, Cin, H, W) with Cin a multiple of 32, weight (Cout, Cin, KH, KW) as nn.Conv2d holds it, residual
    (B, Cout, OH, OW); bn: a dict with 'weight', 'bias', 'running_mean', 'running_var' -- the frozen BatchNorm that follows the
    convolution (no gradient reaches it).  backward_precision: 'f32' or 'f16x3', the engine of the gradients; forward_precision:
    'f32' or 'f16x3', the engine of y (independent of it; anything else raises ValueError); either may be 'auto': choose_engine
    decides per call.  reuse_maxima: see the module's docstring.  prepared: a PreparedLayer of this layer (fold_conv of the same
    weight, bias and bn, then engine.prepare_train_weights): its w and b are used, and the f16x3 calls skip their passes over the
    weight.  Returns (B, Cout, OH, OW)."""
    prec = Precision(forward_precision, backward_precision, reuse_maxima)
    _check(x, weight)
    if int(x.shape[1]) % 32 != 0:
        raise ValueError("Cin must be a multiple of 32 (got %d)" % int(x.shape[1]))
    w, b, planes = _folded(prepared, lambda: fold_conv(weight, bias, bn))
    r = None if residual is None else _ToNHWC.apply(residual)
    y = _conv_nhwc(_ToNHWC.apply(x), w, b, r, int(stride), int(padding), bool(relu), prec, planes)
    return _ToNCHW.apply(y)


def linear(x, weight, bias=None, relu=False, backward_precision='f32', forward_precision='f32', reuse_maxima=True, _prec=None,
           prepared=None):
    """relu?(x @ weight.T + bias) as a 1x1 convolution over an (n, 1, 1, K) tensor: x (n, K), weight (out, K) as nn.Linear holds
    it.  K must be a multiple of 32.  _prec: conv2d_nhwc's.  prepared: conv2d's, from fold_linear."""
    prec = _prec or Precision(forward_precision, backward_precision, reuse_maxima)
    _check(x, weight)
    n, K = int(x.shape[0]), int(x.shape[1])
    if K % 32 != 0:
        raise ValueError("linear: K must be a multiple of 32 (got %d)" % K)
    out = int(weight.shape[0])
    w, b, planes = _folded(prepared, lambda: fold_linear(weight, bias))
    y = _conv_nhwc(x.contiguous().view(n, 1, 1, K), w, b, None, 1, 0, bool(relu), prec, planes)
    return y.view(n, out)


def conv2d_nhwc(x, weight, bias=None, stride=1, padding=0, relu=False, residual=None, bn=None, backward_precision='f32', forward_precision='f32',
                reuse_maxima=True, _prec=None, prepared=None):
    """conv2d without the layout edges: x (B, H, W, Cin), residual and the result (B, OH, OW, Cout) NHWC; weight still
    (Cout, Cin, KH, KW) as nn.Conv2d holds it (its re-layout is one small kernel and carries the gradient back).  _prec (private,
    stereo_rcnn_amd.training's): an already validated Precision, used in place of the three keywords.  prepared: conv2d's."""
    prec = _prec or Precision(forward_precision, backward_precision, reuse_maxima)
    _check(x, weight)
    if int(x.shape[3]) % 32 != 0:
        raise ValueError("Cin must be a multiple of 32 (got %d)" % int(x.shape[3]))
    w, b, planes = _folded(prepared, lambda: fold_conv(weight, bias, bn))
    return _conv_nhwc(x.contiguous(), w, b, None if residual is None else residual.contiguous(),
                      int(stride), int(padding), bool(relu), prec, planes)


def _check_nhwc(x, what):
    if not x.is_cuda:
        raise NotImplementedError
    if x.dtype != torch.float32:
        raise TypeError("float32 tensors only")
    if x.dim() != 4 or int(x.shape[3]) % 8 != 0:
        raise ValueError("%s: (B, H, W, C) with C a multiple of 8 (got %s)" % (what, tuple(x.shape)))


class _UpsampleAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, top, lateral):
        B, H, W, C = (int(v) for v in lateral.shape)
        TH, TW = int(top.shape[1]), int(top.shape[2])
        y = torch.empty_like(lateral)
        engine.upsample_add(top, TH, TW, lateral, B, H, W, C, y)
        ctx.geom = (B, H, W, C, TH, TW)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, C, TH, TW = ctx.geom
        dy = dy.contiguous()
        d_top = None
        if ctx.needs_input_grad[0]:
            d_top = torch.empty((B, TH, TW, C), dtype=torch.float32, device=dy.device)
            _lib.check(_lib.lib().srcnn_upsample_add_backward(dy.data_ptr(), B, H, W, C, d_top.data_ptr(), TH, TW, _lib.stream()),
                       "srcnn_upsample_add_backward")
        return d_top, (dy if ctx.needs_input_grad[1] else None)        # the lateral's gradient is dy itself


def upsample_add(top, lateral):
    """bilinear(top -> lateral's size, align_corners=True) + lateral (stereo_rcnn.py:91-108): top (B, TH, TW, C), lateral
    (B, H, W, C) with H >= TH, W >= TW; NHWC, differentiable with respect to both."""
    _check_nhwc(top, "upsample_add"), _check_nhwc(lateral, "upsample_add")
    if top.shape[0] != lateral.shape[0] or top.shape[3] != lateral.shape[3] or top.shape[1] > lateral.shape[1] \
            or top.shape[2] > lateral.shape[2]:
        raise ValueError("upsample_add: top %s does not go with lateral %s" % (tuple(top.shape), tuple(lateral.shape)))
    return _UpsampleAdd.apply(top.contiguous(), lateral.contiguous())


class _Subsample2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, H, W, C = (int(v) for v in x.shape)
        OH, OW = (H + 1) // 2, (W + 1) // 2
        y = torch.empty((B, OH, OW, C), dtype=torch.float32, device=x.device)
        engine.subsample2(x, B, H, W, C, y, OH, OW)
        ctx.geom = (B, H, W, C, OH, OW)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, C, OH, OW = ctx.geom
        dy = dy.contiguous()
        dx = torch.empty((B, H, W, C), dtype=torch.float32, device=dy.device)
        _lib.check(_lib.lib().srcnn_subsample2_backward(dy.data_ptr(), B, OH, OW, C, dx.data_ptr(), H, W, _lib.stream()),
                   "srcnn_subsample2_backward")
        return dx


def subsample2(x):
    """MaxPool2d(1, stride=2) (stereo_rcnn.py:39,168): y[b, i, j, :] = x[b, 2i, 2j, :], NHWC, differentiable."""
    _check_nhwc(x, "subsample2")
    return _Subsample2.apply(x.contiguous())


def pixel_shuffle2(x, cq, inverse=False):
    """srcnn_pixel_shuffle2: packed (M, h, w, 4 cq) ordered (i, j, co) -> (M, 2h, 2w, cq), or back with inverse: (M, 2h, 2w, cq)
    -> (M, h, w, 4 cq).  float32 device tensors, cq a multiple of 8; a shape that is not one of the two raises ValueError."""
    _check_nhwc(x, "pixel_shuffle2")
    cq = int(cq)
    M, H, W, C = (int(v) for v in x.shape)
    if cq <= 0 or cq % 8 != 0:
        raise ValueError("pixel_shuffle2: cq must be a positive multiple of 8 (got %d)" % cq)
    if inverse:
        if C != cq or H % 2 != 0 or W % 2 != 0:
            raise ValueError("pixel_shuffle2 inverse: (M, 2h, 2w, %d) expected (got %s)" % (cq, tuple(x.shape)))
        h, w = H // 2, W // 2
    else:
        if C != 4 * cq:
            raise ValueError("pixel_shuffle2: (M, h, w, %d) expected (got %s)" % (4 * cq, tuple(x.shape)))
        h, w = H, W
    x = x.contiguous()
    y = torch.empty((M, h, w, 4 * cq) if inverse else (M, 2 * h, 2 * w, cq), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().srcnn_pixel_shuffle2(x.data_ptr(), M, h, w, cq, y.data_ptr(), int(bool(inverse)), _lib.stream()),
               "srcnn_pixel_shuffle2")
    return y


class _PixelShuffle2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cq):
        ctx.cq = cq
        return pixel_shuffle2(x, cq)

    @staticmethod
    def backward(ctx, dy):
        return pixel_shuffle2(dy.contiguous(), ctx.cq, inverse=True), None


def conv_transpose2x2(x, weight, bias=None, relu=False, backward_precision='f32', forward_precision='f32', reuse_maxima=True, _prec=None,
                      prepared=None):
    """relu?(ConvTranspose2d(k=2, s=2)(x)): x (M, h, w, Cin) NHWC with Cin a multiple of 32, weight (Cin, Cout, 2, 2) as
    nn.ConvTranspose2d holds it, Cout a multiple of 8; returns (M, 2h, 2w, Cout).  A 1x1 convolution to 4 Cout channels in
    engine.prep_deconv2x2's row order (i, j, co) with the bias replicated four times, then the pixel shuffle; the ReLU commutes
    with the shuffle and stays in the convolution's epilogue.  Backward: the inverse shuffle of dy, then the convolution's
    backward; torch's autograd takes dw back to (Cin, Cout, 2, 2) and sums db over the four (i, j) groups.  _prec: conv2d_nhwc's.  prepared: conv2d's, from fold_deconv2x2."""
    prec = _prec or Precision(forward_precision, backward_precision, reuse_maxima)
    _check(x, weight)
    cin, cout = int(weight.shape[0]), int(weight.shape[1])
    if tuple(weight.shape[2:]) != (2, 2) or int(x.shape[3]) != cin:
        raise ValueError("conv_transpose2x2: weight (Cin, Cout, 2, 2) with x's Cin (got %s)" % (tuple(weight.shape),))
    if cin % 32 != 0 or cout % 8 != 0:
        raise ValueError("conv_transpose2x2: Cin a multiple of 32 and Cout a multiple of 8 (got %d, %d)" % (cin, cout))
    w, b, planes = _folded(prepared, lambda: fold_deconv2x2(weight, bias))
    y = _conv_nhwc(x.contiguous(), w, b, None, 1, 0, bool(relu), prec, planes)
    out = _PixelShuffle2.apply(y, cout)
    word = _known_maximum(y)
    if word is not None:
        _record_maximum(out, word)          # the shuffle moves every element and changes none: the same maximum
    return out
