"""GPU: srcnn_train_weights_fold / srcnn_train_weights_fold_backward (csrc/train_fold.hip, include/srcnn_hip.h) and
autograd.fold_all over them, against the eager folds they replace -- autograd.fold_conv / fold_linear / fold_deconv2x2 +
.contiguous() (torch.cat for several parts) and torch autograd through them -- on the same device.  Every comparison is on int32
bit views.  ONE list crosses the table search, the unit edges (rows and channels that do not fill a unit, several channel chunks
per row, several rows per unit) and the argument-block edge (one layer more than a block)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
ABSENT = (3, 5)             # the layers whose folded tensors receive no gradient
FROZEN = 9                  # the layer whose weight does not require a gradient


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


class Case(object):
    """The list: per layer the engine.FoldSpec over its parameters and `eager`, a function returning the parent path's (w, b)."""

    def __init__(self, dev):
        from stereo_rcnn_amd import autograd as A, engine
        g = torch.Generator(device=dev).manual_seed(5)
        rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)
        par = lambda *shape: rnd(*shape).requires_grad_(True)

        def bn(n):
            d = {'weight': rnd(n) + 1.0, 'bias': rnd(n), 'running_mean': rnd(n), 'running_var': torch.rand(n, device=dev, generator=g) + 0.1}
            d['weight'][0] = 0.0                                    # gamma 0
            d['running_var'][0] = 1e-12
            if n > 2:
                d['weight'][1] = -1.5                               # negative gamma
                d['running_var'][2] = 0.0
                d['running_var'][n - 1] = 1e-12
            d['weight'].requires_grad_(True), d['bias'].requires_grad_(True)          # frozen all the same: they must receive nothing
            return d

        S = engine.FoldSpec
        self.layers = []

        def conv(cout, cin, k, with_bn, bias, view=False):
            w, b, n = par(cout, cin, k, k), par(cout) if bias else None, bn(cout) if with_bn else None
            if view:                                                # RCNN_top.0's form: the window as one row of a linear layer
                eager = lambda: A.fold_linear(w.permute(0, 2, 3, 1).reshape(cout, -1), b)
            else:
                eager = lambda: A.fold_conv(w, b, n)
            self.layers.append((S('conv', [(w, b)], n), eager, view))

        conv(5, 32, 3, True, False)
        conv(33, 64, 1, True, False)
        conv(3, 32, 7, False, True, view=True)
        conv(40, 96, 3, False, True)
        ws, bs = [par(6, 64, 1, 1), par(18, 64, 1, 1)], [par(6), par(18)]
        self.layers.append((S('conv', list(zip(ws, bs))), lambda ws=ws, bs=bs: A.fold_conv(torch.cat(ws, 0), torch.cat(bs, 0)), False))
        wl, bl = [par(12, 96), par(10, 96), par(2, 96)], [par(12), par(10), par(2)]
        self.layers.append((S('linear', list(zip(wl, bl))), lambda: A.fold_linear(torch.cat(wl, 0), torch.cat(bl, 0)), False))
        w7 = par(7, 32)
        self.layers.append((S('linear', [(w7, None)]), lambda: A.fold_linear(w7, None), False))
        wd, bd = par(32, 8, 2, 2), par(8)
        self.layers.append((S('deconv2x2', [(wd, bd)]), lambda: A.fold_deconv2x2(wd, bd), False))
        i = 0
        while len(self.layers) < engine._lib.TRAIN_FOLD_LAYERS_PER_BLOCK + 1:
            # 1x1 fillers, Cout 1..4: BN without a bias, BN with a bias, a bias alone, nothing
            conv(1 + i % 4, 32, 1, i % 4 < 2, i % 4 in (1, 2))
            i += 1
        self.layers[FROZEN][0].parts[0][0].requires_grad_(False)
        self.specs = [s for s, _, _ in self.layers]
        self.params = [t for s in self.specs for w, b in s.parts for t in (w, b) if t is not None]
        self.bn_tensors = [t for s in self.specs if s.bn is not None for t in s.bn.values()]

    def eager(self):
        out = []
        for _, fold, _ in self.layers:
            w, b = fold()
            out.append((w.contiguous(), b))
        return out

    def device(self):
        from stereo_rcnn_amd import autograd as A
        return [(w.view(int(w.shape[0]), 1, 1, -1) if view else w, b) for (w, b), (_, _, view) in zip(A.fold_all(self.specs), self.layers)]


@pytest.fixture(scope='module')
def case(dev):
    import __graft_entry__ as ge
    ge.build()
    c = Case(dev)
    assert len(c.specs) == 25 and {s.kind for s in c.specs} == {'conv', 'linear', 'deconv2x2'}
    c.reference = [(w.detach().clone(), None if b is None else b.detach().clone()) for w, b in c.eager()]        # computed once
    return c


class Raw(object):
    """The forward entry on caller-supplied destinations: one buffer of NaN, each destination followed by GUARD floats."""

    def __init__(self, case, dev):
        from stereo_rcnn_amd import _lib, engine
        self.lib, self._lib = _lib.lib(), _lib
        specs, self.descs = engine._fold_descs(case.specs)
        self.n = len(specs)
        self.spans, off = [], 0
        for s in specs:
            span = []
            for numel in (s.shape[0] * s.shape[1] * s.shape[2] * s.shape[3], s.shape[0] if s.has_b else 0):
                span.append((off, numel))
                off = -(-(off + numel + GUARD) // 4) * 4 if numel else off
            self.spans.append(span)
        self.buf = torch.full((off,), float('nan'), dtype=torch.float32, device=dev)
        for d, ((wo, _), (bo, bn)) in zip(self.descs, self.spans):
            d.dst_w, d.dst_b = self.buf.data_ptr() + 4 * wo, self.buf.data_ptr() + 4 * bo if bn else None
        self.ws = torch.empty(self.lib.srcnn_train_fold_workspace_bytes(self.n), dtype=torch.uint8, device=dev)

    def run(self):
        self._lib.check(self.lib.srcnn_train_weights_fold(self.descs, self.n, self.ws.data_ptr(), self.ws.numel(), self._lib.stream()),
                        "srcnn_train_weights_fold")

    def outputs(self):
        return [tuple(self.buf[o:o + n] if n else None for o, n in span) for span in self.spans]


def test_forward_bits_and_guards(case, dev):
    raw = Raw(case, dev)
    raw.run()
    written = torch.zeros(raw.buf.numel(), dtype=torch.bool, device=dev)
    for i, ((w, b), (rw, rb)) in enumerate(zip(raw.outputs(), case.reference)):
        assert torch.equal(_bits(w), _bits(rw).view(-1)), i
        assert (b is None) == (rb is None), i
        if b is not None:
            assert torch.equal(_bits(b), _bits(rb)), i
    for span in raw.spans:
        for o, n in span:
            written[o:o + n] = True
    assert bool(torch.isnan(raw.buf[~written]).all()), "a guard zone was written"
    assert int((~written).sum()) >= GUARD * (len(case.specs) + 1)
    first = raw.buf.clone()
    raw.buf.fill_(float('nan'))
    raw.run()
    assert torch.equal(_bits(first), _bits(raw.buf))            # two runs, equal bits


def test_fold_all_forward_carries_the_graph(case):
    for i, ((w, b), (rw, rb), (ew, eb)) in enumerate(zip(case.device(), case.reference, case.eager())):
        assert w.shape == rw.shape and w.is_contiguous() and torch.equal(_bits(w), _bits(rw)), i
        assert (b is None) == (rb is None), i
        if b is not None:
            assert torch.equal(_bits(b), _bits(rb)), i
            assert b.requires_grad == eb.requires_grad, i        # a BN's shift alone depends on no parameter
        assert w.requires_grad


def _gradients(case, folded, grads):
    for t in case.params + case.bn_tensors:
        t.grad = None
    outs, gs = [], []
    for i, ((w, b), (gw, gb)) in enumerate(zip(folded, grads)):
        if i in ABSENT:
            continue
        if w.requires_grad:
            outs.append(w), gs.append(gw)
        if b is not None and b.requires_grad:
            outs.append(b), gs.append(gb)
    torch.autograd.backward(outs, gs)
    return [None if t.grad is None else t.grad for t in case.params], [t.grad for t in case.bn_tensors]


def test_backward_bits(case, dev):
    g = torch.Generator(device=dev).manual_seed(9)

    def spread(shape):                                             # magnitudes over 1e-8 .. 1e3, both signs
        mag = 10.0 ** (torch.rand(shape, device=dev, generator=g) * 11.0 - 8.0)
        return mag * (torch.randint(0, 2, shape, device=dev, generator=g).float() * 2.0 - 1.0)

    grads = [(spread(tuple(w.shape)), None if b is None else spread(tuple(b.shape))) for w, b in case.reference]
    want, want_bn = _gradients(case, case.eager(), grads)
    got, got_bn = _gradients(case, case.device(), grads)
    again, _ = _gradients(case, case.device(), grads)
    absent = {id(t) for i in ABSENT for w, b in case.specs[i].parts for t in (w, b)}
    frozen = id(case.specs[FROZEN].parts[0][0])
    assert all(t is None for t in want_bn + got_bn)
    some = 0
    for p, a, b, c in zip(case.params, want, got, again):
        if id(p) in absent or id(p) == frozen:
            assert a is None and b is None
            continue
        assert a is not None and b is not None, tuple(p.shape)
        assert b.shape == p.shape and b.is_contiguous()
        assert torch.equal(_bits(a), _bits(b)), tuple(p.shape)
        assert torch.equal(_bits(b), _bits(c)), tuple(p.shape)  # two runs, equal bits
        some += 1
    assert some == len(case.params) - len(absent) - 1


def test_capturable_in_a_graph(case, dev):
    raw = Raw(case, dev)
    raw.run()
    direct = raw.buf.clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        raw.run()                                                   # warm-up on the capture's side of the allocator
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # one stream, no parallel branches
        raw.run()
    raw.buf.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(raw.buf), _bits(direct))
