"""Float64 restatement of the three adjoints of csrc/train_ops.hip (include/srcnn_hip.h, "training: remaining adjoints"), NHWC.

The bilinear taps use the forward's own float32 index and weight expressions (upsample_add_kernel), so the reference sums
exactly the terms the device sums and differs from it by the float32 accumulation alone; tests/test_train_ops_ref_cpu.py checks
the restatement itself against torch.autograd of F.interpolate, strided slicing and F.conv_transpose2d.
"""
import numpy as np
import torch

U = 2.0 ** -24          # float32 unit roundoff


def up_taps(n_out, n_top):
    """Per output index: (i1, i1 + i1p, l0, l1), float32 arithmetic as the forward kernel's."""
    r = np.float32(n_top - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    f = (r * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i1 = f.astype(np.int32)
    i1p = (i1 < n_top - 1).astype(np.int32)
    l1 = (f - i1.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i1, i1 + i1p, l0, l1


def up_candidates(n_out, n_top, t):
    """The gather kernel's candidate range [lo, hi] of output indices for top index t (csrc/train_ops.hip, up_candidates),
    float32 operation by operation: indices with i1 in {t - 1, t} lie in [(t - 1) / r, (t + 1) / r), one index of slack on each
    side, clipped to the axis; r == 0: the whole axis."""
    f = np.float32
    r = f(n_top - 1) / f(n_out - 1) if n_out > 1 else f(0)
    if r == 0:
        return 0, n_out - 1
    a = f(np.floor(f(f(t - 1) / r))) - f(1)
    b = f(np.ceil(f(f(t + 1) / r))) + f(1)
    return (0 if a < 0 else int(a)), (n_out - 1 if b > f(n_out - 1) else int(b))


def up_gather_matrix(n_out, n_top):
    """up_matrix rebuilt the way the kernel gathers: per top index, only the candidates of up_candidates, each accepted after
    its taps have been recomputed the forward's way.  Equal to up_matrix exactly when the candidate range loses no term (and no
    term can be doubled: each (output index, tap) pair is visited for one top index only)."""
    i1, i2, l0, l1 = up_taps(n_out, n_top)
    A = np.zeros((n_out, n_top))
    for t in range(n_top):
        lo, hi = up_candidates(n_out, n_top, t)
        for o in range(lo, hi + 1):
            if i1[o] == t:
                A[o, t] += float(l0[o])
            if i2[o] == t:
                A[o, t] += float(l1[o])
    return torch.from_numpy(A)


def up_matrix(n_out, n_top):
    """(n_out, n_top) float64 interpolation matrix of one axis: row o holds l0 at i1 and l1 at i1 + i1p (added where both
    are the same top index)."""
    i1, i2, l0, l1 = up_taps(n_out, n_top)
    A = np.zeros((n_out, n_top))
    for o in range(n_out):
        A[o, i1[o]] += float(l0[o])
        A[o, i2[o]] += float(l1[o])
    return torch.from_numpy(A)


def upsample(top, H, W):
    """(B, TH, TW, C) -> (B, H, W, C) float64: the forward without the lateral."""
    Ah, Aw = up_matrix(H, int(top.shape[1])), up_matrix(W, int(top.shape[2]))
    return torch.einsum('ht,btsc,ws->bhwc', Ah, top.double(), Aw)


def upsample_add_backward(dy, TH, TW):
    """d_top (B, TH, TW, C) float64 of dy (B, H, W, C), and S: the same sum over |coefficient * dy| (the error scale)."""
    Ah, Aw = up_matrix(int(dy.shape[1]), TH), up_matrix(int(dy.shape[2]), TW)
    g = torch.einsum('ht,bhwc,ws->btsc', Ah, dy.double(), Aw)
    S = torch.einsum('ht,bhwc,ws->btsc', Ah, dy.double().abs(), Aw)
    return g, S


def fmaf32(k, v, acc):
    """round_float32(k * v + acc) with ONE rounding, for float32 arrays: the product of two float32 is exact in float64; the sum
    is taken in float64 with its rounding error (TwoSum) and, where inexact, moved to the neighbour with an odd last bit
    (round to odd), after which the rounding to float32 is the correct single one (53 >= 2 * 24 + 2 bits)."""
    p = np.asarray(k, np.float32).astype(np.float64) * np.asarray(v, np.float32).astype(np.float64)
    a = np.asarray(acc, np.float32).astype(np.float64)
    s = p + a
    t = s - p
    err = (p - (s - t)) + (a - t)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def upsample_add_backward_f32(dy, TH, TW):
    """float32 restatement of srcnn_upsample_add_backward in its DEFINED SUMMATION ORDER (include/srcnn_hip.h): per top pixel,
    ascending h, inside a row ascending w, inside an output pixel the taps (l0h, l0w) (l0h, l1w) (l1h, l0w) (l1h, l1w); one
    chain acc = fmaf(k, dy, acc) from 0 with k = lh * lw rounded to float32 once.  The taps and weights are those of
    small_kernels_ref.upsample_add_f32 (the forward's restatement).  dy (B, H, W, C) float32 numpy -> (B, TH, TW, C) float32."""
    from small_kernels_ref import _taps
    dy = np.asarray(dy, np.float32)
    B, H, W, C = dy.shape
    f = lambda a: a.astype(np.float32)
    h0, h1, a0, a1 = _taps(TH, H)
    w0, w1, b0, b1 = _taps(TW, W)
    rows, cols = ((h0, f(a0)), (h1, f(a1))), ((w0, f(b0)), (w1, f(b1)))
    out = np.zeros((B, TH, TW, C), np.float32)
    for th in range(TH):
        for tw in range(TW):
            acc = np.zeros((B, C), np.float32)
            for h in range(H):
                for w in range(W):
                    for ih, lh in rows:
                        for iw, lw in cols:
                            if ih[h] == th and iw[w] == tw:
                                acc = fmaf32(lh[h] * lw[w], dy[:, h, w, :], acc)
            out[:, th, tw, :] = acc
    return out


def subsample2(x):
    return x[:, ::2, ::2, :]


def subsample2_backward(dy, H, W):
    dx = torch.zeros((dy.shape[0], H, W, dy.shape[3]), dtype=dy.dtype)
    dx[:, ::2, ::2, :] = dy
    return dx


def pixel_shuffle2(packed, cq):
    """(M, h, w, 4 cq) ordered (i, j, co) -> (M, 2h, 2w, cq)."""
    M, h, w, _ = packed.shape
    return packed.reshape(M, h, w, 2, 2, cq).permute(0, 1, 3, 2, 4, 5).reshape(M, 2 * h, 2 * w, cq)


def pixel_unshuffle2(wide):
    M, H2, W2, cq = wide.shape
    return wide.reshape(M, H2 // 2, 2, W2 // 2, 2, cq).permute(0, 1, 3, 2, 4, 5).reshape(M, H2 // 2, W2 // 2, 4 * cq)


def conv_transpose2x2(x, weight, bias):
    """x (M, h, w, Cin) NHWC, weight (Cin, Cout, 2, 2), bias (Cout): pre-activation output (M, 2h, 2w, Cout), float64, as the
    product builds it: a matrix product to (i, j, co) columns, then the shuffle."""
    cout = int(weight.shape[1])
    y = torch.einsum('mhwc,cnij->mhwijn', x.double(), weight.double()).reshape(x.shape[0], x.shape[1], x.shape[2], 4 * cout)
    return pixel_shuffle2(y, cout) + bias.double()


def conv_transpose2x2_backward(x, weight, g):
    """Gradients of conv_transpose2x2 for upstream g (M, 2h, 2w, Cout) (already masked by the ReLU): dx, dw (Cin, Cout, 2, 2),
    db, and the absolute-value sums S_dx, S_dw, S_db."""
    cout = int(weight.shape[1])
    gp = pixel_unshuffle2(g.double()).reshape(x.shape[0], x.shape[1], x.shape[2], 2, 2, cout)
    xd, wd = x.double(), weight.double()
    out = {'dx': torch.einsum('mhwijn,cnij->mhwc', gp, wd), 'dw': torch.einsum('mhwc,mhwijn->cnij', xd, gp),
           'db': gp.sum((0, 1, 2, 3, 4)),
           'S_dx': torch.einsum('mhwijn,cnij->mhwc', gp.abs(), wd.abs()),
           'S_dw': torch.einsum('mhwc,mhwijn->cnij', xd.abs(), gp.abs()), 'S_db': gp.abs().sum((0, 1, 2, 3, 4))}
    return out
