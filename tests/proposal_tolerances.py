"""The one float tolerance of the proposal stage tests: how far a float32 evaluation of `decode_one` + clip
(csrc/rpn_proposal.hip; bbox_transform.py:81-104,177-185) may lie from the float64 evaluation of the same float32 inputs.

Everything else the stage tests compare -- selection order, keep lists, counts, gathered scores, RoI rows, padding -- is exact.

Derivation.  The library is built with -ffp-contract=off, so every float32 operation of the kernel rounds once, to nearest:
fl(x) = x (1 + d), |d| <= U = 2^-24.  A result that falls below the smallest normal number may also be flushed to zero, which
costs at most TINY = 2^-126 absolutely.  With a computed value a^ = a + ea (|ea| bounded) the operations of decode_one give

    add / sub   r = a +- b      e(r) = ea + eb + U (|r| + ea + eb)
    mul         r = a b         e(r) = E + U (|r| + E) + TINY,   E = |a| eb + |b| ea + ea eb
    0.5 * a     exact           e(r) = ea / 2
    expf        r = exp(d)      e(r) = EXPF_ULPS * 2 U * r + TINY      (an ulp is at most 2 U relative)

and the sequence is, per eye and axis (inputs a1, a2, d, dl are float32 and therefore exact),

    w   = (a2 - a1) + 1          2 roundings
    c   = a1 + 0.5 w             1 rounding
    pc  = d * w + c              2 roundings
    p   = expf(dl) * w           expf + 1 rounding
    lo  = pc - 0.5 p             1 rounding
    hi  = pc + 0.5 p             1 rounding

followed by the clip to [0, limit], which is monotone and 1-Lipschitz: it never enlarges an error, and a value that lies beyond
the limit by more than its bound comes out as the limit EXACTLY.  That also holds for an infinite p (expf overflows above
dl = 88.72): lo is -inf -> 0, hi is +inf -> limit; the float64 evaluation (finite there) is clipped to the same two numbers.
The limit itself, im_info - 1, is exact for the integer image sizes of the tests (`bound` refuses anything else).

EXPF_ULPS.  No copy of the device library's accuracy table ships with the toolchain, so the constant is a stated conservative
figure: 2 ulps.  The published accuracy of the device library's single-precision exp is 1 ulp; glibc's and torch's CPU expf are
below 1 ulp as well.  tests/test_proposal_ref_cpu.py holds torch's float32 exp to this figure against float64 exp over the
exponents the tests feed, so the CPU path of the derivation is checked; the device is held to the resulting bound as it stands.

The bound is worst case (all roundings aligned), so a correct float32 evaluation typically uses a fraction of it; the CPU test
prints how much the oracle's float32 path uses and asserts it is not vacuous: the planted mistakes of the same file all exceed it
a hundredfold.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
EXPF_ULPS = 2.0
F32_EXP_OVERFLOW = 88.7228394          # log(FLT_MAX): above it expf returns +inf


def _add(a, ea, b, eb):
    r = a + b
    return r, ea + eb + U * (np.abs(r) + ea + eb)


def _mul(a, ea, b, eb):
    r = a * b
    e = np.abs(a) * eb + np.abs(b) * ea + ea * eb
    return r, e + U * (np.abs(r) + e) + TINY


def _half(a, ea):
    return 0.5 * a, 0.5 * ea


def axis(a1, a2, d, dl):
    """One axis of decode_one in float64 from float32 inputs: (lo, hi) before the clip and the bound of the float32 evaluation's
    error on each.  All arguments are float64 arrays holding float32 values."""
    zero = np.zeros_like(a1)
    with np.errstate(over='ignore', invalid='ignore'):
        w, ew = _add(*_add(a2, zero, -a1, zero), 1.0, 0.0)
        hw, ehw = _half(w, ew)
        c, ec = _add(a1, zero, hw, ehw)
        pc, epc = _add(*_mul(d, zero, w, ew), c, ec)
        ex = np.exp(dl)
        p, ep = _mul(ex, EXPF_ULPS * 2.0 * U * ex + TINY, w, ew)
        hp, ehp = _half(p, ep)
        lo, elo = _add(pc, epc, -hp, ehp)
        hi, ehi = _add(pc, epc, hp, ehp)
    return lo, hi, elo, ehi


def clip_limit(size):
    """im_info's height or width -> the clip limit size - 1, which has to be exact in float32 for the bound to hold."""
    lim = np.float64(size) - 1.0
    assert np.float64(np.float32(size)) == np.float64(size) and np.float64(np.float32(lim)) == lim, size
    return lim
