"""The case table of the SPLIT16 DMA-ring convolution kernel's reference tests (csrc/conv_f16s.hip, conv_f16s_tile.h,
conv_f16s_body.inc), shared by tests/test_conv_f16s_cases_cpu.py -- which asserts, without a GPU or the library, that every case
still has the property that earns it its place -- and tests/test_conv_f16s_matrix_gpu.py, which runs every case on every
instantiation against float64 torch.  Nothing here imports torch or the package.

A case's sizes are the smallest at which its path can still go wrong; `expect` writes the property out as numbers, and the CPU
test recomputes each of them from the geometry with the functions below, so that an edit of a shape that hollows a case out fails
there."""
import collections

# Every (tile_mr, tile_nr, waves, stages) of launch_conv_f16s -> the per-wave tile (MR, NR) of its instantiation, in 32x32 MFMA
# blocks: the workgroup tile is (64 mr) x (64 nr), `waves` wavefronts share it.
PER_WAVE = collections.OrderedDict([
    ((1, 1, 4, 2), (1, 1)), ((1, 1, 4, 4), (1, 1)),
    ((2, 1, 4, 2), (2, 1)), ((2, 1, 4, 3), (2, 1)),
    ((1, 2, 4, 2), (1, 2)), ((1, 2, 4, 3), (1, 2)),
    ((2, 2, 4, 2), (2, 2)),
    ((2, 2, 8, 2), (1, 2)), ((2, 2, 8, 4), (1, 2)),      # 128x128 on 8 waves of 32x64
    ((4, 2, 8, 3), (2, 2)),                              # 256x128 on 8 waves of 64x64
    ((4, 4, 8, 2), (2, 4)),                              # 256x256 on 8 waves of 64x128
    ((4, 4, 4, 2), (4, 4)),                              # 256x256 on 4 waves of 128x128
    ((4, 2, 4, 2), (4, 2)), ((4, 2, 4, 3), (4, 2)),      # 256x128 on 4 waves of 128x64
    ((2, 4, 4, 2), (2, 4)), ((2, 4, 4, 3), (2, 4)),      # 128x256 on 4 waves of 64x128
])
PLANS = list(PER_WAVE)
assert len(PLANS) == 16


def chains(plan):
    """Accumulator chains the three split products of a K step are kept in: a per-wave tile of >= 4 blocks has one, of 2 blocks two,
    of 1 block three.  Unsplit plans with the same number add a row's products in the same order and give identical bits
    (test_conv_f16s_plans_of_one_order_class_give_the_same_bits in tests/test_ops_gpu.py lists the same classes)."""
    blocks = PER_WAVE[tuple(plan[:4])][0] * PER_WAVE[tuple(plan[:4])][1]
    return 1 if blocks >= 4 else 2 if blocks == 2 else 3


ORDER_CLASSES = [[p for p in PLANS if chains(p) == n] for n in (1, 2, 3)]


def vector_only(plan):
    """The instantiations that have no scalar general epilogue (per-wave tile of >= 8 blocks: `if constexpr (MR * NR < 8)` in
    conv_f16s_body.inc): every 256x256 tile and the 4-wave 256x128 / 128x256.  conv_f16s_plan_ok refuses them for a convolution whose
    vector-epilogue predicate is false, and the library then launches its heuristic plan: the one documented fallback.  (256x128 on
    8 waves has 64x64 per wave and carries the general epilogue.)"""
    mr, nr = PER_WAVE[tuple(plan[:4])]
    return mr * nr >= 8


Case = collections.namedtuple('Case', 'id kind B H W cin cout k stride pad bn bias relu res y_fmt y_cstride y_coffset res_cstride '
                                      'splits why expect')
# kind: 'conv' (mode 0), 'deconv' (mode 1: ConvTranspose2d(2, 2), cout = channels per output pixel cq, the GEMM has N = 4 cq),
#       'stem' (7x7/2 pad 3 through prep_stem + stem_pack: x_cstride 4, 7x1 taps of 32 floats, stride 2; H, W are the image's)
# res: None, 'split16' or 'f32';  y_fmt: 0 F32, 1 SPLIT16;  y_cstride / res_cstride None = dense;  splits: requests besides 1
# expect: M, N, nkt;  exact_m / exact_n: the tile heights / widths (of 64, 128, 256) that divide M / N -- every other is ragged;
#         slices: {splits request: [K tiles of each slice]};  vector: the epilogue predicate;  m_fast: the FC tile order;
#         inside: (mode 1) {tile width: the tile boundaries below N, each of which falls strictly inside an (i, j) tap group}


def _c(id, kind, shape, k, stride, pad, why, expect, bn=False, bias=False, relu=False, res=None, y_fmt=1, y_cstride=None, y_coffset=0,
       res_cstride=None, splits=()):
    B, H, W, cin, cout = shape
    return Case(id, kind, B, H, W, cin, cout, k, stride, pad, bn, bias, relu, res, y_fmt, y_cstride, y_coffset, res_cstride,
                tuple(splits), why, expect)


_RAGGED = dict(M=1702, N=200, nkt=27, exact_m=(), exact_n=(), slices={1: [27], 3: [9, 9, 9], 4: [7, 7, 7, 6]}, vector=True, m_fast=False)

CASES = [
    _c('ragged3x3', 'conv', (2, 23, 37, 96, 200), 3, 1, 1,
       'M = 1702 and N = 200 are ragged for every tile, border taps, 27 K tiles (a short last slice at splits 4): also on the five '
       '4-wave big tiles, which no other reference test runs at a ragged shape or with split-K',
       _RAGGED, bn=True, relu=True, res='split16', y_fmt=1, splits=(3, 4)),
    _c('f32out-res16', 'conv', (2, 23, 37, 96, 200), 3, 1, 1,
       'OUT_SPLIT = false on every tile, SPLIT16 residual', _RAGGED, bn=True, relu=True, res='split16', y_fmt=0, splits=(3, 4)),
    _c('f32out-res32', 'conv', (2, 23, 37, 96, 200), 3, 1, 1,
       'OUT_SPLIT = false and res_fmt = 0 (an F32 residual into a SPLIT16 launch) on every tile',
       _RAGGED, bn=True, relu=True, res='f32', y_fmt=0, splits=(3, 4)),
    _c('narrow', 'conv', (1, 9, 11, 64, 20), 1, 1, 0,
       'cq % 8 != 0: the scalar general epilogue (production: the narrow heads); K = 2 tiles, so splits 2 is one tile per slice '
       'and the split-K reduction kernel takes its scalar branch',
       dict(M=99, N=20, nkt=2, exact_m=(), exact_n=(), slices={1: [2], 2: [1, 1]}, vector=False, m_fast=False),
       bias=True, y_fmt=0, splits=(2,)),
    _c('slice', 'conv', (1, 9, 11, 64, 24), 1, 1, 0,
       'cq = 24 is a multiple of 8: the vector predicate is false through the output slice alone (channels [4, 28) of 36); '
       'channels [0, 4) and [28, 36) keep their canary bits',
       dict(M=99, N=24, nkt=2, exact_m=(), exact_n=(), slices={1: [2]}, vector=False, m_fast=False),
       bias=True, y_fmt=0, y_cstride=36, y_coffset=4),
    _c('slice8', 'conv', (2, 12, 21, 64, 72), 3, 1, 1,
       'the vector epilogue with every stride different: cq 72, y SPLIT16 in channels [8, 80) of 88, SPLIT16 residual rows of 80; '
       'canary bits around the slice',
       dict(M=504, N=72, nkt=18, exact_m=(), exact_n=(), slices={1: [18]}, vector=True, m_fast=False),
       bias=True, relu=True, res='split16', y_fmt=1, y_cstride=88, y_coffset=8, res_cstride=80),
    _c('deconv40-y16', 'deconv', (2, 9, 11, 64, 40), 1, 1, 0,
       'the mode-1 pixel scatter of the vector epilogues when a 64- or 128-column tile boundary falls inside an (i, j) group; a '
       '256-wide tile holds all four taps; SPLIT16 output',
       dict(M=198, N=160, nkt=2, exact_m=(), exact_n=(), slices={1: [2]}, vector=True, m_fast=False,
            inside={64: [64, 128], 128: [128], 256: []}),
       bias=True, relu=True, y_fmt=1),
    _c('deconv40-y32', 'deconv', (2, 9, 11, 64, 40), 1, 1, 0,
       'the same scatter with OUT_SPLIT = false',
       dict(M=198, N=160, nkt=2, exact_m=(), exact_n=(), slices={1: [2]}, vector=True, m_fast=False,
            inside={64: [64, 128], 128: [128], 256: []}),
       bias=True, relu=True, y_fmt=0),
    _c('deconv6', 'deconv', (2, 5, 7, 32, 6), 1, 1, 0,
       'the mode-1 scatter of the scalar general epilogue (cq = 6): all four taps inside the first 24 columns of one tile',
       dict(M=70, N=24, nkt=1, exact_m=(), exact_n=(), slices={1: [1]}, vector=False, m_fast=False,
            inside={64: [], 128: [], 256: []}),
       bias=True, y_fmt=0),
    _c('stem131', 'stem', (2, 37, 131, 3, 64), 7, 2, 3,
       'the packed-stem geometry (x_cstride 4, 7x1 taps, stride 2) on every tile; odd packed width 139',
       dict(M=2508, N=64, nkt=7, exact_m=(), exact_n=(64,), slices={1: [7]}, vector=True, m_fast=False),
       bn=True, relu=True, y_fmt=1),
    _c('stem130', 'stem', (2, 37, 130, 3, 64), 7, 2, 3,
       'the packed-stem geometry; even packed width 138',
       dict(M=2470, N=64, nkt=7, exact_m=(), exact_n=(64,), slices={1: [7]}, vector=True, m_fast=False),
       bn=True, relu=True, y_fmt=1),
    _c('stride2', 'conv', (2, 21, 33, 64, 136), 1, 2, 0,
       'odd input sizes under a stride-2 1x1 conv (11 x 17 outputs); N = 136 is ragged',
       dict(M=374, N=136, nkt=2, exact_m=(), exact_n=(), slices={1: [2]}, vector=True, m_fast=False),
       bn=True, relu=True, y_fmt=1),
    _c('fc', 'conv', (1, 6, 25, 64, 328), 1, 1, 0,
       'M = 150 < Cout: the FC tile order m_fast (mt = logical % mtiles), three M tiles of 64',
       dict(M=150, N=328, nkt=2, exact_m=(), exact_n=(), slices={1: [2]}, vector=True, m_fast=True),
       bias=True, y_fmt=1),
]
BY_ID = collections.OrderedDict((c.id, c) for c in CASES)
assert len(BY_ID) == len(CASES)


# ---- the geometry, recomputed ------------------------------------------------------------------------------------------------
def out_hw(c):
    """(OH, OW) of the GEMM's rows: the conv's output grid (the deconv's GEMM runs over its input grid)."""
    if c.kind == 'deconv':
        return c.H, c.W
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def gemm(c):
    """(M, N, K tiles) of the case's GEMM.  The stem's K is 7 row taps of 32 floats (8 pixels x NHWC4)."""
    oh, ow = out_hw(c)
    n = 4 * c.cout if c.kind == 'deconv' else c.cout
    k = 7 * 32 if c.kind == 'stem' else c.k * c.k * c.cin
    assert k % 32 == 0
    return c.B * oh * ow, n, k // 32


def strides(c):
    """(cq, y_cstride, y_coffset, res_cstride or None) as the descriptor carries them."""
    cq = c.cout
    return cq, (cq if c.y_cstride is None else c.y_cstride), c.y_coffset, \
        (None if c.res is None else (c.cout if c.res_cstride is None else c.res_cstride))


def vector_epilogue(c):
    """The condition under which the kernel takes its vector epilogues (conv_f16s_body.inc: cq, ycs, yco and, with a residual, rcs
    all multiples of 8); false = the scalar general epilogue."""
    cq, ycs, yco, rcs = strides(c)
    return cq % 8 == 0 and ycs % 8 == 0 and yco % 8 == 0 and (rcs is None or rcs % 8 == 0)


def slice_lengths(nkt, splits, mode1=False):
    """K tiles per split-K slice as plan_for forms them from a request: never split in mode 1, at most one slice per K tile, equal
    slices of ceil(nkt / s) with a shorter last one, and no empty slice."""
    s = 1 if mode1 else min(max(splits, 1), nkt)
    per = -(-nkt // s)
    n = -(-nkt // per)
    return [min(per, nkt - i * per) for i in range(n)]


def expected_plan(plan, nkt, mode1=False, never_split=False):
    """What srcnn_conv2d_plan must report for an implemented request (mr, nr, waves, stages, splits)."""
    return tuple(plan[:4]) + (len(slice_lengths(nkt, 1 if never_split else plan[4], mode1)),)


def falls_back(c, plan):
    """The documented fallback: a vector-epilogue-only instantiation asked for a convolution that needs the general epilogue."""
    return vector_only(plan) and not vector_epilogue(c)


def boundaries_inside_groups(c, bn):
    """(mode 1) the multiples of the tile width bn below N that fall strictly inside an (i, j) group of cq columns."""
    cq, n = c.cout, 4 * c.cout
    return [b for b in range(bn, n, bn) if b % cq != 0]


def launches(c):
    """Every (plan, splits request) the matrix runs for the case: all sixteen instantiations unsplit and at each extra request."""
    return [(p, s) for s in (1,) + c.splits for p in PLANS]
