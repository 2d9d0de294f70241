// Training forward, error-compensated 3 x f16 form: y = relu?(conv(x, w) + bias + residual) on the f16 matrix pipe
// (v_mfma_f32_32x32x16_f16, fp32 accumulation) with the scales of conv_backward_f16x3.hip -- one power of two per operand tensor,
// found on the device -- so that weights that change every step need no prepared planes, no calibrated activation scale and no
// exponent on the host.  include/srcnn_hip.h states the definitions; nothing here is derived from the reference (it calls cuDNN).
// The inference f16x3 engine (conv_f16x3.hip, conv_f16s*) is another thing: prepared weights, host-known exponents, SPLIT16.
//
// ARITHMETIC.  conv_backward_f16x3.hip's, from the same header (conv_f16x3_scaled.h): t = s v, hi = f16(t), lo = f16(t - hi), every
// product hi hi + hi lo + lo hi, s = 2^(14 - floor(log2 max|v|)) with the exponent clamped to +-126; one s for x, one for w.
//
//   f16x3_clear_scales       the max words <- 0
//   absmax_kernel            max|w|, max|x| (x: channels [0, Cin) of every pixel; floats behind Cin are not read)
//   fwd_weight_split         w (Cout, taps, Cin) fp32 -> w_hi, w_lo (Cp, taps, Cin) f16, rows [Cout, Cp) zero.  K is already
//                            contiguous in the engine's layout: no transpose
//   conv_fwd_f16x3_kernel    conv_dgrad_f16x3_kernel's tile, staging and K loop (f16x3_scaled_kloop, conv_f16x3_scaled.h) with the
//                            forward's gather (OutPixelGather, conv_tile_4w.h): rows = the B OH OW output pixels, columns = Cout.
//                            x stays fp32 in memory and is split while it is staged into LDS; taps outside the image and rows
//                            beyond M are staged as zeros, whose halves are exact zeros.
//
// SUMMATION ORDER (fixed by the geometry alone: never split, and an element's K order does not depend on the tile it falls in).
//   K tiles over taps in (kh, kw) row-major order, inside a tap the 32-channel tiles of Cin ascending; a K tile is two MFMA steps
//   of 16 channels.  Per step cross += lo hi, main += hi hi, cross += hi lo; at the end (main + cross) * 1/s_x * 1/s_w, + bias,
//   + residual, ReLU, each rounded once.  Inside one MFMA step the 16 products are summed by the matrix unit in its own fixed order.
//
// No atomics other than the max words (whose result no order can change), no host read, no device-scope fence: every kernel
// reads what an earlier kernel of the same stream completed.
//
// PREPARED (srcnn_conv2d_forward_f16x3_prepared).  max|w| and the planes are functions of w alone; train_weights.hip computes them
// for all layers once per step.  The entry binds the caller's planes instead of the workspace's, launches neither absmax_kernel over
// w nor fwd_weight_split, and its clear (f16x3_clear_scales_prepared) copies the layer's word into amax[1]: the GEMM is unchanged.
//
// MAXIMA (srcnn_conv2d_forward_f16x3_maxima).  max|x| is a function of x alone, so a caller that already holds it as a device word
// (x_amax) spares the pass: the GEMM reads s_x from that word and absmax_kernel is not launched for x.  y_amax is the word the
// NEXT layer wants: the epilogue of conv_fwd_f16x3_kernel<.., true> keeps fmaxf(mx, |v|) over the values it stores (rows < M,
// columns < Cout, after bias, residual and ReLU), reduces it over the wave and issues one integer atomicMax per wave; the word is
// cleared by f16x3_clear_scales with the workspace's.  The <.., false> kernel is the one the plain entry launches.
#include "conv_f16x3_scaled.h"
#include "conv_train_geometry.h"

namespace srcnn {

struct FwdArgs {
    const float *x, *w, *bias, *res;
    float *y;
    _Float16 *w_hi, *w_lo;         // workspace: the weights' hi and lo plane (Cp, Kw)
    unsigned *amax;                // workspace: float bits of max|x|, max|w|
    const unsigned *xmax;          // the word s_x is taken from: amax, or the caller's x_amax
    unsigned *ymax;                // the caller's y_amax or null
    int H, W, Cin, xcs;
    int OH, OW, Cout, Cp;
    int KH, KW, stride, pad;
    int ycs, yco, relu;
    int M, Min;                    // output pixels B OH OW, input pixels B H W
    int taps, Kw;                  // KH KW, taps * Cin
    int ctiles, nkt, mtiles, ntiles;
};

struct FwdPlan {
    int mr, nr;
    size_t off_hi, off_lo, off_scale, bytes;
};

// one thread per 4 consecutive k of one row of the (Cp, Kw) planes
__global__ __launch_bounds__(256) void fwd_weight_split(const FwdArgs p)
{
    const int per_row = p.Kw / 4;
    const long long total = (long long)p.Cp * per_row;
    const float s = pow2_scale(p.amax[1]).s;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int n = (int)(i / per_row);
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n < p.Cout) f = *reinterpret_cast<const float4 *>(p.w + i * 4);
        half4 hi, lo;
        split_f16x4(f, s, hi, lo);
        *reinterpret_cast<half4 *>(p.w_hi + i * 4) = hi;
        *reinterpret_cast<half4 *>(p.w_lo + i * 4) = lo;
    }
}

template <int MR, int NR, bool YMAX>
__global__ __launch_bounds__(256, 2) void conv_fwd_f16x3_kernel(const FwdArgs p)
{
    constexpr int BM = 64 * MR, BN = 64 * NR;
    __shared__ __attribute__((aligned(16))) _Float16 smem[2][f16x3_buf_halves(MR, NR)];

    const int t = threadIdx.x;
    const int logical = xcd_logical_tile(blockIdx.x, p.mtiles * p.ntiles);
    const int mt = logical / p.ntiles, nt = logical - mt * p.ntiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const Pow2 sx = pow2_scale(*p.xmax), sw = pow2_scale(p.amax[1]);

    // A: the forward's gather (rows = output pixels); a row beyond M never passes the image test.  B: rows = output channels of the
    // Cp-row planes, K = taps * Cin contiguous
    const int lrow = t >> 3, lcol = (t & 7) * 4;
    const OutPixelGather<BM / 32, FwdArgs> a(m0, lrow, p);
    const WaveGeom g(t);
    floatx16 acc[MR][NR], accx[MR][NR];
    f16x3_scaled_kloop(smem[0], a, lrow, lcol, sx.s, p.w_hi, p.w_lo, n0, p.Cp, p.ctiles, p.KW, p.nkt, g, acc, accx);

    // every (row, col) of the tile inside (M, Cout) is stored once; the 32 lanes of a row write 128 contiguous bytes
    float mx = 0.f;                 // YMAX: max |v| over what this thread stores, nothing else
#pragma unroll
    for (int i = 0; i < MR; ++i) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int col = c_col<NR>(g, n0, j);
            if (col >= p.Cout) continue;
            const float bv = p.bias ? p.bias[col] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = c_row<MR>(g, m0, i, e);
                if (row >= p.M) continue;
                float v = (acc[i][j][e] + accx[i][j][e]) * sx.inv * sw.inv;
                if (p.bias) v += bv;
                if (p.res) v += p.res[(size_t)row * p.Cout + col];
                if (p.relu) v = fmaxf(v, 0.f);
                p.y[(size_t)row * p.ycs + p.yco + col] = v;
                if (YMAX) mx = fmaxf(mx, fabsf(v));
            }
        }
    }
    if (YMAX) wave_absmax_to_word(mx, p.ymax);
}

// Validates the descriptor and lays out the call (workspace pointers are bound by the caller)
static int fwd_prepare(const srcnn_conv_fwd_f16x3_desc *d, FwdArgs &a, FwdPlan &pl)
{
    SRCNN_REQUIRE(d != nullptr, "null descriptor");
    SRCNN_REQUIRE(d->x != nullptr, "null pointer: x");
    SRCNN_REQUIRE(d->w != nullptr, "null pointer: w");
    SRCNN_REQUIRE(d->y != nullptr, "null pointer: y");
    SRCNN_REQUIRE(d->x_format == SRCNN_FMT_F32 && d->y_format == SRCNN_FMT_F32, "format must be SRCNN_FMT_F32");
    SRCNN_REQUIRE((reinterpret_cast<uintptr_t>(d->w) & 15) == 0, "w must be 16-byte aligned (vector loads)");
    const int rc = check_conv_geometry(__func__, d, true, a);
    if (rc != SRCNN_OK) return rc;
    a.x = d->x; a.w = d->w; a.bias = d->bias; a.res = d->residual; a.y = d->y;
    a.w_hi = a.w_lo = nullptr; a.amax = nullptr; a.xmax = nullptr; a.ymax = nullptr;

    // the engine's rule: the largest tile that still gives two workgroups per CU
    choose_tile_4w(a.M, a.Cout, &pl.mr, &pl.nr);
    if (d->tile_mr > 0 && d->tile_nr > 0) {
        pl.mr = d->tile_mr;
        pl.nr = d->tile_nr;
    }
    a.ctiles = a.Cin / BK;
    a.nkt = a.taps * a.ctiles;
    a.mtiles = cdiv(a.M, 64 * pl.mr);
    a.ntiles = cdiv(a.Cout, 64 * pl.nr);
    SRCNN_REQUIRE((long long)a.mtiles * a.ntiles < (1LL << 31), "bad shape: tensor too large");

    const size_t plane = align_up((size_t)a.Cp * a.Kw * sizeof(_Float16), 256);
    pl.off_hi = 0;
    pl.off_lo = plane;
    pl.off_scale = 2 * plane;
    pl.bytes = 2 * plane + 256;
    return SRCNN_OK;
}

// What srcnn_train_weights_prepare left for the layer (the _prepared entry), or nothing
struct FwdPrepared {
    const unsigned *w_amax;
    const void *w_hi, *w_lo;
    size_t plane_bytes;
};

// The three entries' body.  x_amax / y_amax: the _maxima entry's words (null, null from the plain entry); prep: the _prepared
// entry's word and planes, or null -- then the call scans and splits w itself
static int fwd_run(const srcnn_conv_fwd_f16x3_desc *d, const unsigned *x_amax, unsigned *y_amax, const FwdPrepared *prep, void *workspace,
                   size_t workspace_bytes, srcnn_stream_t stream)
{
    FwdArgs a;
    FwdPlan pl;
    int rc = fwd_prepare(d, a, pl);
    if (rc != SRCNN_OK) return rc;
    rc = check_amax_words(x_amax, y_amax);
    if (rc != SRCNN_OK) return rc;
    if (prep) {
        rc = check_prepared_planes("srcnn_conv2d_forward_f16x3_prepared", prep->w_amax, prep->w_hi, prep->w_lo, prep->plane_bytes,
                                   (size_t)a.Cp * a.Kw * sizeof(_Float16));
        if (rc != SRCNN_OK) return rc;
        SRCNN_REQUIRE_AS("srcnn_conv2d_forward_f16x3_prepared", prep->w_amax != y_amax, "w_amax and y_amax alias: they must be two words");
    }
    if (!workspace || workspace_bytes < pl.bytes) {
        set_error("srcnn_conv2d_forward_f16x3: workspace too small (%zu < %zu)", workspace ? workspace_bytes : (size_t)0, pl.bytes);
        return SRCNN_ERR_WORKSPACE;
    }
    char *ws = static_cast<char *>(workspace);
    a.w_hi = reinterpret_cast<_Float16 *>(ws + pl.off_hi);
    a.w_lo = reinterpret_cast<_Float16 *>(ws + pl.off_lo);
    a.amax = reinterpret_cast<unsigned *>(ws + pl.off_scale);
    a.xmax = x_amax ? x_amax : a.amax;
    a.ymax = y_amax;

    hipStream_t st = as_stream(stream);
    if (prep) {
        // the GEMM reads the caller's planes; const is cast away for FwdArgs' sake, nothing writes them
        a.w_hi = static_cast<_Float16 *>(const_cast<void *>(prep->w_hi));
        a.w_lo = static_cast<_Float16 *>(const_cast<void *>(prep->w_lo));
        SRCNN_LAUNCH(f16x3_clear_scales_prepared, dim3(1), dim3(64), 0, st, a.amax, a.ymax, prep->w_amax);
    } else {
        SRCNN_LAUNCH(f16x3_clear_scales, dim3(1), dim3(64), 0, st, a.amax, a.ymax);
        launch_absmax(a.w, a.Cout, a.Kw, a.Kw, a.amax + 1, st);
    }
    if (!x_amax) launch_absmax(a.x, a.Min, a.Cin, a.xcs, a.amax, st);
    if (!prep) {
        const long long groups = (long long)a.Cp * (a.Kw / 4);
        SRCNN_LAUNCH(fwd_weight_split, dim3((unsigned)min(2048LL, (groups + 255) / 256)), dim3(256), 0, st, a);
    }
    dispatch_tile_4w(pl.mr, pl.nr, [&](auto mr, auto nr) {
        constexpr int MR = decltype(mr)::value, NR = decltype(nr)::value;
        if (a.ymax) SRCNN_LAUNCH((conv_fwd_f16x3_kernel<MR, NR, true>), dim3(a.mtiles * a.ntiles), dim3(256), 0, st, a);
        else SRCNN_LAUNCH((conv_fwd_f16x3_kernel<MR, NR, false>), dim3(a.mtiles * a.ntiles), dim3(256), 0, st, a);
    });
    return check_launch("srcnn_conv2d_forward_f16x3");
}

}  // namespace srcnn

extern "C" {

size_t srcnn_conv2d_forward_f16x3_workspace_bytes(const srcnn_conv_fwd_f16x3_desc *d)
{
    using namespace srcnn;
    FwdArgs a;
    FwdPlan pl;
    if (fwd_prepare(d, a, pl) != SRCNN_OK) return 0;
    return pl.bytes;
}

int srcnn_conv2d_forward_f16x3(const srcnn_conv_fwd_f16x3_desc *d, void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    return srcnn::fwd_run(d, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int srcnn_conv2d_forward_f16x3_maxima(const srcnn_conv_fwd_f16x3_desc *d, const unsigned *x_amax, unsigned *y_amax, void *workspace,
                                      size_t workspace_bytes, srcnn_stream_t stream)
{
    return srcnn::fwd_run(d, x_amax, y_amax, nullptr, workspace, workspace_bytes, stream);
}

int srcnn_conv2d_forward_f16x3_prepared(const srcnn_conv_fwd_f16x3_desc *d, const unsigned *x_amax, unsigned *y_amax, const unsigned *w_amax,
                                        const void *w_hi, const void *w_lo, size_t plane_bytes, void *workspace, size_t workspace_bytes,
                                        srcnn_stream_t stream)
{
    const srcnn::FwdPrepared prep = {w_amax, w_hi, w_lo, plane_bytes};
    return srcnn::fwd_run(d, x_amax, y_amax, &prep, workspace, workspace_bytes, stream);
}

int srcnn_absmax(const float *x, long long rows, int len, long long stride, unsigned *word, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(x != nullptr, "null pointer: x");
    SRCNN_REQUIRE(word != nullptr, "null pointer: word");
    SRCNN_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(word) & 3) == 0, "x and word must be 4-byte aligned");
    SRCNN_REQUIRE(rows > 0 && len > 0, "bad shape: rows and len must be positive");
    SRCNN_REQUIRE(stride >= len, "stride: a stride of at least len floats");
    SRCNN_REQUIRE(rows < (1LL << 31), "bad shape: tensor too large");
    hipStream_t st = as_stream(stream);
    SRCNN_LAUNCH(f16x3_clear_scales, dim3(1), dim3(64), 0, st, static_cast<unsigned *>(nullptr), word);
    launch_absmax(x, rows, len, stride, word, st);
    return check_launch("srcnn_absmax");
}

}  // extern "C"
