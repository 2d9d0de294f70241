// Convolution backward, error-compensated 3 x f16 form: dx and dw of conv_backward.hip on the f16 matrix pipe
// (v_mfma_f32_32x32x16_f16, fp32 accumulation), db and g_out from the very same mask / bias pass (conv_backward_common.h).
// include/srcnn_hip.h states the definitions; nothing here is derived from the reference (it calls cuDNN through torch.autograd).
//
// ARITHMETIC.  Every product of the two GEMMs is  a b ~ (a_hi b_hi + a_hi b_lo + a_lo b_hi) / (s_a s_b)  with
//   t = s v,  hi = f16(t),  lo = f16(t - hi)   (t and t - hi are exact in fp32; the lo lo term is dropped)
// as in conv_f16x3.hip.  What is new is s: gradients are routinely 1e-6 and smaller, and unscaled they would land in the f16
// subnormals.  Each operand TENSOR has one power of two, s = 2^(14 - floor(log2 max|v|)) (exponent clamped to +-126), so that
// its largest element lands in [2^14, 2^15) whatever the tensor's range is; an all-zero tensor gives s = 2^126 and exact zeros.
// max|v| is found on the device as the float's bits (integer atomicMax, order-independent): for g in the mask / bias pass,
// for w and x in one read-only pass each.  The three words live in the workspace, are cleared by the call's first kernel with
// plain stores, and are read by the kernels that split: nothing comes back to the host.  The sums are rescaled by the two exact
// powers of two in the epilogue.  A tensor's scale can only be known after a whole pass over it, so no pass can both find the
// scale of a tensor and split it: the weights (small, L2-resident) are read twice -- max, then re-layout + split into the hi and lo
// planes dgrad's B operand is -- while g and x stay fp32 in memory and are split while they are staged into LDS, as the
// forward splits its activations.
//
//   f16x3_clear_scales          the three max words <- 0
//   bwd_mask_bias_kernel<true>  conv_backward.hip's pass (g -> workspace (M, Cp), g_out, bias partials: same code, same bits) + max|g|
//   absmax_kernel               max|w|, max|x|
//   bwd_weight_relayout_split   w (Cout, taps, Cin) -> wt_hi, wt_lo (Cin, taps, Cp) f16
//   conv_dgrad_f16x3_kernel     conv_f16x3_kernel's tile (four swizzled f16 panels, one ds_read_b128 per MFMA operand) with
//                               conv_dgrad_kernel's gathered A operand.  Every element of dx is stored once, zeros included.
//   conv_wgrad_f16x3_kernel     see below
//   wgrad_reduce_kernel         split-K partials -> dw, ascending slice order (shared with the fp32 backward)
//
// WGRAD OPERAND LAYOUT.  K is the output pixel, and a lane of the f16 MFMA holds 8 consecutive k of one row, but memory holds a
// pixel's channels contiguously: both operands arrive transposed.  The choice here: TRANSPOSE IN REGISTERS ON THE WAY INTO LDS.
// A thread loads the same 4 channels (one float4) of P = 4 or 2 consecutive pixels, splits them, and stores per channel one
// 8- or 4-byte run of P halves into that channel's LDS row; the rows are then the forward's 64-byte K-contiguous rows and the
// MFMA loop is the forward's.  The alternative -- K-major hi / lo f16 planes emitted by the passes -- was not taken because
// (1) the scale is not known while the mask pass runs, so the planes would need a second pass over g and x each, writing and
// re-reading as many bytes as the fp32 tensors have; (2) a 3x3 layer needs x shifted and zero-padded per tap: in a K-major
// plane a run of 8 output pixels maps to 8 input pixels that start at any alignment and break at every image row, so the
// 16-byte loads the planes exist for would turn into per-element gathers for eight taps of nine, whereas with pixel-major
// fp32 x a tap is just another pixel index per load, as in the fp32 kernel.  The price is splitting both operands in the K
// loop (VALU work the fp32 kernel does not have).
// LDS rows are stored CHANNEL-PLANAR: the thread's channel 4 g + j sits in row j (BM / 4) + g of the panel, so that the 16 lanes
// that write channel j of 16 neighbouring groups hit 16 consecutive rows -- with the forward's XOR swizzle those are 16
// distinct 16-byte slots, and the lanes' pixel groups fill the slots' halves: conflict-free 8-byte / 4-byte stores.  An
// MFMA row is therefore a permuted channel; the epilogue undoes the permutation in its addresses.
//
// SUMMATION ORDER (fixed by the descriptor; no atomics outside the max words, whose result does not depend on order).
//   dx: K tiles over taps in (kh, kw) row-major order, inside a tap the 32-channel tiles of Cp ascending; a K tile is two MFMA
//       steps of 16 channels.  Per step the cross terms lo hi then hi lo are added into one accumulator, hi hi into another;
//       at the end main + cross, then * 1/s_g, then * 1/s_w.  Never split.
//   dw: K tiles of 32 pixels in ascending m inside the slice, the same two accumulators, main + cross, * 1/s_g, * 1/s_x; the
//       slices' (already rescaled) sums are added in ascending slice order by wgrad_reduce_kernel.
//   Inside one MFMA step the 16 products are summed by the matrix unit in its own fixed order.
//
// pow2_scale, split_f16, f16x3_clear_scales, absmax_kernel, the K tile's MFMA loop and dgrad's staging and K loop
// (f16x3_scaled_kloop) live in conv_f16x3_scaled.h, shared with the training forward (conv_forward_f16x3.hip); dgrad's gather
// (InPixelGather) lives in conv_backward_common.h, shared with the fp32 backward.
//
// srcnn_conv2d_backward_f16x3_maxima: the caller already holds max|x| of the saved x as a device word (the forward found it, or
// its producer's epilogue did); wgrad reads s_x from that word and the max|x| pass is not launched.  Nothing else differs.
//
// srcnn_conv2d_backward_f16x3_prepared: max|w| and the re-laid planes come from train_weights.hip (once per step for all layers);
// dgrad reads the caller's planes, absmax_kernel over w and bwd_weight_relayout_split are not launched, and the clear
// (f16x3_clear_scales_prepared) copies the layer's word into amax[1].  The GEMM kernels are unchanged.
#include "conv_backward_common.h"
#include "conv_f16x3_scaled.h"

namespace srcnn {

struct F16x3Args {
    _Float16 *wt_hi, *wt_lo;       // workspace: re-laid weights (Cin, taps, Cp), hi and lo plane
    unsigned *amax;                // workspace: float bits of max|g|, max|w|, max|x|
    const unsigned *xmax;          // the word wgrad takes s_x from: amax + 2, or the caller's x_amax
};

// bwd_weight_relayout with the split: grid (Cin / 32, Cp / 32, taps), block (32, 8)
__global__ __launch_bounds__(256) void bwd_weight_relayout_split(const BwdArgs p, const F16x3Args q)
{
    __shared__ float tile[32][33];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int c0 = blockIdx.x * 32, n0 = blockIdx.y * 32, tap = blockIdx.z;
    const float s = pow2_scale(q.amax[1]).s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + ty + 8 * j;
        tile[ty + 8 * j][tx] = n < p.Cout ? p.w[((size_t)n * p.taps + tap) * p.Cin + c0 + tx] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + ty + 8 * j;
        _Float16 hi, lo;
        split_f16(tile[tx][ty + 8 * j], s, hi, lo);
        const size_t o = ((size_t)c * p.taps + tap) * p.Cp + n0 + tx;
        q.wt_hi[o] = hi;
        q.wt_lo[o] = lo;
    }
}

template <int MR, int NR>
__global__ __launch_bounds__(256, 2) void conv_dgrad_f16x3_kernel(const BwdArgs p, const F16x3Args q)
{
    constexpr int BM = 64 * MR, BN = 64 * NR;
    __shared__ __attribute__((aligned(16))) _Float16 smem[2][f16x3_buf_halves(MR, NR)];

    const int t = threadIdx.x;
    const int logical = xcd_logical_tile(blockIdx.x, p.d_mtiles * p.d_ntiles);
    const int mt = logical / p.d_ntiles, nt = logical - mt * p.d_ntiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const Pow2 sg = pow2_scale(q.amax[0]), sw = pow2_scale(q.amax[1]);

    // A: conv_dgrad_kernel's gather (rows = input pixels).  B: rows = input channels of the re-laid planes, K = taps * Cp contiguous
    const int lrow = t >> 3, lcol = (t & 7) * 4;
    const InPixelGather<BM / 32> a(m0, lrow, p);
    const WaveGeom g(t);
    floatx16 acc[MR][NR], accx[MR][NR];
    f16x3_scaled_kloop(smem[0], a, lrow, lcol, sg.s, q.wt_hi, q.wt_lo, n0, p.Cin, p.d_ctiles, p.KW, p.d_nkt, g, acc, accx);

    // every (row, col) of the tile inside the tensor is stored, zeros included: dx needs no fill
#pragma unroll
    for (int i = 0; i < MR; ++i) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int col = c_col<NR>(g, n0, j);
            if (col >= p.Cin) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = c_row<MR>(g, m0, i, e);
                if (row >= p.Min) continue;
                p.dx[(size_t)row * p.xcs + col] = (acc[i][j][e] + accx[i][j][e]) * sg.inv * sw.inv;
            }
        }
    }
}

// One operand of the wgrad tile: R = 64 * (MR or NR) channel rows x 32 pixels.  Thread (cg, pg) owns channels 4 cg .. 4 cg + 3 of
// pixels P pg .. P pg + P - 1 of the K tile; 16 neighbouring cg are 16 neighbouring lanes (see the header: channel-planar rows).
template <int R>
struct WgradOperand {
    static constexpr int CG = R / 4, P = R / 32, NPG = 256 / CG;
    typedef _Float16 halfP __attribute__((ext_vector_type(P)));
    int cg, pg;
    float4 r[P];
    __device__ __forceinline__ explicit WgradOperand(int t) : cg((t & 15) + 16 * (t / (16 * NPG))), pg((t >> 4) % NPG) {}
    // registers -> the hi / lo panels (R rows each)
    __device__ __forceinline__ void store(_Float16 *hi_panel, _Float16 *lo_panel, float s) const
    {
        const int p0 = pg * P;
        float v[P][4];
#pragma unroll
        for (int k = 0; k < P; ++k) {
            v[k][0] = r[k].x; v[k][1] = r[k].y; v[k][2] = r[k].z; v[k][3] = r[k].w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            halfP hi, lo;
#pragma unroll
            for (int k = 0; k < P; ++k) {
                _Float16 h, l;
                split_f16(v[k][j], s, h, l);
                hi[k] = h;
                lo[k] = l;
            }
            const int row = j * CG + cg;
            const int o = row * HROW + (((p0 >> 3) ^ ((row >> 2) & 3)) << 3) + (p0 & 7);
            *reinterpret_cast<halfP *>(hi_panel + o) = hi;
            *reinterpret_cast<halfP *>(lo_panel + o) = lo;
        }
    }
    // the channel of LDS row `row`
    static __device__ __forceinline__ int channel(int row) { return 4 * (row % CG) + row / CG; }
};

template <int MR, int NR>
__global__ __launch_bounds__(256, 2) void conv_wgrad_f16x3_kernel(const BwdArgs p, const F16x3Args q)
{
    constexpr int BM = 64 * MR, BN = 64 * NR;
    constexpr int PANEL_A = BM * HROW, PANEL_B = BN * HROW;
    __shared__ __attribute__((aligned(16))) _Float16 smem[2][f16x3_buf_halves(MR, NR)];

    const int t = threadIdx.x;
    const int logical = xcd_logical_tile(blockIdx.x, p.w_mtiles * p.w_ntiles);
    const int mt = logical / p.w_ntiles, nt = logical - mt * p.w_ntiles;
    const int n0 = mt * BM, j0 = nt * BN;               // first output channel / first (tap, c) column of the tile
    const int kt_begin = blockIdx.y * p.w_kt_per_split;
    const int kt_end = min(p.w_nkt, kt_begin + p.w_kt_per_split);
    const Pow2 sg = pow2_scale(q.amax[0]), sx = pow2_scale(*q.xmax);

    // The two operand loads are conv_wgrad_kernel's, a second copy on purpose: see the comment there.
    // A: g rows.  This thread's channel group is the same in every K tile
    WgradOperand<BM> A(t);
    const bool a_ok = n0 + 4 * A.cg < p.Cp;
    const float *a_ptr = p.g + p.gco + (a_ok ? n0 + 4 * A.cg : 0);
    // B: x rows at a tap.  This thread's (tap, channel group) is the same in every K tile
    WgradOperand<BN> B(t);
    const int jcol = j0 + 4 * B.cg;
    const bool b_ok = jcol < p.Kw;
    const int tap = b_ok ? jcol / p.Cin : 0;
    const int cin0 = b_ok ? jcol - tap * p.Cin : 0;
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const int ohw = p.OH * p.OW;
    constexpr int PA = WgradOperand<BM>::P, PB = WgradOperand<BN>::P;

    auto load_tile = [&](int kt) {
#pragma unroll
        for (int k = 0; k < PA; ++k) {
            const int m = kt * BK + A.pg * PA + k;
            const bool ok = a_ok && m < p.M;
            const float4 v = *reinterpret_cast<const float4 *>(a_ptr + (size_t)(ok ? m : 0) * p.gcs);
            A.r[k] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < PB; ++k) {
            const int m = kt * BK + B.pg * PB + k;
            bool ok = b_ok && m < p.M;
            const int mm = ok ? m : 0;
            const int b = mm / ohw;
            const int rem = mm - b * ohw;
            const int oh = rem / p.OW;
            const int ih = oh * p.stride - p.pad + kh, iw = (rem - oh * p.OW) * p.stride - p.pad + kw;
            ok = ok && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
            const int pix = ok ? (b * p.H + ih) * p.W + iw : 0;
            const float4 v = *reinterpret_cast<const float4 *>(p.x + (size_t)pix * p.xcs + cin0);
            B.r[k] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store_tile = [&](int buf) {
        A.store(smem[buf], smem[buf] + PANEL_A, sg.s);
        B.store(smem[buf] + 2 * PANEL_A, smem[buf] + 2 * PANEL_A + PANEL_B, sx.s);
    };

    const WaveGeom g(t);
    floatx16 acc[MR][NR], accx[MR][NR];
    zero_acc(acc);
    zero_acc(accx);
    ktile_pipeline(kt_begin, kt_end, load_tile, store_tile, [&](int buf) { f16x3_ktile(smem[buf], g, acc, accx); });

    float *out = gridDim.y > 1 ? p.partial + (size_t)blockIdx.y * p.Cout * p.Kw : p.dw;
#pragma unroll
    for (int i = 0; i < MR; ++i) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int col = j0 + WgradOperand<BN>::channel(c_col<NR>(g, 0, j));
            if (col >= p.Kw) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = n0 + WgradOperand<BM>::channel(c_row<MR>(g, 0, i, e));
                if (row >= p.Cout) continue;
                out[(size_t)row * p.Kw + col] = (acc[i][j][e] + accx[i][j][e]) * sg.inv * sx.inv;
            }
        }
    }
}

// What srcnn_train_weights_prepare left for the layer (the _prepared entry)
struct BwdPrepared {
    const unsigned *w_amax;
    const void *wt_hi, *wt_lo;
    size_t plane_bytes;
};

// The _maxima and _prepared entries' body (below).  prep: the layer's word and re-laid planes, or null -- then the call scans,
// re-lays and splits w itself
static int bwd_f16x3_run(const srcnn_conv_bwd_desc *d, const unsigned *x_amax, const BwdPrepared *prep, void *workspace,
                         size_t workspace_bytes, srcnn_stream_t stream);

}  // namespace srcnn

extern "C" {

size_t srcnn_conv2d_backward_f16x3_workspace_bytes(const srcnn_conv_bwd_desc *d)
{
    using namespace srcnn;
    BwdArgs a;
    BwdPlan pl;
    if (bwd_prepare(d, a, pl, true) != SRCNN_OK) return 0;
    return pl.bytes;
}

int srcnn_conv2d_backward_f16x3(const srcnn_conv_bwd_desc *d, void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    return srcnn_conv2d_backward_f16x3_maxima(d, nullptr, workspace, workspace_bytes, stream);
}

int srcnn_conv2d_backward_f16x3_maxima(const srcnn_conv_bwd_desc *d, const unsigned *x_amax, void *workspace, size_t workspace_bytes,
                                       srcnn_stream_t stream)
{
    return srcnn::bwd_f16x3_run(d, x_amax, nullptr, workspace, workspace_bytes, stream);
}

int srcnn_conv2d_backward_f16x3_prepared(const srcnn_conv_bwd_desc *d, const unsigned *x_amax, const unsigned *w_amax, const void *wt_hi,
                                         const void *wt_lo, size_t plane_bytes, void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    const srcnn::BwdPrepared prep = {w_amax, wt_hi, wt_lo, plane_bytes};
    return srcnn::bwd_f16x3_run(d, x_amax, &prep, workspace, workspace_bytes, stream);
}

}  // extern "C"

namespace srcnn {

static int bwd_f16x3_run(const srcnn_conv_bwd_desc *d, const unsigned *x_amax, const BwdPrepared *prep, void *workspace,
                         size_t workspace_bytes, srcnn_stream_t stream)
{
    BwdArgs a;
    BwdPlan pl;
    int rc = bwd_prepare(d, a, pl, true);
    if (rc != SRCNN_OK) return rc;
    rc = check_amax_words(x_amax, nullptr);
    if (rc != SRCNN_OK) return rc;
    if (prep && d->dx) {                // the weight gradient reads no weights: without dx the three may be null
        rc = check_prepared_planes("srcnn_conv2d_backward_f16x3_prepared", prep->w_amax, prep->wt_hi, prep->wt_lo, prep->plane_bytes,
                                   (size_t)a.Cin * a.taps * a.Cp * sizeof(_Float16));
        if (rc != SRCNN_OK) return rc;
    }
    if (!workspace || workspace_bytes < pl.bytes) {
        set_error("srcnn_conv2d_backward_f16x3: workspace too small (%zu < %zu)", workspace ? workspace_bytes : (size_t)0, pl.bytes);
        return SRCNN_ERR_WORKSPACE;
    }
    char *ws = static_cast<char *>(workspace);
    const bool gemm = d->dx || d->dw;
    a.gp = gemm ? reinterpret_cast<float *>(ws + pl.off_gp) : nullptr;
    a.db_part = d->db ? reinterpret_cast<float *>(ws + pl.off_db) : nullptr;
    a.wt = nullptr;
    a.partial = (d->dw && pl.splits > 1) ? reinterpret_cast<float *>(ws + pl.off_part) : nullptr;
    a.g = a.gp; a.gcs = a.Cp; a.gco = 0;
    F16x3Args q;
    q.wt_hi = d->dx ? reinterpret_cast<_Float16 *>(ws + pl.off_wt) : nullptr;
    q.wt_lo = d->dx ? q.wt_hi + (size_t)a.Cin * a.taps * a.Cp : nullptr;
    q.amax = reinterpret_cast<unsigned *>(ws + pl.off_scale);
    q.xmax = x_amax ? x_amax : q.amax + 2;

    hipStream_t st = as_stream(stream);
    if (prep) {
        if (d->dx) {                    // dgrad reads the caller's planes; nothing writes them
            q.wt_hi = static_cast<_Float16 *>(const_cast<void *>(prep->wt_hi));
            q.wt_lo = static_cast<_Float16 *>(const_cast<void *>(prep->wt_lo));
        }
        SRCNN_LAUNCH(f16x3_clear_scales_prepared, dim3(1), dim3(64), 0, st, q.amax, static_cast<unsigned *>(nullptr),
                     d->dx ? prep->w_amax : static_cast<const unsigned *>(nullptr));
    } else {
        SRCNN_LAUNCH(f16x3_clear_scales, dim3(1), dim3(64), 0, st, q.amax, static_cast<unsigned *>(nullptr));
    }
    SRCNN_LAUNCH(bwd_mask_bias_kernel<true>, dim3(pl.nq, a.Cp / BK), dim3(256), 0, st, a, q.amax);
    if (d->db) SRCNN_LAUNCH(bwd_bias_reduce_kernel, dim3(a.Cp / BK), dim3(256), 0, st, a, pl.nq);
    if (d->dx) {
        if (!prep) {
            launch_absmax(a.w, a.Cout, a.Kw, a.Kw, q.amax + 1, st);
            SRCNN_LAUNCH(bwd_weight_relayout_split, dim3(a.Cin / BK, a.Cp / BK, a.taps), dim3(32, 8), 0, st, a, q);
        }
        dispatch_tile_4w(pl.d_mr, pl.d_nr, [&](auto mr, auto nr) {
            SRCNN_LAUNCH((conv_dgrad_f16x3_kernel<decltype(mr)::value, decltype(nr)::value>), dim3(a.d_mtiles * a.d_ntiles), dim3(256), 0, st, a, q);
        });
    }
    if (d->dw) {
        if (!x_amax) launch_absmax(a.x, a.Min, a.Cin, a.xcs, q.amax + 2, st);
        dispatch_tile_4w(pl.w_mr, pl.w_nr, [&](auto mr, auto nr) {
            SRCNN_LAUNCH((conv_wgrad_f16x3_kernel<decltype(mr)::value, decltype(nr)::value>), dim3(a.w_mtiles * a.w_ntiles, pl.splits), dim3(256), 0, st, a, q);
        });
        if (pl.splits > 1) {
            const size_t total = (size_t)a.Cout * a.Kw;
            SRCNN_LAUNCH(wgrad_reduce_kernel, dim3(grid_for(total, 256, 2048)), dim3(256), 0, st, a, pl.splits);
        }
    }
    return check_launch("srcnn_conv2d_backward_f16x3");
}

}  // namespace srcnn
