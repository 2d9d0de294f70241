// Convolution backward for the exact-fp32 engine: dx, dw, db of y = act(conv(x, w) + bias + residual) (srcnn_conv2d, mode 0).
//
// The reference calls cuDNN through torch.autograd for every learnable layer (stereo_rcnn/resnet.py:66-146,243-286;
// rpn/stereo_rpn.py:32-40); nothing here is derived from it.  include/srcnn_hip.h states the definitions, the scheme and the
// summation orders; this file is their implementation:
//
//   bwd_mask_bias_kernel     g = dy * [y > 0] -> workspace rows of Cp = roundup(Cout, 32) floats (zero padded), g_out, bias partials
//   bwd_bias_reduce_kernel   partials -> db, fixed order
//   bwd_weight_relayout      w (Cout, taps, Cin) -> wt (Cin, taps, Cp): dgrad's B operand, K-contiguous rows like the forward's weights
//   conv_dgrad_kernel        dx: the forward's implicit GEMM (conv_tile_4w.h: the same tile, LDS layout, prefetch, XCD remap) with the
//                            A operand GATHERED: row m = input pixel (b, h, w), K tile = 32 channels of g at output pixel
//                            ((h + pad - kh) / s, (w + pad - kw) / s) when that division is exact and in range, else zeros
//   conv_wgrad_kernel        dw: rows = Cout, columns = (tap, c), K = output pixels.  Both operands are K-strided in memory (a pixel's
//                            channels are contiguous), which is the fp32 MFMA's operand layout: lane l holds A[i = l & 31][k = l >> 5],
//                            so an LDS tile stored [k pixel][channel] -- written with 16-byte stores straight from coalesced
//                            global rows -- is read back with ds_read_b32 at consecutive addresses over the 32 lanes of a half
//                            wave: conflict-free (the two halves are served separately) and no padding is needed.
//   wgrad_reduce_kernel      split-K partials -> dw, ascending slice order
// (the mask / bias pass, the two reductions, the call's layout and dgrad's gather, InPixelGather, are in
// conv_backward_common.h: the f16x3 backward shares them)
#include "conv_backward_common.h"

namespace srcnn {

// grid (Cin / 32, Cp / 32, taps), block (32, 8): one 32 x 32 transpose per block through LDS, both sides coalesced
__global__ __launch_bounds__(256) void bwd_weight_relayout(const BwdArgs p)
{
    __shared__ float tile[32][33];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int c0 = blockIdx.x * 32, n0 = blockIdx.y * 32, tap = blockIdx.z;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + ty + 8 * j;
        tile[ty + 8 * j][tx] = n < p.Cout ? p.w[((size_t)n * p.taps + tap) * p.Cin + c0 + tx] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + ty + 8 * j;
        p.wt[((size_t)c * p.taps + tap) * p.Cp + n0 + tx] = tile[tx][ty + 8 * j];
    }
}

template <int MR, int NR>
__global__ __launch_bounds__(256, 2) void conv_dgrad_kernel(const BwdArgs p)
{
    constexpr int BM = 64 * MR, BN = 64 * NR;
    constexpr int A_LD = BM / 32, B_LD = BN / 32;   // float4 loads per thread per tile
    __shared__ __attribute__((aligned(16))) float smem[2][(BM + BN) * LDS_ROW];

    const int t = threadIdx.x;
    const int logical = xcd_logical_tile(blockIdx.x, p.d_mtiles * p.d_ntiles);
    const int mt = logical / p.d_ntiles, nt = logical - mt * p.d_ntiles;
    const int m0 = mt * BM, n0 = nt * BN;

    const int lrow = t >> 3;          // 0..31
    const int lcol = (t & 7) * 4;     // float offset inside the 32-float run
    const InPixelGather<A_LD> a(m0, lrow, p);
    const WeightRows<B_LD> b(p.wt, n0, lrow, lcol, p.Cin, (size_t)p.taps * p.Cp);

    float4 ra[A_LD], rb[B_LD];
    auto load_tile = [&](int kt) {
        const int tap = kt / p.d_ctiles;
        const int c0 = (kt - tap * p.d_ctiles) * BK;
        const int kh = tap / p.KW;
        const int kw = tap - kh * p.KW;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) ra[i] = a.load(i, kh, kw, c0 + lcol);
        b.load(kt, rb);
    };
    auto store_tile = [&](int buf) {      // conv_mfma_kernel's store
        float *sa = smem[buf];
        float *sb = smem[buf] + BM * LDS_ROW;
#pragma unroll
        for (int i = 0; i < A_LD; ++i)
            *reinterpret_cast<float4 *>(sa + (lrow + 32 * i) * LDS_ROW + lcol) = ra[i];
#pragma unroll
        for (int i = 0; i < B_LD; ++i)
            *reinterpret_cast<float4 *>(sb + (lrow + 32 * i) * LDS_ROW + lcol) = rb[i];
    };

    const WaveGeom g(t);
    floatx16 acc[MR][NR];
    zero_acc(acc);

    // Own copies of the LDS store, of ktile_pipeline and of the for_each_c walk (conv_tile_4w.h), kept after measurement: with for_each_c
    // the 24-channel RPN head (one K tile, all epilogue) is 1.4 % slower, and of the compositions without it this one is the
    // one whose every layer stays inside the run-to-run spread of the kernel as it was (profiles/conv_tile_core_ab.txt).
    const int nkt = p.d_nkt;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        const bool more = kt + 1 < nkt;
        if (more) load_tile(kt + 1);
        mfma_ktile_f32(smem[buf], g, acc);
        if (more) store_tile(buf ^ 1);
        __syncthreads();
    }

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
                p.dx[(size_t)row * p.xcs + col] = acc[i][j][e];
            }
        }
    }
}

template <int MR, int NR>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(const BwdArgs p)
{
    constexpr int BM = 64 * MR, BN = 64 * NR;
    constexpr int A_LD = BM / 32, B_LD = BN / 32;       // float4 loads per thread per tile (32 pixels x BM / 4 float4 over 256 threads)
    constexpr int A_Q = BM / 4, B_Q = BN / 4;           // float4 per pixel row
    constexpr int A_RS = 256 / A_Q, B_RS = 256 / B_Q;   // pixel rows covered by one pass of the 256 threads
    __shared__ __attribute__((aligned(16))) float smem[2][BK * (BM + BN)];

    const int t = threadIdx.x;
    const int logical = xcd_logical_tile(blockIdx.x, p.w_mtiles * p.w_ntiles);
    const int mt = logical / p.w_ntiles, nt = logical - mt * p.w_ntiles;
    const int n0 = mt * BM, j0 = nt * BN;               // first output channel / first (tap, c) column of the tile
    const int kt_begin = blockIdx.y * p.w_kt_per_split;
    const int kt_end = min(p.w_nkt, kt_begin + p.w_kt_per_split);

    // Own copy of the two operand loads that conv_wgrad_f16x3_kernel repeats, kept after measurement: with both kernels on one
    // shared pair of load functions the 24-channel layers, whose backward is mostly this kernel, were 3.5 % (RPN head) and 2.5 %
    // (linear heads) slower in two consecutive jobs, and with this copy back they are inside the parent-against-parent spread
    // (profiles/train_conv_staging_ab.txt).
    // A: g rows.  This thread's channel group is the same in every K tile
    const int a_c = (t % A_Q) * 4, a_r = t / A_Q;
    const bool a_ok = n0 + a_c < p.Cp;
    const float *a_ptr = p.g + p.gco + (a_ok ? n0 + a_c : 0);
    // B: x rows at a tap.  This thread's (tap, channel group) is the same in every K tile
    const int b_c = (t % B_Q) * 4, b_r = t / B_Q;
    const int jcol = j0 + b_c;
    const bool b_ok = jcol < p.Kw;
    const int tap = b_ok ? jcol / p.Cin : 0;
    const int cin0 = b_ok ? jcol - tap * p.Cin : 0;
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const int ohw = p.OH * p.OW;

    float4 ra[A_LD], rb[B_LD];
    auto load_tile = [&](int kt) {
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int m = kt * BK + a_r + A_RS * i;
            const bool ok = a_ok && m < p.M;
            const float4 v = *reinterpret_cast<const float4 *>(a_ptr + (size_t)(ok ? m : 0) * p.gcs);
            ra[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const int m = kt * BK + b_r + B_RS * i;
            bool ok = b_ok && m < p.M;
            const int mm = ok ? m : 0;
            const int b = mm / ohw;
            const int rem = mm - b * ohw;
            const int oh = rem / p.OW;
            const int ih = oh * p.stride - p.pad + kh, iw = (rem - oh * p.OW) * p.stride - p.pad + kw;
            ok = ok && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
            const int pix = ok ? (b * p.H + ih) * p.W + iw : 0;
            const float4 v = *reinterpret_cast<const float4 *>(p.x + (size_t)pix * p.xcs + cin0);
            rb[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store_tile = [&](int buf) {
        float *sa = smem[buf];
        float *sb = smem[buf] + BK * BM;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) *reinterpret_cast<float4 *>(sa + (a_r + A_RS * i) * BM + a_c) = ra[i];
#pragma unroll
        for (int i = 0; i < B_LD; ++i) *reinterpret_cast<float4 *>(sb + (b_r + B_RS * i) * BN + b_c) = rb[i];
    };

    const WaveGeom g(t);
    floatx16 acc[MR][NR];
    zero_acc(acc);
    ktile_pipeline(kt_begin, kt_end, load_tile, store_tile, [&](int buf) {
        // lane (li, lg) of MFMA step ks holds A[n = li][pixel 2 ks + lg] and B[pixel 2 ks + lg][column li]: ascending pixel order
        const float *sa = smem[buf] + g.lg * BM + g.wm * 32 * MR + g.li;
        const float *sb = smem[buf] + BK * BM + g.lg * BN + g.wn * 32 * NR + g.li;
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) {
            float fa[MR], fb[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i) fa[i] = sa[2 * ks * BM + i * 32];
#pragma unroll
            for (int j = 0; j < NR; ++j) fb[j] = sb[2 * ks * BN + j * 32];
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int j = 0; j < NR; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
    });

    float *out = gridDim.y > 1 ? p.partial + (size_t)blockIdx.y * p.Cout * p.Kw : p.dw;
    for_each_c(acc, g, n0, j0, p.Cout, p.Kw, [&](int row, int col, float v) { out[(size_t)row * p.Kw + col] = v; });
}

}  // namespace srcnn

extern "C" {

size_t srcnn_conv2d_backward_workspace_bytes(const srcnn_conv_bwd_desc *d)
{
    using namespace srcnn;
    BwdArgs a;
    BwdPlan pl;
    if (bwd_prepare(d, a, pl, false) != SRCNN_OK) return 0;
    return pl.bytes;
}

int srcnn_conv2d_backward(const srcnn_conv_bwd_desc *d, void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    using namespace srcnn;
    BwdArgs a;
    BwdPlan pl;
    int rc = bwd_prepare(d, a, pl, false);
    if (rc != SRCNN_OK) return rc;
    if (!workspace || workspace_bytes < pl.bytes) {
        set_error("srcnn_conv2d_backward: workspace too small (%zu < %zu)", workspace ? workspace_bytes : (size_t)0, pl.bytes);
        return SRCNN_ERR_WORKSPACE;
    }
    char *ws = static_cast<char *>(workspace);
    const bool gemm = d->dx || d->dw;
    a.gp = (pl.pass && gemm) ? reinterpret_cast<float *>(ws + pl.off_gp) : nullptr;
    a.db_part = d->db ? reinterpret_cast<float *>(ws + pl.off_db) : nullptr;
    a.wt = d->dx ? reinterpret_cast<float *>(ws + pl.off_wt) : nullptr;
    a.partial = (d->dw && pl.splits > 1) ? reinterpret_cast<float *>(ws + pl.off_part) : nullptr;
    if (pl.pass) {
        a.g = a.gp; a.gcs = a.Cp; a.gco = 0;
    } else {
        a.g = a.dy; a.gcs = a.ycs; a.gco = a.yco;
    }
    hipStream_t st = as_stream(stream);
    if (pl.pass) {
        SRCNN_LAUNCH(bwd_mask_bias_kernel<false>, dim3(pl.nq, a.Cp / BK), dim3(256), 0, st, a, (unsigned *)nullptr);
        if (d->db) SRCNN_LAUNCH(bwd_bias_reduce_kernel, dim3(a.Cp / BK), dim3(256), 0, st, a, pl.nq);
    }
    if (d->dx) {
        SRCNN_LAUNCH(bwd_weight_relayout, dim3(a.Cin / BK, a.Cp / BK, a.taps), dim3(32, 8), 0, st, a);
        dispatch_tile_4w(pl.d_mr, pl.d_nr, [&](auto mr, auto nr) {
            SRCNN_LAUNCH((conv_dgrad_kernel<decltype(mr)::value, decltype(nr)::value>), dim3(a.d_mtiles * a.d_ntiles), dim3(256), 0, st, a);
        });
    }
    if (d->dw) {
        dispatch_tile_4w(pl.w_mr, pl.w_nr, [&](auto mr, auto nr) {
            SRCNN_LAUNCH((conv_wgrad_kernel<decltype(mr)::value, decltype(nr)::value>), dim3(a.w_mtiles * a.w_ntiles, pl.splits), dim3(256), 0, st, a);
        });
        if (pl.splits > 1) {
            const size_t total = (size_t)a.Cout * a.Kw;
            SRCNN_LAUNCH(wgrad_reduce_kernel, dim3(grid_for(total, 256, 2048)), dim3(256), 0, st, a, pl.splits);
        }
    }
    return check_launch("srcnn_conv2d_backward");
}

}  // extern "C"
