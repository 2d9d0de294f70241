// What the two convolution backwards share (conv_backward.hip: exact fp32; conv_backward_f16x3.hip: 3 x f16 split): the kernel
// arguments, the call's layout, dgrad's operand gather (InPixelGather), the mask / bias pass with its defined summation order,
// and the split-K reduction.
// include/srcnn_hip.h states the definitions and the orders.
#pragma once
#include "conv_tile_4w.h"
#include "conv_train_geometry.h"
#include <cstdint>

namespace srcnn {

struct BwdArgs {
    const float *x, *w, *y, *dy;
    float *dx, *dw, *db, *g_out;
    const float *g;            // what the GEMMs read: gp, or dy in place
    int gcs, gco;              // its pixel stride and channel offset; it has Cp channels
    float *gp;                 // workspace: masked gradient (M, Cp), or nullptr
    float *db_part;            // workspace: bias partials (nq, Cp)
    float *wt;                 // workspace: weights (Cin, taps, Cp)
    float *partial;            // workspace: wgrad slices (splits, Cout, Kw)
    int H, W, Cin, xcs;
    int OH, OW, Cout, Cp;
    int KH, KW, stride, pad;
    int ycs, yco, relu;
    int M, Min;                // output pixels B OH OW, input pixels B H W
    int taps, Kw;              // KH KW, taps * Cin
    int d_ctiles, d_nkt, d_mtiles, d_ntiles;                // dgrad: Cp / 32, taps * d_ctiles, tile counts
    int w_nkt, w_kt_per_split, w_mtiles, w_ntiles;          // wgrad: ceil(M / 32), K tiles per slice, tile counts
};

struct BwdPlan {
    bool pass;                 // the mask / bias pass runs
    int d_mr, d_nr, w_mr, w_nr, splits, nq;
    size_t off_gp, off_db, off_wt, off_part, off_scale, bytes;
};

// dgrad's A operand: the thread's A_LD input pixels m0 + lrow + 32 i, and for a tap the output pixel whose gradient reaches them
// through it: ((h + pad - kh) / stride, (w + pad - kw) / stride) where both divisions are exact and in range.  Holds a reference
// to the kernel's arguments, like OutPixelGather.
template <int A_LD>
struct InPixelGather {
    const BwdArgs &p;
    int a_h[A_LD], a_w[A_LD], a_base[A_LD];
    __device__ __forceinline__ InPixelGather(int m0, int lrow, const BwdArgs &args) : p(args)
    {
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int m = m0 + lrow + 32 * i;
            if (m < p.Min) {
                const int hw = p.H * p.W;
                const int b = m / hw;
                const int rem = m - b * hw;
                const int h = rem / p.W;
                a_h[i] = h + p.pad;
                a_w[i] = rem - h * p.W + p.pad;
                a_base[i] = b * p.OH * p.OW;
            } else {
                a_h[i] = -(1 << 28);
                a_w[i] = 0;
                a_base[i] = 0;
            }
        }
    }
    // the thread's float4 of g at that output pixel, channels c .. c + 3 (zeros where no output pixel reads the input pixel there)
    __device__ __forceinline__ float4 load(int i, int kh, int kw, int c) const
    {
        const int th = a_h[i] - kh, tw = a_w[i] - kw;
        bool ok = th >= 0 && tw >= 0;
        const int oh = ok ? th / p.stride : 0, ow = ok ? tw / p.stride : 0;
        ok = ok && oh * p.stride == th && ow * p.stride == tw && oh < p.OH && ow < p.OW;
        const int pix = ok ? a_base[i] + oh * p.OW + ow : 0;
        const float4 v = *reinterpret_cast<const float4 *>(p.g + (size_t)pix * p.gcs + p.gco + c);
        return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
};

// ABSMAX (the f16x3 backward): the largest |g| of the call also goes into *gmax (wave_absmax_to_word); the word must be zero
// before the launch.
template <bool ABSMAX>
__global__ __launch_bounds__(256) void bwd_mask_bias_kernel(const BwdArgs p, unsigned *gmax)
{
    __shared__ float red[8][32];
    const int t = threadIdx.x, c = t & 31, r = t >> 5;
    const int n = blockIdx.y * 32 + c;          // < Cp
    const bool nok = n < p.Cout;
    const int m_base = blockIdx.x * 256;
    float s = 0.f, mx = 0.f;
    for (int i = 0; i < 32; ++i) {
        const int m = m_base + r + 8 * i;
        if (m >= p.M) break;
        float v = 0.f;
        if (nok) {
            const size_t o = (size_t)m * p.ycs + p.yco + n;
            v = p.dy[o];
            if (p.relu && !(p.y[o] > 0.f)) v = 0.f;
            if (p.g_out) p.g_out[(size_t)m * p.Cout + n] = v;
        }
        if (p.gp) p.gp[(size_t)m * p.Cp + n] = v;
        s += v;
        if (ABSMAX) mx = fmaxf(mx, fabsf(v));
    }
    if (ABSMAX) wave_absmax_to_word(mx, gmax);
    if (!p.db) return;
    red[r][c] = s;
    __syncthreads();
    if (r == 0) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) a += red[k][c];
        p.db_part[(size_t)blockIdx.x * p.Cp + n] = a;
    }
}

static __global__ __launch_bounds__(256) void bwd_bias_reduce_kernel(const BwdArgs p, int nq)
{
    __shared__ float red[8][32];
    const int t = threadIdx.x, c = t & 31, r = t >> 5;
    const int n = blockIdx.x * 32 + c;          // < Cp
    float s = 0.f;
    for (int q = r; q < nq; q += 8) s += p.db_part[(size_t)q * p.Cp + n];
    red[r][c] = s;
    __syncthreads();
    if (r == 0 && n < p.Cout) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) a += red[k][c];
        p.db[n] = a;
    }
}

static __global__ __launch_bounds__(256) void wgrad_reduce_kernel(const BwdArgs p, int splits)
{
    const size_t total = (size_t)p.Cout * p.Kw;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < splits; ++s) v += p.partial[(size_t)s * total + idx];
        p.dw[idx] = v;
    }
}

// Validates the descriptor and lays out the call: kernel arguments (workspace pointers as OFFSETS from nullptr until the caller
// binds them), tiles, slices and the workspace size.  f16x3: the descriptor must ask for precision 1, the mask pass always runs
// (it finds the gradient's scale), the re-laid weights are two f16 planes and four scale words are added.
static int bwd_prepare(const srcnn_conv_bwd_desc *d, BwdArgs &a, BwdPlan &pl, bool f16x3)
{
    SRCNN_REQUIRE(d != nullptr, "null descriptor");
    SRCNN_REQUIRE(d->dy != nullptr, "null pointer: dy");
    SRCNN_REQUIRE(d->dx || d->dw || d->db || d->g_out, "null pointer: no output requested");
    SRCNN_REQUIRE(!d->dw || d->x, "null pointer: dw needs x");
    SRCNN_REQUIRE(!d->dx || d->w, "null pointer: dx needs w");
    SRCNN_REQUIRE(!d->relu || d->y, "null pointer: relu needs the saved output y");
    SRCNN_REQUIRE(d->mode == 0, "mode 0 only (ConvTranspose2d and the RPN pair mode have no backward)");
    if (f16x3) SRCNN_REQUIRE(d->precision == 1, "precision must be 1 (the 3 x f16 split)");
    else SRCNN_REQUIRE(d->precision == 0, "precision must be 0 (the exact fp32 engine)");
    SRCNN_REQUIRE(d->x_format == SRCNN_FMT_F32 && d->y_format == SRCNN_FMT_F32, "format must be SRCNN_FMT_F32");
    SRCNN_REQUIRE(!d->head_w && !d->head_wf, "a fused head has no backward");
    SRCNN_REQUIRE(!d->x2, "a second input has no backward");
    SRCNN_REQUIRE(!d->up_top, "the fused upsample-add has no backward");
    SRCNN_REQUIRE(d->splits >= 0, "splits must be >= 0");
    const int rc = check_conv_geometry(__func__, d, d->dw != nullptr, a);
    if (rc != SRCNN_OK) return rc;
    a.x = d->x; a.w = d->w; a.y = d->y; a.dy = d->dy;
    a.dx = d->dx; a.dw = d->dw; a.db = d->db; a.g_out = d->g_out;
    const bool gemm = d->dx || d->dw;
    pl.pass = f16x3 || d->relu || d->db || d->g_out || d->Cout % BK != 0 || d->y_cstride % 4 != 0 || d->y_coffset % 4 != 0 ||
              (reinterpret_cast<uintptr_t>(d->dy) & 15) != 0;
    pl.nq = cdiv(a.M, 256);

    // dgrad tile: the forward's rule -- the largest tile that still gives two workgroups per CU
    choose_tile_4w(a.Min, a.Cin, &pl.d_mr, &pl.d_nr);
    // wgrad tile: M x N is small and K long, so the tile is as large as the matrix allows and split-K fills the chip
    pl.w_mr = a.Cout > 64 ? 2 : 1;
    pl.w_nr = a.Kw > 64 ? 2 : 1;
    if (d->tile_mr > 0 && d->tile_nr > 0) {
        pl.d_mr = pl.w_mr = d->tile_mr;
        pl.d_nr = pl.w_nr = d->tile_nr;
    }
    a.d_ctiles = a.Cp / BK;
    a.d_nkt = a.taps * a.d_ctiles;
    a.d_mtiles = cdiv(a.Min, 64 * pl.d_mr);
    a.d_ntiles = cdiv(a.Cin, 64 * pl.d_nr);
    SRCNN_REQUIRE((long long)a.d_mtiles * a.d_ntiles < (1LL << 31), "bad shape: tensor too large");
    a.w_nkt = cdiv(a.M, BK);
    a.w_mtiles = cdiv(a.Cout, 64 * pl.w_mr);
    a.w_ntiles = cdiv(a.Kw, 64 * pl.w_nr);
    SRCNN_REQUIRE((long long)a.w_mtiles * a.w_ntiles < (1LL << 31), "bad shape: tensor too large");
    int s = d->splits;
    if (s <= 0) {
        const long blocks = (long)a.w_mtiles * a.w_ntiles;
        s = (int)min(64L, (512 + blocks - 1) / blocks);
        s = min(s, max(1, a.w_nkt / 8));
    }
    s = max(1, min(min(s, a.w_nkt), 65535));
    a.w_kt_per_split = cdiv(a.w_nkt, s);
    pl.splits = cdiv(a.w_nkt, a.w_kt_per_split);

    size_t off = 0;
    auto take = [&](size_t floats) {
        const size_t at = off;
        off += align_up(floats * sizeof(float), 256);
        return at;
    };
    pl.off_gp = pl.off_db = pl.off_wt = pl.off_part = pl.off_scale = 0;
    if (pl.pass && gemm) pl.off_gp = take((size_t)a.M * a.Cp);
    if (d->db) pl.off_db = take((size_t)pl.nq * a.Cp);
    if (d->dx) pl.off_wt = take((size_t)a.Cin * a.taps * a.Cp);      // f16x3: the hi and the lo plane, two bytes each
    if (d->dw && pl.splits > 1) pl.off_part = take((size_t)pl.splits * a.Cout * a.Kw);
    if (f16x3) pl.off_scale = take(4);
    pl.bytes = off > 256 ? off : 256;
    return SRCNN_OK;
}

}  // namespace srcnn
