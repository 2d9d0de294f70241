// The 4-wave implicit-GEMM workgroup shared by conv_mfma_kernel, conv_f16x3_kernel, conv_dgrad_kernel, conv_wgrad_kernel and the
// training-side f16x3 kernels (conv_f16x3_scaled.h):
// 256 threads as a 2x2 wave grid, (32*MR)x(32*NR) wave tiles of 32x32 MFMAs, register prefetch, double-buffered LDS.
//
// The forward kernels compute
//   y[m, n] = act( sum_k A[m, k] * W[n, k] + bias[n] + residual[m, n] )
//   m = (b, oh, ow)   k = (kh, kw, c)   n = cout          NHWC activations, W = [Cout][KH][KW][Cin]
// and the design note below is written for them; dgrad is the same GEMM with rows = input pixels and a gathered A operand, wgrad
// has rows = Cout, columns = (tap, c), K = output pixels and its own LDS layout (conv_backward.hip states both).
//
// Design (MI355X-first, not a cuDNN/CUTLASS shape):
//   * v_mfma_f32_32x32x2_f32: exact fp32 (bitwise an fmaf chain), 157 TF peak.  It is paced at
//     64 cycles/instruction, so LDS/HBM pressure per flop is 16x lower than a bf16 GEMM: a 2x2
//     wave grid with (32*MR)x(32*NR) wave tiles saturates the pipe without deep pipelining.
//   * K order inside a 32-wide K tile is permuted so that ONE ds_read_b128 feeds FOUR MFMAs:
//     lane (i, g) reads k = kk*8 + g*4 .. +3 of row i; MFMA s pairs k=kk*8+s (g=0) with
//     k=kk*8+4+s (g=1) on both operands.  The sum over k is order-independent in exact
//     arithmetic; in fp32 it is one fixed, deterministic order.
//   * LDS rows are 32 floats + 4 pad (144 B): the 16-lane groups of ds_read_b128 then touch 16
//     distinct 4-bank slots -> conflict-free; ds_write_b128 writes one row per 8 lanes.
//   * im2col is never materialised: a K tile is 32 contiguous channels of one (kh, kw) tap,
//     i.e. one 128-B run per output pixel, fetched as 8 lanes x 16 B (coalesced), zero-filled
//     outside the image.  Global->register prefetch of tile t+1 overlaps the MFMAs of tile t;
//     LDS is double-buffered -> one barrier per K tile.
//   * 256 CUs / 8 XCDs: tile ids are remapped so that consecutive logical tiles (which share the
//     activation rows) run on the same XCD and hit its L2; small-M layers use split-K so that
//     the grid still covers the chip (partials in the caller's workspace, deterministic reduce).
//   * epilogue fuses folded-BN bias, residual add, ReLU, channel-offset writes (concat in place)
//     and the ConvTranspose2d(2,2) pixel scatter.
#pragma once
#include "conv_common.h"
#include <type_traits>

namespace srcnn {

// bijective XCD-aware tile id (blocks b -> XCD b % 8): consecutive logical tiles run on one XCD and share its L2
__device__ __forceinline__ int xcd_logical_tile(int bid, int nblk)
{
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = bid & 7, slot = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

// wave (wm, wn) of the 2x2 grid; lane (li, lg) of a 32x32 MFMA
struct WaveGeom {
    int wm, wn, li, lg;
    __device__ __forceinline__ explicit WaveGeom(int t) : wm(t >> 7), wn((t >> 6) & 1), li(t & 31), lg((t & 63) >> 5) {}
};

template <int MR, int NR>
__device__ __forceinline__ void zero_acc(floatx16 (&acc)[MR][NR])
{
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}

// K tiles [kt_begin, kt_end): load(kt) global -> registers, store(buf) registers -> LDS buffer, compute(buf) the MFMAs of a buffer.
// The loads of tile t+1 are in flight under the MFMAs of tile t; two LDS buffers -> one barrier per K tile.
template <class Load, class Store, class Compute>
__device__ __forceinline__ void ktile_pipeline(int kt_begin, int kt_end, Load load, Store store, Compute compute)
{
    if (kt_begin < kt_end) {
        load(kt_begin);
        store(0);
    }
    __syncthreads();
    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const int buf = (kt - kt_begin) & 1;
        const bool more = kt + 1 < kt_end;
        if (more) load(kt + 1);
        compute(buf);
        if (more) store(buf ^ 1);
        __syncthreads();
    }
}

// Forward A operand: the thread's A_LD output pixels m0 + lrow + 32 i, and for a tap whether it lies inside the image and where.
// Holds a reference to the kernel's argument struct (ConvArgs, or any struct with its x, xcs, H, W, OH, OW, stride, pad, M): a
// local of the kernel, never stored or returned.
template <int A_LD, class Args = ConvArgs>
struct OutPixelGather {
    const Args &p;
    int ih0[A_LD], iw0[A_LD], pix0[A_LD];
    __device__ __forceinline__ OutPixelGather(int m0, int lrow, const Args &args) : p(args)
    {
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int m = m0 + lrow + 32 * i;
            if (m < p.M) {
                const int ohw = p.OH * p.OW;
                const int b = m / ohw;
                const int rem = m - b * ohw;
                const int oh = rem / p.OW;
                const int ow = rem - oh * p.OW;
                ih0[i] = oh * p.stride - p.pad;
                iw0[i] = ow * p.stride - p.pad;
                pix0[i] = (b * p.H + ih0[i]) * p.W + iw0[i];
            } else {
                ih0[i] = -(1 << 28);
                iw0[i] = 0;
                pix0[i] = 0;
            }
        }
    }
    __device__ __forceinline__ bool tap(int i, int kh, int kw, int &pix) const
    {
        const int ih = ih0[i] + kh, iw = iw0[i] + kw;
        const bool ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
        pix = ok ? pix0[i] + kh * p.W + kw : 0;
        return ok;
    }
    // the thread's float4 of the tap's 32-channel run starting at channel c (zeros outside the image)
    __device__ __forceinline__ float4 load(int i, int kh, int kw, int c) const
    {
        int pix;
        const bool ok = tap(i, kh, kw, pix);
        const float4 v = *reinterpret_cast<const float4 *>(p.x + (size_t)pix * p.xcs + c);
        return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
};

// A thread's max |v| (>= 0, NaNs already dropped by fmaxf) -> the word: one integer atomicMax on the float bits (which order like
// the values for non-negative floats) per wave, none for a wave of zeros.  Every lane of the wave must call it.
__device__ __forceinline__ void wave_absmax_to_word(float mx, unsigned *word)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(word, __float_as_uint(mx));
}

// fp32 B operand: the thread's B_LD rows n0 + lrow + 32 i of a K-contiguous (rows, K) matrix, rows beyond `rows` read as zeros
template <int B_LD>
struct WeightRows {
    const float *ptr[B_LD];
    bool ok[B_LD];
    __device__ __forceinline__ WeightRows(const float *w, int n0, int lrow, int lcol, int rows, size_t K)
    {
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const int n = n0 + lrow + 32 * i;
            ok[i] = n < rows;
            ptr[i] = w + (size_t)(ok[i] ? n : 0) * K + lcol;
        }
    }
    __device__ __forceinline__ void load(int kt, float4 (&rb)[B_LD]) const
    {
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const float4 v = *reinterpret_cast<const float4 *>(ptr[i] + (size_t)kt * BK);
            rb[i] = ok[i] ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
};

// one K tile of fp32 MFMAs out of an LDS buffer of (64 MR + 64 NR) LDS_ROW-padded fp32 rows, A rows first: the permuted-K order of
// the design note above
template <int MR, int NR>
__device__ __forceinline__ void mfma_ktile_f32(const float *buf, const WaveGeom &g, floatx16 (&acc)[MR][NR])
{
    const float *sa = buf + (g.wm * 32 * MR + g.li) * LDS_ROW + g.lg * 4;
    const float *sb = buf + 64 * MR * LDS_ROW + (g.wn * 32 * NR + g.li) * LDS_ROW + g.lg * 4;
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
        float4 fa[MR], fb[NR];
#pragma unroll
        for (int i = 0; i < MR; ++i) fa[i] = *reinterpret_cast<const float4 *>(sa + i * 32 * LDS_ROW + kk * 8);
#pragma unroll
        for (int j = 0; j < NR; ++j) fb[j] = *reinterpret_cast<const float4 *>(sb + j * 32 * LDS_ROW + kk * 8);
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[j].x, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[j].y, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[j].z, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[j].w, acc[i][j], 0, 0, 0);
            }
    }
}

// C/D layout of the 32x32 MFMA: col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5).  Column of the wave's fragment
// (., j) and row of element e of its fragment (i, .) in a tile whose first row / column are m0 / n0:
template <int NR>
__device__ __forceinline__ int c_col(const WaveGeom &g, int n0, int j)
{
    return n0 + (g.wn * NR + j) * 32 + g.li;
}

template <int MR>
__device__ __forceinline__ int c_row(const WaveGeom &g, int m0, int i, int e)
{
    return m0 + (g.wm * MR + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * g.lg;
}

// f(row, col, value) for every element of the wave's fragments inside (row_limit, col_limit)
template <int MR, int NR, class F>
__device__ __forceinline__ void for_each_c(const floatx16 (&acc)[MR][NR], const WaveGeom &g, int m0, int n0, int row_limit,
                                           int col_limit, F f)
{
#pragma unroll
    for (int i = 0; i < MR; ++i) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int col = c_col<NR>(g, n0, j);
            if (col >= col_limit) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = c_row<MR>(g, m0, i, e);
                if (row >= row_limit) continue;
                f(row, col, acc[i][j][e]);
            }
        }
    }
}

// The forward kernels' epilogue, modes 0 and 1, on the wave's fragments (SCALED: times p.out_scale, the f16x3 engine's
// power-of-two rescale): split-K partial store, or bias (mode 1: modulo Cq), residual, ReLU, channel-offset store and the
// ConvTranspose2d pixel scatter.  One loop nest with the tests of split / mode inside, not for_each_c with a functor or a
// per-element function: only in this form does the compiler hoist those tests and the column's division of mode 1 out of the
// 16-element loop (through a functor: +13 % instructions in the 64x64 kernel, +18 % in the 128x128 one).
template <bool SCALED, int MR, int NR>
__device__ __forceinline__ void conv_epilogue(const ConvArgs &p, const floatx16 (&acc)[MR][NR], const WaveGeom &g, int m0, int n0)
{
    const bool split = gridDim.y > 1;
    const float os = p.out_scale;
#pragma unroll
    for (int i = 0; i < MR; ++i) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int col = c_col<NR>(g, n0, j);
            if (col >= p.Cout) continue;
            const float bv = (!split && p.bias) ? p.bias[p.mode == 1 ? col % (p.Cout >> 2) : col] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = c_row<MR>(g, m0, i, e);
                if (row >= p.M) continue;
                float v = SCALED ? acc[i][j][e] * os : acc[i][j][e];
                if (split) {
                    p.partial[((size_t)blockIdx.y * p.M + row) * p.Cout + col] = v;
                    continue;
                }
                v += bv;
                if (p.mode == 0) {
                    if (p.res) v += p.res[(size_t)row * p.rcs + col];
                    if (p.relu) v = fmaxf(v, 0.f);
                    p.y[(size_t)row * p.ycs + p.yco + col] = v;
                } else {   // ConvTranspose2d(k=2, s=2): col = (i2*2 + j2)*Cq + co
                    const int cq = p.Cout >> 2;
                    const int ij = col / cq, co = col - ij * cq;
                    const int ohw = p.OH * p.OW;
                    const int b = row / ohw, rem = row - b * ohw;
                    const int oh = rem / p.OW, ow = rem - oh * p.OW;
                    const size_t opix = ((size_t)b * 2 * p.OH + 2 * oh + (ij >> 1)) * (2 * p.OW) + 2 * ow + (ij & 1);
                    if (p.relu) v = fmaxf(v, 0.f);
                    p.y[opix * p.ycs + p.yco + co] = v;
                }
            }
        }
    }
}

// ---- host

// The largest 4-wave tile that still gives 512 workgroups (two per CU), no 128-wide N tile for N <= 64; else 64x64 and false
inline bool choose_tile_4w(int M, int N, int *mr, int *nr)
{
    static const int cand[4][2] = {{2, 2}, {2, 1}, {1, 2}, {1, 1}};
    for (auto &c : cand) {
        if (c[1] == 2 && N <= 64) continue;
        if ((long)cdiv(M, 64 * c[0]) * cdiv(N, 64 * c[1]) >= 512) {
            *mr = c[0];
            *nr = c[1];
            return true;
        }
    }
    *mr = *nr = 1;
    return false;
}

// f(MR, NR) with the tile as compile-time constants (std::integral_constant): the four instantiations of a 4-wave kernel
template <class F>
inline void dispatch_tile_4w(int mr, int nr, F f)
{
    using one = std::integral_constant<int, 1>;
    using two = std::integral_constant<int, 2>;
    if (mr == 2 && nr == 2) f(two{}, two{});
    else if (mr == 2) f(two{}, one{});
    else if (nr == 2) f(one{}, two{});
    else f(one{}, one{});
}

}  // namespace srcnn
