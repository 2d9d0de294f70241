// What the training-side 3 x f16 calls share (conv_backward_f16x3.hip: dgrad and wgrad; conv_forward_f16x3.hip: the forward): the
// device-found power-of-two scale of a tensor, the split of a scaled fp32 value into two halves, one K tile of the
// three-product MFMA loop, and the staging + K loop of the tile that the forward and dgrad have in common (fp32 A split on the way
// into LDS, prepared f16 B planes: F16PlaneRows, f16x3_store_a, f16x3_scaled_kloop).  One copy, so that the forward and the
// backward round alike.  include/srcnn_hip.h states the scheme.
#pragma once
#include "conv_tile_4w.h"
#include <cstdint>

namespace srcnn {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

constexpr int HROW = BK;           // halves per LDS row (64 B; 16-byte chunks XOR-swizzled with (row >> 2) & 3)
constexpr int F16X3_TOP = 14;      // a tensor's largest |element| is scaled into [2^14, 2^15): below f16's 65504 after rounding

struct Pow2 {
    float s, inv;
};

// s = 2^(TOP - floor(log2 max)) and 1 / s, exponent clamped to +-126 so that both are normal floats; a zero (or subnormal) max
// gives the clamp
__device__ __forceinline__ Pow2 pow2_scale(unsigned maxbits)
{
    const int e = (int)(maxbits >> 23) - 127;
    const int sh = min(max(F16X3_TOP - e, -126), 126);
    Pow2 r;
    r.s = __uint_as_float((unsigned)(127 + sh) << 23);
    r.inv = __uint_as_float((unsigned)(127 - sh) << 23);
    return r;
}

__device__ __forceinline__ void split_f16(float v, float s, _Float16 &hi, _Float16 &lo)
{
    const float t = v * s;              // exact: a power of two
    hi = (_Float16)t;                   // round to nearest even
    lo = (_Float16)(t - (float)hi);     // the residual is exact in fp32
}

// the call's four max words in the workspace <- 0, and `extra`, one word of the caller's that the call will overwrite with a
// maximum; either may be null
static __global__ void f16x3_clear_scales(unsigned *amax, unsigned *extra)
{
    if (threadIdx.x < 4 && amax) amax[threadIdx.x] = 0u;
    if (threadIdx.x == 4 && extra) *extra = 0u;
}

// The *_prepared entries' clear: the same words, except that the max|w| word (amax[1] in the forward's and the backward's
// layout alike) takes the bits srcnn_train_weights_prepare left in *wmax -- the GEMM kernels go on reading s_w from the workspace
// and stay as they are.  wmax may be null (a backward without dx reads no weights): the word is cleared.
static __global__ void f16x3_clear_scales_prepared(unsigned *amax, unsigned *extra, const unsigned *wmax)
{
    if (threadIdx.x < 4) amax[threadIdx.x] = (threadIdx.x == 1 && wmax) ? *wmax : 0u;
    if (threadIdx.x == 4 && extra) *extra = 0u;
}

// The *_prepared entries' three arguments: the layer's max word and its plane pair, each plane `need` bytes at least
static int check_prepared_planes(const char *who, const unsigned *w_amax, const void *hi, const void *lo, size_t plane_bytes, size_t need)
{
    SRCNN_REQUIRE_AS(who, w_amax != nullptr, "null pointer: w_amax");
    SRCNN_REQUIRE_AS(who, hi != nullptr && lo != nullptr, "null pointer: a prepared plane");
    SRCNN_REQUIRE_AS(who, (reinterpret_cast<uintptr_t>(w_amax) & 3) == 0, "w_amax must be 4-byte aligned");
    SRCNN_REQUIRE_AS(who, ((reinterpret_cast<uintptr_t>(hi) | reinterpret_cast<uintptr_t>(lo)) & 15) == 0,
                     "the prepared planes must be 16-byte aligned (vector loads)");
    SRCNN_REQUIRE_AS(who, plane_bytes >= need, "plane_bytes: a prepared plane holds Cp KH KW Cin halves");
    return SRCNN_OK;
}

// max |v| over `rows` rows of `len` floats at a stride of `stride` floats.  VEC: len, stride multiples of 4 and a 16-byte aligned base
template <bool VEC>
__global__ __launch_bounds__(256) void absmax_kernel(const float *v, long long rows, int len, long long stride, unsigned *word)
{
    const int per_row = VEC ? len / 4 : len;
    const long long total = rows * per_row;
    float mx = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / per_row;
        const float *ptr = v + r * stride + (i - r * per_row) * (VEC ? 4 : 1);
        if (VEC) {
            const float4 f = *reinterpret_cast<const float4 *>(ptr);
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(f.x), fabsf(f.y))), fmaxf(fabsf(f.z), fabsf(f.w)));
        } else {
            mx = fmaxf(mx, fabsf(*ptr));
        }
    }
    wave_absmax_to_word(mx, word);
}

static void launch_absmax(const float *v, long long rows, int len, long long stride, unsigned *word, hipStream_t st)
{
    const bool vec = (reinterpret_cast<uintptr_t>(v) & 15) == 0 && len % 4 == 0 && stride % 4 == 0;
    const long long total = rows * (vec ? len / 4 : len);
    const unsigned blocks = (unsigned)min(1024LL, (total + 255) / 256);
    if (vec) SRCNN_LAUNCH(absmax_kernel<true>, dim3(blocks), dim3(256), 0, st, v, rows, len, stride, word);
    else SRCNN_LAUNCH(absmax_kernel<false>, dim3(blocks), dim3(256), 0, st, v, rows, len, stride, word);
}

// The caller-owned max words of the *_maxima entries (either may be null): 4-byte aligned, and never the same word -- the call's
// clear of y_amax would destroy x_amax before the GEMM reads it
static int check_amax_words(const unsigned *x_amax, const unsigned *y_amax)
{
    SRCNN_REQUIRE((reinterpret_cast<uintptr_t>(x_amax) & 3) == 0, "x_amax must be 4-byte aligned");
    SRCNN_REQUIRE((reinterpret_cast<uintptr_t>(y_amax) & 3) == 0, "y_amax must be 4-byte aligned");
    SRCNN_REQUIRE(x_amax == nullptr || x_amax != y_amax, "x_amax and y_amax alias: they must be two words");
    return SRCNN_OK;
}

// One K tile out of an LDS buffer of four panels [A_hi | A_lo | B_hi | B_lo] of swizzled 64-byte rows (conv_f16x3_kernel's layout):
// two MFMA steps; the cross terms go into accx, hi hi into acc, so consecutive MFMAs never share an accumulator.
template <int MR, int NR>
__device__ __forceinline__ void f16x3_ktile(const _Float16 *buf, const WaveGeom &g, floatx16 (&acc)[MR][NR], floatx16 (&accx)[MR][NR])
{
    constexpr int PANEL_A = 64 * MR * HROW, PANEL_B = 64 * NR * HROW;
    const int r_sw = (g.lg ^ ((g.li >> 2) & 3)) << 3;     // chunk kk * 2 + lg swizzled; kk = 1 flips bit 4 (halves)
    const _Float16 *sah = buf + (g.wm * 32 * MR + g.li) * HROW + r_sw;
    const _Float16 *sal = sah + PANEL_A;
    const _Float16 *sbh = buf + 2 * PANEL_A + (g.wn * 32 * NR + g.li) * HROW + r_sw;
    const _Float16 *sbl = sbh + PANEL_B;
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
        const int ko = kk ? ((r_sw ^ 16) - r_sw) : 0;
        half8 ah[MR], al[MR], bh[NR], bl[NR];
#pragma unroll
        for (int i = 0; i < MR; ++i) {
            ah[i] = *reinterpret_cast<const half8 *>(sah + i * 32 * HROW + ko);
            al[i] = *reinterpret_cast<const half8 *>(sal + i * 32 * HROW + ko);
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            bh[j] = *reinterpret_cast<const half8 *>(sbh + j * 32 * HROW + ko);
            bl[j] = *reinterpret_cast<const half8 *>(sbl + j * 32 * HROW + ko);
        }
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                accx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], accx[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                accx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], accx[i][j], 0, 0, 0);
            }
    }
}

// halves in one such buffer
constexpr int f16x3_buf_halves(int mr, int nr) { return 2 * 64 * (mr + nr) * HROW; }

// ---- The tile of conv_fwd_f16x3_kernel and conv_dgrad_f16x3_kernel: A is gathered as fp32 and split with its tensor's scale on the
// way into LDS, B comes from prepared hi / lo f16 planes of K-contiguous rows.

// B side: the thread's B_LD rows n0 + (t >> 2) + 64 i of the two planes (rows of K halves; rows beyond `rows` read as zeros), one
// 16-byte chunk of each per K tile
template <int B_LD>
struct F16PlaneRows {
    const _Float16 *hi[B_LD], *lo[B_LD];
    bool ok[B_LD];
    int brow, sw;
    uint4 rh[B_LD], rl[B_LD];
    __device__ __forceinline__ F16PlaneRows(const _Float16 *hi_plane, const _Float16 *lo_plane, int n0, int rows, size_t K)
    {
        const int t = threadIdx.x, bcol = (t & 3) * 8;
        brow = t >> 2;
        sw = ((t & 3) ^ ((brow >> 2) & 3)) << 3;
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const int n = n0 + brow + 64 * i;
            ok[i] = n < rows;
            const size_t off = (size_t)(ok[i] ? n : 0) * K + bcol;
            hi[i] = hi_plane + off;
            lo[i] = lo_plane + off;
        }
    }
    __device__ __forceinline__ void load(int kt)
    {
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const uint4 vh = *reinterpret_cast<const uint4 *>(hi[i] + (size_t)kt * BK);
            const uint4 vl = *reinterpret_cast<const uint4 *>(lo[i] + (size_t)kt * BK);
            rh[i] = ok[i] ? vh : make_uint4(0, 0, 0, 0);
            rl[i] = ok[i] ? vl : make_uint4(0, 0, 0, 0);
        }
    }
    // registers -> the B_hi / B_lo panels
    __device__ __forceinline__ void store(_Float16 *b_hi, _Float16 *b_lo) const
    {
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const int o = (brow + 64 * i) * HROW + sw;
            *reinterpret_cast<uint4 *>(b_hi + o) = rh[i];
            *reinterpret_cast<uint4 *>(b_lo + o) = rl[i];
        }
    }
};

__device__ __forceinline__ void split_f16x4(const float4 &f, float s, half4 &hi, half4 &lo)
{
    const float v[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        _Float16 h, l;
        split_f16(v[e], s, h, l);
        hi[e] = h;
        lo[e] = l;
    }
}

// A store: the thread's float4 ra[i] of row lrow + 32 i, floats lcol .. lcol + 3 (lcol a multiple of 4), split with s into the
// A_hi / A_lo panels
template <int A_LD>
__device__ __forceinline__ void f16x3_store_a(const float4 (&ra)[A_LD], int lrow, int lcol, float s, _Float16 *a_hi, _Float16 *a_lo)
{
    const int sw = (((lcol >> 3) ^ ((lrow >> 2) & 3)) << 3) + (lcol & 4);
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
        half4 hi, lo;
        split_f16x4(ra[i], s, hi, lo);
        const int o = (lrow + 32 * i) * HROW + sw;
        *reinterpret_cast<half4 *>(a_hi + o) = hi;
        *reinterpret_cast<half4 *>(a_lo + o) = lo;
    }
}

// The tile's whole K loop into zeroed accumulators.  K tile kt is channels [32 c, 32 c + 32) of tap (kh, kw), kt = (kh KW + kw) ctiles + c;
// a.load(i, kh, kw, channel) is the gather (OutPixelGather, InPixelGather), built by the kernel for the same (lrow, lcol) = (t >> 3,
// (t & 7) * 4) it passes here -- row lrow + 32 i, floats lcol .. lcol + 3 of the tile's A rows -- and s_a its tensor's scale; the
// planes have nkt * 32 halves per row.  smem: two buffers of f16x3_buf_halves(MR, NR).
template <int MR, int NR, class Gather>
__device__ __forceinline__ void f16x3_scaled_kloop(_Float16 *smem, const Gather &a, int lrow, int lcol, float s_a, const _Float16 *b_hi,
                                                   const _Float16 *b_lo, int n0, int b_rows, int ctiles, int KW, int nkt, const WaveGeom &g,
                                                   floatx16 (&acc)[MR][NR], floatx16 (&accx)[MR][NR])
{
    constexpr int A_LD = 2 * MR, PANEL_A = 64 * MR * HROW, PANEL_B = 64 * NR * HROW, BUF = f16x3_buf_halves(MR, NR);
    F16PlaneRows<NR> b(b_hi, b_lo, n0, b_rows, (size_t)nkt * BK);
    float4 ra[A_LD];
    zero_acc(acc);
    zero_acc(accx);
    ktile_pipeline(
        0, nkt,
        [&](int kt) {
            const int tap = kt / ctiles;
            const int c0 = (kt - tap * ctiles) * BK;
            const int kh = tap / KW;
            const int kw = tap - kh * KW;
#pragma unroll
            for (int i = 0; i < A_LD; ++i) ra[i] = a.load(i, kh, kw, c0 + lcol);
            b.load(kt);
        },
        [&](int buf) {
            _Float16 *s = smem + buf * BUF;
            f16x3_store_a(ra, lrow, lcol, s_a, s, s + PANEL_A);
            b.store(s + 2 * PANEL_A, s + 2 * PANEL_A + PANEL_B);
        },
        [&](int buf) { f16x3_ktile(smem + buf * BUF, g, acc, accx); });
}

}  // namespace srcnn
