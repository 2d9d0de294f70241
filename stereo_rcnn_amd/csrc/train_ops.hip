// Training: the adjoints the conv / ROIAlign / loss backward kernels leave open -- the FPN top-down step (_upsample_add), the
// P6 subsample (MaxPool2d(1, stride 2)) and the layout step of ConvTranspose2d(k = 2, s = 2) (conv mode 1).
// All are one-pass HBM-bound NHWC float32 kernels on 8-channel groups (float4 loads and stores, coalesced over C), without
// atomics: every output element is owned by one thread and stored once, so no output needs a zero fill and every result is
// run-to-run bit-equal.  include/srcnn_hip.h ("training: remaining adjoints") states the sums and their order.
#include "bilinear_tap.h"

namespace srcnn {

// Output indices that can read top index t: those with i1 in {t - 1, t}, i.e. r * o in [t - 1, t + 1); one index of slack on
// each side, the caller recomputes every candidate's taps the forward's way.  r == 0: every output index reads top index 0.
__device__ __forceinline__ void up_candidates(float r, int t, int n_out, int &lo, int &hi)
{
    if (r == 0.f) {
        lo = 0;
        hi = n_out - 1;
        return;
    }
    const float a = floorf((float)(t - 1) / r) - 1.f, b = ceilf((float)(t + 1) / r) + 1.f;
    lo = a < 0.f ? 0 : (int)a;
    hi = b > (float)(n_out - 1) ? n_out - 1 : (int)b;
}

// d_top[b, th, tw, :] = sum over the forward's taps that read top pixel (th, tw).  grid (ceil(TW * C/8 / 256), B * TH): one
// top row per blockIdx.y, so the candidate rows and their vertical weights are wave-uniform.
__global__ void upsample_add_backward_kernel(const float *__restrict__ dy, int H, int W, int C, float *__restrict__ d_top,
                                             int TH, int TW)
{
    const float rh = align_ratio(TH, H), rw = align_ratio(TW, W);
    const int G = C / 8;
    const int row = blockIdx.y;                      // b * TH + th
    const int b = row / TH, th = row - b * TH;
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (unsigned)(TW * G)) return;
    const int tw = (int)(idx / (unsigned)G), g = (int)(idx - (unsigned)tw * (unsigned)G);
    int hlo, hhi, wlo, whi;
    up_candidates(rh, th, H, hlo, hhi);
    up_candidates(rw, tw, W, wlo, whi);
    float8 acc;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc.v[e] = 0.f;
    for (int h = hlo; h <= hhi; ++h) {
        const UpTap ht = align_tap(rh, h, TH);
        // the forward's two row taps (ht.i1 with ht.l0, ht.i1 + ht.i1p with ht.l1); at the last top row both are the same row
        const bool r0 = ht.i1 == th, r1 = ht.i1 + ht.i1p == th;
        if (!r0 && !r1) continue;
        for (int w = wlo; w <= whi; ++w) {
            const UpTap wt = align_tap(rw, w, TW);
            const bool c0 = wt.i1 == tw, c1 = wt.i1 + wt.i1p == tw;
            if (!c0 && !c1) continue;
            const float8 v = act_load8(dy, 0, ((size_t)b * H + h) * W + w, C, g);
            // align_blend's tap order, (row, column) weights: (l0, l0) (l0, l1) (l1, l0) (l1, l1); each coefficient rounded once
            const float hl[2] = {ht.l0, ht.l1}, wl[2] = {wt.l0, wt.l1};
            const bool rr[2] = {r0, r1}, cc[2] = {c0, c1};
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (rr[i] && cc[j]) {
                        const float k = hl[i] * wl[j];
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc.v[e] = fmaf(k, v.v[e], acc.v[e]);
                    }
        }
    }
    act_store8(d_top, 0, (size_t)row * TW + tw, C, g, acc);
}

// dx[b, 2i, 2j, :] = dy[b, i, j, :], zeros elsewhere
__global__ void subsample2_backward_kernel(const float4 *__restrict__ dy, int B, int OH, int OW, int C4, float4 *__restrict__ dx,
                                           int H, int W)
{
    const size_t total = (size_t)B * H * W * C4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        const auto [b, h, w, c] = nhwc_split(idx, H, W, C4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (((h | w) & 1) == 0) v = dy[(((size_t)b * OH + (h >> 1)) * OW + (w >> 1)) * C4 + c];
        dx[idx] = v;
    }
}

// packed (M, h, w, 4 Cq) ordered (i, j, co)  <->  wide (M, 2h, 2w, Cq): wide[m, 2a + i, 2b + j, co] = packed[m, a, b, (2i + j) Cq + co].
// One thread per float4 of the wide tensor in either direction.
__global__ void pixel_shuffle2_kernel(const float4 *__restrict__ x, int M, int h, int w, int C4, float4 *__restrict__ y, int inverse)
{
    const int W2 = 2 * w, H2 = 2 * h;
    const size_t total = (size_t)M * H2 * W2 * C4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        const auto [m, Y, X, c] = nhwc_split(idx, H2, W2, C4);
        const size_t packed = ((((size_t)m * h + (Y >> 1)) * w + (X >> 1)) * 4 + (size_t)((Y & 1) * 2 + (X & 1))) * C4 + c;
        if (inverse) y[packed] = x[idx];
        else y[idx] = x[packed];
    }
}

}  // namespace srcnn

extern "C" {

int srcnn_upsample_add_backward(const float *dy, int B, int H, int W, int C, float *d_top, int TH, int TW, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(dy != nullptr, "null pointer: dy");
    SRCNN_REQUIRE(d_top != nullptr, "null pointer: d_top");
    SRCNN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && TH > 0 && TW > 0, "bad shape: sizes must be positive");
    SRCNN_REQUIRE(H >= TH && W >= TW, "bad shape: the output map must be at least as large as top (H >= TH, W >= TW)");
    SRCNN_REQUIRE(C % 8 == 0, "bad channel stride: C must be a multiple of 8");
    SRCNN_REQUIRE(aligned16(dy) && aligned16(d_top), "dy and d_top must be 16-byte aligned");
    SRCNN_REQUIRE((long long)B * TH <= 65535 && (long long)TW * (C / 8) < (1LL << 31) && (long long)H < (1 << 24) &&
                  (long long)W < (1 << 24), "bad shape: map too large");
    SRCNN_LAUNCH(upsample_add_backward_kernel, dim3((TW * (C / 8) + 255) / 256, B * TH), dim3(256), 0, as_stream(stream), dy, H, W,
                 C, d_top, TH, TW);
    return check_launch("srcnn_upsample_add_backward");
}

int srcnn_subsample2_backward(const float *dy, int B, int OH, int OW, int C, float *dx, int H, int W, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(dy != nullptr, "null pointer: dy");
    SRCNN_REQUIRE(dx != nullptr, "null pointer: dx");
    SRCNN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && OH > 0 && OW > 0, "bad shape: sizes must be positive");
    SRCNN_REQUIRE(OH == (H + 1) / 2 && OW == (W + 1) / 2, "bad shape: OH, OW must be ceil(H / 2), ceil(W / 2)");
    SRCNN_REQUIRE(C % 8 == 0, "bad channel stride: C must be a multiple of 8");
    SRCNN_REQUIRE(aligned16(dy) && aligned16(dx), "dy and dx must be 16-byte aligned");
    const size_t total = (size_t)B * H * W * (C / 4);
    SRCNN_LAUNCH(subsample2_backward_kernel, dim3(grid_for(total, 256, 16384)), dim3(256), 0, as_stream(stream),
                 reinterpret_cast<const float4 *>(dy), B, OH, OW, C / 4, reinterpret_cast<float4 *>(dx), H, W);
    return check_launch("srcnn_subsample2_backward");
}

int srcnn_pixel_shuffle2(const float *x, int M, int h, int w, int Cq, float *y, int inverse, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(x != nullptr, "null pointer: x");
    SRCNN_REQUIRE(y != nullptr, "null pointer: y");
    SRCNN_REQUIRE(M > 0 && h > 0 && w > 0 && Cq > 0, "bad shape: sizes must be positive");
    SRCNN_REQUIRE((unsigned)inverse <= 1, "bad shape: inverse must be 0 or 1");
    SRCNN_REQUIRE(Cq % 8 == 0, "bad channel stride: Cq must be a multiple of 8");
    SRCNN_REQUIRE(aligned16(x) && aligned16(y), "x and y must be 16-byte aligned");
    SRCNN_REQUIRE((long long)h < (1 << 20) && (long long)w < (1 << 20), "bad shape: map too large");
    const size_t total = (size_t)M * h * w * Cq;      // float4s of either tensor: M * 2h * 2w * Cq / 4
    SRCNN_LAUNCH(pixel_shuffle2_kernel, dim3(grid_for(total, 256, 16384)), dim3(256), 0, as_stream(stream),
                 reinterpret_cast<const float4 *>(x), M, h, w, Cq / 4, reinterpret_cast<float4 *>(y), inverse);
    return check_launch("srcnn_pixel_shuffle2");
}

}  // extern "C"
