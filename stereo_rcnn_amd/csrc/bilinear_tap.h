// The align_corners=True bilinear tap (torch-0.3 F.upsample, ATen's upsample_bilinear2d: area_pixel_compute_scale =
// (in - 1) / (out - 1); i1 = (int)(r * o); lambda = r * o - i1) and its blend.  Callers: upsample_add_kernel (pool_resize.hip),
// its adjoint upsample_add_backward_kernel (train_ops.hip) and upsample2x_at (dense_align.hip).
// TWO SITES RESTATE THIS TEXT BY HAND and must be edited with it, because calling the header moved the instruction stream of a
// kernel that must not move (profiles/nhwc_helpers_ab.txt):
//   * the fused up_top epilogue of conv_f16s_body.inc -- ratio, tap and blend written out;
//   * upsample2x_kernel (dense_align.hip) -- the two ratio lines, without align_ratio's n_out > 1 guard.
// Every caller is built with -ffp-contract=off: each operation below rounds on its own.
// (resize_tap.h is another rule -- OpenCV's INTER_LINEAR: half-pixel centres, clamped taps -- and stays apart.)
#pragma once
#include "conv_common.h"

namespace srcnn {

// source index and weights of output index o: taps i1 (weight l0) and i1 + i1p (weight l1)
struct UpTap {
    int i1, i1p;
    float l0, l1;
};

__device__ __forceinline__ float align_ratio(int n_src, int n_out) { return n_out > 1 ? (float)(n_src - 1) / (float)(n_out - 1) : 0.f; }

__device__ __forceinline__ UpTap align_tap(float r, int o, int n_src)
{
    UpTap t;
    const float f = r * (float)o;
    t.i1 = (int)f;
    t.i1p = (t.i1 < n_src - 1) ? 1 : 0;
    t.l1 = f - (float)t.i1;
    t.l0 = 1.f - t.l1;
    return t;
}

// a, b: row ht.i1 at columns wt.i1, wt.i1 + wt.i1p; c, d: the same columns of row ht.i1 + ht.i1p
__device__ __forceinline__ float align_blend(const UpTap &ht, const UpTap &wt, float a, float b, float c, float d)
{
    return ht.l0 * (wt.l0 * a + wt.l1 * b) + ht.l1 * (wt.l0 * c + wt.l1 * d);
}

__device__ __forceinline__ float8 align_blend(const UpTap &ht, const UpTap &wt, const float8 &a, const float8 &b, const float8 &c,
                                              const float8 &d)
{
    float8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = align_blend(ht, wt, a.v[e], b.v[e], c.v[e], d.v[e]);
    return o;
}

}  // namespace srcnn
