// ROIAlign arithmetic shared by the forward (roi_align.hip) and the backward (roi_align_backward.hip): the one statement of
// each piece whose rounding the tests pin bit by bit -- the roi's geometry and the tap location (roi_align_kernel.cu:33-62
// forward, :104-131 backward, the same expressions), the bilinear blend (:64-67), the ordered 2x2 average of
// RoIAlignAvg and its adjoint, max_pool2d's NaN rule, the pyramid's level table and the per-roi view of it.
// The library is built with -ffp-contract=off: every operation below is rounded on its own.
#pragma once
#include <hip/hip_runtime.h>

namespace srcnn {

struct RoiGeom {
    float start_w, start_h, bin_w, bin_h;
    int batch;
};

__device__ __forceinline__ RoiGeom roi_geom(const float *r, float scale, int ah, int aw)
{
    RoiGeom g;
    g.batch = (int)r[0];
    g.start_w = r[1] * scale;
    g.start_h = r[2] * scale;
    float end_w = r[3] * scale;
    float end_h = r[4] * scale;
    float roi_w = fmaxf((float)((double)(end_w - g.start_w) + 1.), 0.0f);   // roi_align_kernel.cu:40
    float roi_h = fmaxf((float)((double)(end_h - g.start_h) + 1.), 0.0f);   // :41
    g.bin_h = (float)((double)roi_h / ((double)ah - 1.));                   // :42
    g.bin_w = (float)((double)roi_w / ((double)aw - 1.));                   // :43
    return g;
}

// One axis of a lattice point at coordinate v on a map of `size` pixels: false when the point lies outside the map
// (:54-55); otherwise `start` is the first of its two taps (clamped so that start + 1 stays inside, :48-49) and `ratio`
// the weight of the second one.  (Outside the map `start` may lie anywhere: a caller that loads before it tests guards it.)
__device__ __forceinline__ bool lattice_axis(float v, int size, int &start, float &ratio)
{
    start = (int)fminf(floorf(v), (float)(size - 2));
    ratio = v - (float)start;
    return !(v < 0 || v >= size);
}

// Value of one lattice point from its four taps (upper/lower, left/right).  :64-67 with C++'s usual arithmetic conversions,
// left to right: `1.` is a double, so the first two terms are double products; `down * h_ratio` is float x float (rounded
// to float) before it meets a double, and the last term is a float product throughout; the double sum is narrowed once.
// (Checked against the reference's own kernel built for gfx950: tests/test_ref_kernels_gpu.py.)
__device__ __forceinline__ float lattice_blend(float ul, float ur, float dl, float dr, float h_ratio, float w_ratio)
{
    const double hr1 = 1. - (double)h_ratio, wr1 = 1. - (double)w_ratio;
    const float dl_h = dl * h_ratio;
    const float dr_hw = dr * h_ratio * w_ratio;
    const double v = (double)ul * hr1 * wr1 + (double)ur * hr1 * (double)w_ratio + (double)dl_h * wr1 + (double)dr_hw;
    return (float)v;
}

// avg_pool2d(2, stride 1) of RoIAlignAvg (modules/roi_align.py:26-29) over the window (a b / c d): ATen's sum order
// (row-major), x 0.25.
__device__ __forceinline__ float avg2x2(float a, float b, float c, float d) { return (((a + b) + c) + d) * 0.25f; }

// Adjoint of a 2x2 / stride-1 window over an oh x ow output, for lattice point (i, j): the up to four outputs that read it,
// in row-major order, the first one assigned to s and the rest added (s stays as it is when there is none).
// `load(oy, ox)` returns the gradient of output (oy, ox) as a struct of N floats `v`; `keep(oy, ox)` is false for an output
// that did not take its value from this point (the maximum).  average: x 0.25f, the adjoint of avg2x2.
template <int N, typename Load, typename Keep>
__device__ __forceinline__ void window2x2_adjoint(float (&s)[N], int i, int j, int oh, int ow, bool average, Load load, Keep keep)
{
    bool first = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int oy = i - 1 + (q >> 1), ox = j - 1 + (q & 1);
        if (oy < 0 || oy >= oh || ox < 0 || ox >= ow || !keep(oy, ox)) continue;
        const auto t = load(oy, ox);
#pragma unroll
        for (int e = 0; e < N; ++e) s[e] = first ? t.v[e] : s[e] + t.v[e];
        first = false;
    }
    if (average) {
#pragma unroll
        for (int e = 0; e < N; ++e) s[e] = s[e] * 0.25f;
    }
}

// The element max_pool2d(2, stride 1) picks from the window (v0 v1 / v2 v3): the first maximum in row-major order, and a
// NaN wins (max_pool2d propagates NaN; fmaxf would drop it).
struct Max4 {
    float value;
    int index;
};

__device__ __forceinline__ Max4 first_max4(float v0, float v1, float v2, float v3)
{
    Max4 m = {v0, 0};
    if (v1 > m.value || v1 != v1) m = {v1, 1};
    if (v2 > m.value || v2 != v2) m = {v2, 2};
    if (v3 > m.value || v3 != v3) m = {v3, 3};
    return m;
}

// pyramid level (0..3 = P2..P5) of a roi, stereo_rcnn.py:113-119 (natural log; round half away from zero; clamp 2..5)
__device__ __forceinline__ int pyramid_level(const float *r)
{
    float bh = r[4] - r[2] + 1.0f;
    float bw = r[3] - r[1] + 1.0f;
    float lv = logf(sqrtf(bh * bw) / 224.0f) + 4.0f;
    lv = copysignf(floorf(fabsf(lv) + 0.5f), lv);
    lv = fminf(fmaxf(lv, 2.0f), 5.0f);
    return (int)lv - 2;
}

// The pyramid's four maps as the kernels see them (passed by value inside their argument structs).
struct RoiLevels {
    int mh[4], mw[4];
    float scale[4];
    const int *roi_limit;        // device-side count of the rois that matter (blocks of later rois exit), or nullptr
};

inline RoiLevels roi_levels(const int *mh_host, const int *mw_host, float im_height, const int *roi_limit)
{
    RoiLevels lv;
    lv.roi_limit = roi_limit;
    for (int l = 0; l < 4; ++l) {
        lv.mh[l] = mh_host[l];
        lv.mw[l] = mw_host[l];
        // python: feat_maps[i].size(2) / im_info[0][0] -> double, narrowed to float at the C boundary
        lv.scale[l] = (float)((double)mh_host[l] / (double)im_height);
    }
    return lv;
}

// What a forward workgroup knows about its roi n: the level it is routed to, that level's map and the (A + 1)^2 lattice.
struct RoiView {
    int l, height, width;
    RoiGeom geo;
    const float *base;           // the level's map
    size_t img;                  // first pixel of the roi's image in it
};

__device__ __forceinline__ RoiView roi_view(const RoiLevels &lv, const float *const *maps, const float *rois, int n, int A)
{
    const float *r = rois + (size_t)n * 5;
    RoiView v;
    v.l = __builtin_amdgcn_readfirstlane(pyramid_level(r));      // same roi for the whole block
    v.height = lv.mh[v.l], v.width = lv.mw[v.l];
    v.geo = roi_geom(r, lv.scale[v.l], A + 1, A + 1);
    v.base = maps[v.l];
    v.img = (size_t)v.geo.batch * v.height * v.width;
    return v;
}

}  // namespace srcnn
