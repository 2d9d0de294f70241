// ROIAlign geometry shared by the forward (roi_align.hip) and the backward (roi_align_backward.hip): one statement of the
// reference's float/double promotion pattern (roi_align_kernel.cu:33-62 forward, :104-131 backward -- the same expressions).
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
// the weight of the second one.
__device__ __forceinline__ bool lattice_axis(float v, int size, int &start, float &ratio)
{
    start = (int)fminf(floorf(v), (float)(size - 2));
    ratio = v - (float)start;
    return !(v < 0 || v >= size);
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

}  // namespace srcnn
