// The image preparation both preprocessing files share (pool_resize.hip: srcnn_preprocess; loader.hip: srcnn_preprocess_train).
// Every file that includes this header is built with -ffp-contract=off: each product and sum below rounds to float32 on its own.
//
// A0 (demo.py:103-129, blob.py:39-64): uint8 RGB (H, W, 3) -> float32 BGR, minus PIXEL_MEANS, resized by
// cv2.resize(img, None, None, fx=s, fy=s, INTER_LINEAR).  The resize follows OpenCV's published float path operation by
// operation (modules/imgproc/src/resize.cpp; restated and pinned in oracle/preprocess.py): tap position
// (float)((d + 0.5) * (1/s) - 0.5) in double then float, cvFloor, float fraction; horizontal taps clamp AND zero the
// fraction at the borders, vertical taps clip the two rows but keep the fraction; HResizeLinear S[sx]*a0 + S[sx+1]*a1,
// VResizeLinear S0*b0 + S1*b1, each product and sum rounded to float32 on its own.  Mean subtraction happens BEFORE the
// resize and in double, as numpy does for float32 -= float64.
// (bilinear_tap.h is another rule -- torch's align_corners=True: corner-aligned ratio, no half-pixel offset -- and stays apart.)
#pragma once
#include <hip/hip_runtime.h>

namespace srcnn {

struct ResizeTap {
    int s0, s1;
    float w0, w1;
    bool copy;     // horizontal only: dx >= xmax, D = S[cols-1] * 1.f
};

__device__ __forceinline__ ResizeTap resize_tap(int d, int n_src, double step, bool horizontal)
{
    ResizeTap t;
    float f = (float)(((double)d + 0.5) * step - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    t.copy = false;
    if (horizontal) {
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= n_src - 1) { s = n_src - 1; f = 0.f; t.copy = true; }
        t.s0 = s;
        t.s1 = min(s + 1, n_src - 1);
    } else {
        t.s0 = min(max(s, 0), n_src - 1);
        t.s1 = min(max(s + 1, 0), n_src - 1);
    }
    t.w1 = f;
    t.w0 = 1.f - f;
    return t;
}

__device__ __forceinline__ float u8_minus_mean(unsigned char v, double mean) { return (float)((double)v - mean); }

__device__ __forceinline__ double pixel_mean_bgr(int c)        // PIXEL_MEANS (config.py:170), BGR
{
    return c == 0 ? 102.9801 : (c == 1 ? 115.9465 : 122.7717);
}

// resized value of output channel c (0, 1, 2 = B, G, R <- input channel 2 - c) at the taps (tx, ty).  mirror: the source is
// read flipped left to right, column s of the flipped image being column W - 1 - s of `img` (minibatch.py:116-119 flips
// before the mean and the resize).
__device__ __forceinline__ float preprocess_channel(const unsigned char *__restrict__ img, int W, const ResizeTap &tx,
                                                    const ResizeTap &ty, int c, bool mirror)
{
    const int x0 = mirror ? W - 1 - tx.s0 : tx.s0, x1 = mirror ? W - 1 - tx.s1 : tx.s1;
    const unsigned char *r0 = img + (size_t)ty.s0 * W * 3, *r1 = img + (size_t)ty.s1 * W * 3;
    const int ic = 2 - c;
    const double mean = pixel_mean_bgr(c);
    const float a = u8_minus_mean(r0[x0 * 3 + ic], mean), b = u8_minus_mean(r0[x1 * 3 + ic], mean);
    const float cc = u8_minus_mean(r1[x0 * 3 + ic], mean), d = u8_minus_mean(r1[x1 * 3 + ic], mean);
    const float h0 = tx.copy ? a : a * tx.w0 + b * tx.w1;
    const float h1 = tx.copy ? cc : cc * tx.w0 + d * tx.w1;
    return h0 * ty.w0 + h1 * ty.w1;
}

// resized BGR value of output pixel (oy, ox): bgr[0..2]
__device__ __forceinline__ void preprocess_pixel(const unsigned char *__restrict__ img, int H, int W, int oy, int ox,
                                                 double step, float bgr[3])
{
    const ResizeTap tx = resize_tap(ox, W, step, true), ty = resize_tap(oy, H, step, false);
#pragma unroll
    for (int c = 0; c < 3; ++c) bgr[c] = preprocess_channel(img, W, tx, ty, c, false);
}

}  // namespace srcnn
