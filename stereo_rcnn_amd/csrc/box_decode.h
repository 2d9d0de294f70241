// bbox_transform_inv of one box followed by clip_boxes.  Called by the proposal layer (rpn_proposal.hip); the detection decode
// (heads.hip:decode_clip) restates it by hand, for the reason given there.
#pragma once

namespace srcnn {

// Box (x1, y1, x2, y2) moved by the deltas (dx, dy, dw, dh) and clipped to [0, wmax] x [0, hmax] into o[0..3].
__device__ __forceinline__ void decode_clip_box(const float x1, const float y1, const float x2, const float y2, float dx, float dy,
                                                float dw, float dh, float wmax, float hmax, float *o)
{
    // bbox_transform.py:81-104, float32, one rounding per operation (no contraction)
    const float widths = x2 - x1 + 1.0f;
    const float heights = y2 - y1 + 1.0f;
    const float ctr_x = x1 + 0.5f * widths;
    const float ctr_y = y1 + 0.5f * heights;
    const float pcx = dx * widths + ctr_x;
    const float pcy = dy * heights + ctr_y;
    const float pw = expf(dw) * widths;
    const float ph = expf(dh) * heights;
    o[0] = fminf(fmaxf(pcx - 0.5f * pw, 0.f), wmax);   // clip_boxes :177-185
    o[1] = fminf(fmaxf(pcy - 0.5f * ph, 0.f), hmax);
    o[2] = fminf(fmaxf(pcx + 0.5f * pw, 0.f), wmax);
    o[3] = fminf(fmaxf(pcy + 0.5f * ph, 0.f), hmax);
}

}  // namespace srcnn
