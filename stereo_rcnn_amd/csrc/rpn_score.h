// What the three RPN score kernels of rpn_proposal.hip (per level, all levels, partial planes) do per location, once, and the
// "level of an index" scan they share with gather_decode_kernel.
#pragma once

namespace srcnn {

// Level of index g from cumulative counts: level l owns [cum[l], cum[l + 1]), n levels.  A linear scan on purpose (at most four
// compares on values the kernels hold in scalar registers); layer_list.h's binary search is for long lists.
__device__ __forceinline__ int level_of(const int *cum, int n, int g)
{
    int l = 0;
    while (l + 1 < n && g >= cum[l + 1]) ++l;
    return l;
}

// One location: h = its 24 head values, [0,6) cls logits, [6,24) deltas.  probs_at / deltas_at = the location's first anchor in
// the (b, anchor, {0,1}) and (b, anchor, 6) outputs; a location's three anchors are consecutive.
__device__ __forceinline__ void rpn_pair_softmax_store(const float *h, float *probs_at, float *deltas_at)
{
    float pr[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {   // softmax over the channel pair (c, c+3)  (stereo_rpn.py:81-83)
        const float s0 = h[c], s1 = h[c + 3];
        const float m = fmaxf(s0, s1);
        const float e0 = expf(s0 - m), e1 = expf(s1 - m);
        const float sum = e0 + e1;
        pr[c] = e0 / sum;
        pr[c + 3] = e1 / sum;
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) probs_at[c] = pr[c];      // NHWC flatten pairs CONSECUTIVE channels (:89-90)
#pragma unroll
    for (int c = 0; c < 18; ++c) deltas_at[c] = h[6 + c];
}

}  // namespace srcnn
