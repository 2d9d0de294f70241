// The frozen-BatchNorm fold as engine.fold_bn / autograd._fold compute it: in float64, every operation rounded once (no
// contraction), the result stored float32.  csrc/prep_weights.hip (inference plans) and csrc/train_fold.hip (training, both
// directions) fold through these, so the two carry the same bits by construction.
#pragma once
#include "common.h"

namespace srcnn {

// s = g / sqrt(v + eps) of channel co: g the BN's weight, v its running variance
__device__ __forceinline__ double bn_scale(const float *g, const float *v, int co)
{
#pragma clang fp contract(off)
    const double d = (double)v[co] + 1e-5;
    return (double)g[co] / sqrt(d);
}

// shift = b - m s of channel co (b the BN's bias, m its running mean): the folded bias of a convolution without one
__device__ __forceinline__ double bn_shift(const float *b, const float *m, int co, double s)
{
#pragma clang fp contract(off)
    const double ms = (double)m[co] * s;
    return (double)b[co] - ms;
}

// w' = w s, stored float32 (also the adjoint: d w = d w' s)
__device__ __forceinline__ float bn_mul(float w, double s)
{
#pragma clang fp contract(off)
    return (float)((double)w * s);
}

}  // namespace srcnn
