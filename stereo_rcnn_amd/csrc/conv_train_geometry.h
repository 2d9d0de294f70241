// Host side of the training convolutions (conv_backward_common.h, conv_forward_f16x3.hip): the one check of the geometry that their
// two descriptors have in common.
#pragma once
#include "conv_common.h"
#include <cstdint>

namespace srcnn {

// What the training descriptors (srcnn_conv_bwd_desc, srcnn_conv_fwd_f16x3_desc) have in common: the geometry is checked --
// refusals carry the caller's name `who` -- and then copied into the kernel arguments (BwdArgs, FwdArgs) with what follows from
// it.  x_loaded: the call reads x with 16-byte loads.
template <class Desc, class Args>
inline int check_conv_geometry(const char *who, const Desc *d, bool x_loaded, Args &a)
{
    SRCNN_REQUIRE_AS(who, d->B > 0 && d->H > 0 && d->W > 0 && d->OH > 0 && d->OW > 0 && d->Cout > 0 && d->Cin > 0, "bad shape: sizes must be positive");
    SRCNN_REQUIRE_AS(who, d->KH > 0 && d->KW > 0 && d->stride > 0 && d->pad >= 0, "bad shape: kernel, stride > 0 and pad >= 0");
    SRCNN_REQUIRE_AS(who, d->H + 2 * d->pad >= d->KH && d->W + 2 * d->pad >= d->KW &&
                         d->OH == (d->H + 2 * d->pad - d->KH) / d->stride + 1 && d->OW == (d->W + 2 * d->pad - d->KW) / d->stride + 1,
                     "bad shape: OH / OW are not the forward's output size");
    SRCNN_REQUIRE_AS(who, d->Cin % BK == 0, "Cin must be a positive multiple of 32");
    SRCNN_REQUIRE_AS(who, d->x_cstride >= d->Cin && d->x_cstride % 4 == 0, "x_cstride: a stride of at least Cin floats, a multiple of 4");
    SRCNN_REQUIRE_AS(who, d->y_coffset >= 0 && d->y_cstride >= d->y_coffset + d->Cout, "y_cstride: a stride of at least y_coffset + Cout floats");
    SRCNN_REQUIRE_AS(who, !x_loaded || (reinterpret_cast<uintptr_t>(d->x) & 15) == 0, "x must be 16-byte aligned (stride-4 vector loads)");
    SRCNN_REQUIRE_AS(who, (unsigned)d->tile_mr <= 2 && (unsigned)d->tile_nr <= 2, "tile_mr / tile_nr must be 0, 1 or 2");
    const long long M = (long long)d->B * d->OH * d->OW, Min = (long long)d->B * d->H * d->W;
    const long long Kw = (long long)d->KH * d->KW * d->Cin;
    SRCNN_REQUIRE_AS(who, M < (1LL << 31) && Min < (1LL << 31) && Kw < (1LL << 31) && d->Cout < (1 << 20) && d->KH < 256 && d->KW < 256,
                     "bad shape: tensor too large");
    a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.xcs = d->x_cstride;
    a.OH = d->OH; a.OW = d->OW; a.Cout = d->Cout; a.Cp = cdiv(d->Cout, BK) * BK;
    a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad;
    a.ycs = d->y_cstride; a.yco = d->y_coffset; a.relu = d->relu ? 1 : 0;
    a.M = (int)M; a.Min = (int)Min; a.taps = d->KH * d->KW; a.Kw = (int)Kw;
    return SRCNN_OK;
}

}  // namespace srcnn
