// 3 x f16 training: max|w| and the hi / lo planes of EVERY layer's weight, once per optimiser step, in a fixed number of launches
// (include/srcnn_hip.h states the contract).  What srcnn_conv2d_forward_f16x3 (f16x3_clear_scales,
// absmax_kernel over w, fwd_weight_split) and srcnn_conv2d_backward_f16x3 (the clear, absmax_kernel over the same w,
// bwd_weight_relayout_split) do per call and per direction is a function of the weights alone; the *_prepared entries of
// conv_forward_f16x3.hip / conv_backward_f16x3.hip read the results instead.  pow2_scale and split_f16 are conv_f16x3_scaled.h's, so
// the planes carry the bits those kernels write.
//
// THE LIST travels in kernel-argument blocks (layer_list.h), TW_LPL layers per block, as far as a table in the workspace:
// row_table_kernel writes its block's rows there and clears the rows' max words.  The two kernels that do the work read the
// table and are ONE launch each for the whole list, so their grids are balanced over all layers at once:
//   tw_absmax_kernel   a layer is TW_MAX_CHUNK-float chunks; workgroup = one chunk, its layer found by a binary search over the
//                      rows' running chunk counts (uniform over the workgroup: scalar loads).  float4 loads, wave_absmax_to_word:
//                      one integer atomicMax on the float bits per wave with a non-zero maximum.
//   tw_planes_kernel   unit = 32 rows of w (one row block of Cp) x up to TW_KTU K tiles (K tile = 32 channels of one tap =
//                      halves [32 kt, 32 kt + 32) of a row, Cin being a multiple of 32), found by the same search over the
//                      running unit counts.  Per K tile: thread (t >> 3, (t & 7) * 4) loads one float4 (rows beyond Cout: zeros),
//                      splits it and parks the halves in LDS (two 32 x 32 tiles, rows of 40 halves: 16-byte aligned rows); then
//                      threads 0..127 serve the hi planes and 128..255 the lo planes, each with one 16-byte store to the forward
//                      plane (8 channels of one row, one LDS read) and one to the backward plane (8 rows of one channel, eight
//                      2-byte LDS reads: the transpose).  The next K tile's load is issued before the stores.
// The clear cannot share a launch with the atomicMax (that would need a device-scope fence); it shares one with the table rows.
#include "conv_f16x3_scaled.h"
#include "layer_list.h"

namespace srcnn {

constexpr int TW_LPL = 48;                 // layers of one kernel-argument block (the header states the number)
constexpr int TW_MAX_CHUNK = 8192;         // floats of one tw_absmax_kernel workgroup: 8 float4 per thread
constexpr int TW_KTU = 8;                  // K tiles of one tw_planes_kernel unit: 32 x 256 floats in, 4 x 16 KB out
constexpr int TW_SROW = 40;                // halves per LDS row

struct TwRow {
    const float *w;
    unsigned *word;
    _Float16 *w_hi, *w_lo, *wt_hi, *wt_lo;
    int cout, cp, taps, cin;
    int max_end, plane_end;                // chunks / units of layers 0..this of the WHOLE list
    int kunits, pad;                       // units along K: ceil(taps * cin / 32 / TW_KTU)
};
static_assert(sizeof(TwRow) == 80, "the documented workspace record");

static_assert(sizeof(RowBlock<TwRow, TW_LPL>) <= 4096 - sizeof(void *), "the layer list must fit HIP's kernel-argument block");

__global__ __launch_bounds__(256) void tw_absmax_kernel(const TwRow *table, int n)
{
    const int t = threadIdx.x;
    const int li = first_run_above(table, &TwRow::max_end, n, blockIdx.x);
    const TwRow L = table[li];
    const int chunk = blockIdx.x - (li ? table[li - 1].max_end : 0);
    const long long groups = (long long)L.cout * L.taps * L.cin / 4;         // Cin % 32 == 0
    const long long base = (long long)chunk * (TW_MAX_CHUNK / 4);
    const float4 *w4 = reinterpret_cast<const float4 *>(L.w);
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < TW_MAX_CHUNK / 4 / 256; ++j) {
        const long long i = base + j * 256 + t;
        if (i < groups) {
            const float4 f = w4[i];
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(f.x), fabsf(f.y))), fmaxf(fabsf(f.z), fabsf(f.w)));
        }
    }
    wave_absmax_to_word(mx, L.word);
}

__global__ __launch_bounds__(256) void tw_planes_kernel(const TwRow *table, int n)
{
    __shared__ __attribute__((aligned(16))) _Float16 sh[2][32][TW_SROW];
    const int t = threadIdx.x;
    const int li = first_run_above(table, &TwRow::plane_end, n, blockIdx.x);
    const TwRow L = table[li];
    const int unit = blockIdx.x - (li ? table[li - 1].plane_end : 0);
    const int rb = unit / L.kunits, ku = unit - rb * L.kunits;
    const int n0 = rb * 32;
    const int ctiles = L.cin / BK, nkt = L.taps * ctiles;
    const int kt0 = ku * TW_KTU, kt1 = min(nkt, kt0 + TW_KTU);
    const size_t Kw = (size_t)L.taps * L.cin;
    const float s = pow2_scale(*L.word).s;

    // load role: row lrow, floats lcol .. lcol + 3 of the K tile
    const int lrow = t >> 3, lcol = (t & 7) * 4;
    const bool row_ok = n0 + lrow < L.cout;
    const float *src = L.w + (size_t)(row_ok ? n0 + lrow : 0) * Kw + lcol;
    // store role: plane pl; forward: row q, channels e .. e + 7; backward: channel q, rows e .. e + 7
    const int pl = t >> 7, q = (t & 127) >> 2, e = (t & 3) * 8;
    _Float16 *fwd = (pl ? L.w_lo : L.w_hi) + (size_t)(n0 + q) * Kw + e;
    _Float16 *bwd = pl ? L.wt_lo : L.wt_hi;

    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row_ok) f = *reinterpret_cast<const float4 *>(src + (size_t)kt0 * BK);
    for (int kt = kt0; kt < kt1; ++kt) {
        half4 hi, lo;
        split_f16x4(f, s, hi, lo);
        *reinterpret_cast<half4 *>(&sh[0][lrow][lcol]) = hi;
        *reinterpret_cast<half4 *>(&sh[1][lrow][lcol]) = lo;
        __syncthreads();
        if (row_ok && kt + 1 < kt1) f = *reinterpret_cast<const float4 *>(src + (size_t)(kt + 1) * BK);
        *reinterpret_cast<uint4 *>(fwd + (size_t)kt * BK) = *reinterpret_cast<const uint4 *>(&sh[pl][q][e]);
        half8 col;
#pragma unroll
        for (int k = 0; k < 8; ++k) col[k] = sh[pl][e + k][q];
        const int tap = kt / ctiles, c = (kt - tap * ctiles) * BK + q;
        *reinterpret_cast<half8 *>(bwd + ((size_t)c * L.taps + tap) * L.cp + n0 + e) = col;
        __syncthreads();                    // the tiles are rewritten by the next K tile
    }
}

// nullptr, or what is wrong with the layer
static const char *tw_check_layer(const srcnn_train_weight_desc &L)
{
    if (!L.w) return "null pointer: w";
    if (!L.w_amax) return "null pointer: w_amax";
    if (!L.w_hi || !L.w_lo || !L.wt_hi || !L.wt_lo) return "null pointer: a plane (w_hi, w_lo, wt_hi, wt_lo)";
    if (!aligned_to(L.w, 16)) return "w must be 16-byte aligned (vector loads)";
    if (!aligned_to(L.w_amax, 4)) return "w_amax must be 4-byte aligned";
    if (!aligned_to(L.w_hi, 16) || !aligned_to(L.w_lo, 16) || !aligned_to(L.wt_hi, 16) || !aligned_to(L.wt_lo, 16))
        return "the planes must be 16-byte aligned (vector stores)";
    if (L.Cout <= 0 || L.KH <= 0 || L.KW <= 0 || L.Cin <= 0) return "bad shape: sizes must be positive";
    if (L.Cin % BK != 0) return "Cin must be a positive multiple of 32";
    if (L.Cout >= (1 << 20) || L.KH >= 256 || L.KW >= 256) return "bad shape: tensor too large";
    const long long cp = (long long)cdiv(L.Cout, BK) * BK;
    if (cp * L.KH * L.KW * L.Cin >= (1LL << 31)) return "bad shape: a layer of 2^31 elements or more";
    return nullptr;
}

}  // namespace srcnn

extern "C" {

size_t srcnn_train_weights_workspace_bytes(int n_layers)
{
    return n_layers > 0 ? srcnn::align_up((size_t)n_layers * sizeof(srcnn::TwRow), 256) : 0;
}

int srcnn_train_weights_prepare(const srcnn_train_weight_desc *layers_host, int n_layers, void *workspace, size_t workspace_bytes,
                                srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(layers_host != nullptr, "null layers_host");
    SRCNN_REQUIRE(n_layers >= 1, "n_layers must be >= 1");
    SRCNN_REQUIRE(workspace != nullptr, "null workspace");
    SRCNN_REQUIRE(aligned_to(workspace, 16), "workspace must be 16-byte aligned");
    long long chunks = 0, units = 0;
    for (int i = 0; i < n_layers; ++i) {
        const char *m = tw_check_layer(layers_host[i]);
        if (m) {
            set_error("srcnn_train_weights_prepare: layer %d: %s", i, m);
            return SRCNN_ERR_ARG;
        }
        const srcnn_train_weight_desc &L = layers_host[i];
        const long long taps = L.KH * L.KW;
        chunks += ((long long)L.Cout * taps * L.Cin + TW_MAX_CHUNK - 1) / TW_MAX_CHUNK;
        units += (long long)cdiv(L.Cout, BK) * ((taps * (L.Cin / BK) + TW_KTU - 1) / TW_KTU);
    }
    SRCNN_REQUIRE(chunks < (1LL << 31) && units < (1LL << 31), "bad shape: the list is too large for one grid");
    if (workspace_bytes < srcnn_train_weights_workspace_bytes(n_layers)) {
        set_error("srcnn_train_weights_prepare: workspace too small (%zu < %zu)", workspace_bytes, srcnn_train_weights_workspace_bytes(n_layers));
        return SRCNN_ERR_WORKSPACE;
    }

    hipStream_t st = as_stream(stream);
    TwRow *table = static_cast<TwRow *>(workspace);
    RowBlock<TwRow, TW_LPL> b;
    b.n = 0, b.base = 0;
    chunks = units = 0;
    for (int i = 0; i < n_layers; ++i) {
        const srcnn_train_weight_desc &L = layers_host[i];
        TwRow &r = b.r[b.n];
        r.w = L.w, r.word = L.w_amax;
        r.w_hi = static_cast<_Float16 *>(L.w_hi), r.w_lo = static_cast<_Float16 *>(L.w_lo);
        r.wt_hi = static_cast<_Float16 *>(L.wt_hi), r.wt_lo = static_cast<_Float16 *>(L.wt_lo);
        r.cout = L.Cout, r.cp = cdiv(L.Cout, BK) * BK, r.taps = L.KH * L.KW, r.cin = L.Cin;
        r.kunits = cdiv(r.taps * (r.cin / BK), TW_KTU), r.pad = 0;
        chunks += ((long long)r.cout * r.taps * r.cin + TW_MAX_CHUNK - 1) / TW_MAX_CHUNK;
        units += (long long)(r.cp / BK) * r.kunits;
        r.max_end = (int)chunks, r.plane_end = (int)units;
        push_row<true>(b, i == n_layers - 1, table, st);
    }
    SRCNN_LAUNCH(tw_absmax_kernel, dim3((unsigned)chunks), dim3(256), 0, st, (const TwRow *)table, n_layers);
    SRCNN_LAUNCH(tw_planes_kernel, dim3((unsigned)units), dim3(256), 0, st, (const TwRow *)table, n_layers);
    return check_launch("srcnn_train_weights_prepare");
}

}  // extern "C"
