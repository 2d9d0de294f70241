// Training: the frozen-BN fold and the re-layout of EVERY layer's weight on the device, and its adjoint, each in a fixed number of
// launches (include/srcnn_hip.h states the contract).  What stereo_rcnn_amd.autograd's fold_conv / fold_linear /
// fold_deconv2x2 + .contiguous() + torch.cat do per layer with eager operators, and what torch autograd does on the way back
// through them.  The float64 fold is bn_fold.h's, which csrc/prep_weights.hip calls too (one rounding per operation, contraction
// off), so the results carry the eager path's bits.
//
// THE LIST travels as csrc/train_weights.hip's does: TF_LPL layers per kernel-argument block into a table in the workspace
// (layer_list.h's row_table_kernel), then ONE launch of tf_kernel<direction> over the running unit counts of the whole table.
//
// A unit is RB output rows x CC input channels (all T = KH KW taps), RB CC T <= TF_TILE floats, CC a multiple of 32 (the host
// chooses RB and CC per layer: prep_weights.hip's cut along the source's contiguous side).  On the PARAMETER side
// ((rows, Cin, T)) a row of the unit is one run of CC T floats from channel c0 on; on the ENGINE side ((Cout, T, Cin)) it is T runs
// of CC floats.  Both start at multiples of 16 bytes (32 | c0, 32 | Cin), so every global access is a float4.
//   forward   parameter side --float4--> fold --float4--> LDS (parameter order); LDS --4 x b32, stride T--> float4 --> engine side
//   backward  engine side --float4--> 4 x b32 stores, stride T --> LDS (parameter order); LDS --float4--> scale --float4--> parameter side
// The stride-T LDS accesses of consecutive lanes are 4 T dwords apart: 4-way conflicts on the 32-bank b32 path for odd T (none
// for T = 1, the copy).  Four of them feed one 16-byte global access, 32 LDS cycles per KB moved and wave: several times above
// the rate at which HBM can feed a CU, so the tile is not padded.
// The deconvolution ((Cin, Cout, 2, 2) -> row (ij, co), column ci) is a full transpose with a row permutation: its unit is 32 ci x
// up to 32 co x 4 ij, rows of the LDS tile padded by 4 floats.
// The rows' biases are written by the units of the first channel chunk.
#include "bn_fold.h"
#include "layer_list.h"

namespace srcnn {

constexpr int TF_THREADS = 256;
constexpr int TF_TILE = 4096;                      // floats of one unit in LDS
constexpr int TF_MAX_RB = 64;                      // rows of one unit (their BN scales sit in LDS)
constexpr int TF_DC = 32;                          // deconvolution unit: TF_DC ci x TF_DC co x 4
constexpr int TF_MAX_TAPS = TF_TILE / 32;          // 32 channels of one row must fit the tile
constexpr int TF_LPL = SRCNN_TRAIN_FOLD_LAYERS_PER_BLOCK;

struct TfRow {
    float *part_w[3];                              // parameter side: the forward reads it, the backward writes it
    float *part_b[3];
    const float *bn_g, *bn_b, *bn_m, *bn_v;
    float *eng_w, *eng_b;                          // engine side: the forward writes it, the backward reads it; nullptr: skipped
    int rows[3];
    int nparts, kind, cout, cin, taps;
    int rb, cc, nchunk;                            // unit: rb rows x cc channels; nchunk units along the channels
    int unit_end;                                  // units of layers 0..this of the WHOLE list
};
static_assert(sizeof(TfRow) == 144, "the documented workspace record");

static_assert(sizeof(RowBlock<TfRow, TF_LPL>) <= 4096 - sizeof(void *), "the layer list must fit HIP's kernel-argument block");

// the folded bias of row co under the BN of scale s: the shift, plus the scaled bias of a convolution that has one
__device__ __forceinline__ float tf_bias(const TfRow &L, int co, double s)
{
#pragma clang fp contract(off)
    const double shift = bn_shift(L.bn_b, L.bn_m, co, s);
    if (!L.part_b[0]) return (float)shift;
    const double bs = (double)L.part_b[0][co] * s;
    return (float)(bs + shift);
}

__device__ __forceinline__ float4 tf_mul4(float4 v, double s)
{
    return make_float4(bn_mul(v.x, s), bn_mul(v.y, s), bn_mul(v.z, s), bn_mul(v.w, s));
}

template <bool BWD>
__device__ __forceinline__ void tf_deconv_unit(const TfRow &L, int unit, float *tile)
{
    const int t = threadIdx.x;
    const int cg = unit / L.nchunk, ch = unit - cg * L.nchunk;
    const int co0 = cg * TF_DC, c0 = ch * TF_DC;
    const int nco = min(TF_DC, L.cout - co0), pitch = nco * 4 + 4;
    if (!BWD && ch == 0 && L.eng_b && t < nco * 4) {
        const int ij = t / nco, col = t - ij * nco;
        L.eng_b[ij * L.cout + co0 + col] = L.part_b[0][co0 + col];
    }
    if (!L.eng_w) return;
    // parameter side: (ci, co) -> the four (i, j) of it, one float4; engine side: row (ij, co), four ci, one float4
    auto param_side = [&](int q, float *&g, float *&s) {
        const int cil = q / nco, col = q - cil * nco;
        g = L.part_w[0] + ((size_t)(c0 + cil) * L.cout + co0 + col) * 4;
        s = tile + cil * pitch + col * 4;
    };
    auto engine_side = [&](int q, float *&g, float *&s) {
        const int rr = q >> 3, cl = (q & 7) << 2;
        const int ij = rr / nco, col = rr - ij * nco;
        g = L.eng_w + (size_t)(ij * L.cout + co0 + col) * L.cin + c0 + cl;
        s = tile + cl * pitch + col * 4 + ij;
    };
    float *g, *s;
    if (!BWD) {
        for (int q = t; q < TF_DC * nco; q += TF_THREADS) {
            param_side(q, g, s);
            *reinterpret_cast<float4 *>(s) = *reinterpret_cast<const float4 *>(g);
        }
        __syncthreads();
        for (int q = t; q < nco * 4 * (TF_DC / 4); q += TF_THREADS) {
            engine_side(q, g, s);
            *reinterpret_cast<float4 *>(g) = make_float4(s[0], s[pitch], s[2 * pitch], s[3 * pitch]);
        }
    } else {
        for (int q = t; q < nco * 4 * (TF_DC / 4); q += TF_THREADS) {
            engine_side(q, g, s);
            const float4 v = *reinterpret_cast<const float4 *>(g);
            s[0] = v.x, s[pitch] = v.y, s[2 * pitch] = v.z, s[3 * pitch] = v.w;
        }
        __syncthreads();
        for (int q = t; q < TF_DC * nco; q += TF_THREADS) {
            param_side(q, g, s);
            *reinterpret_cast<float4 *>(g) = *reinterpret_cast<const float4 *>(s);
        }
    }
}

template <bool BWD>
__global__ __launch_bounds__(TF_THREADS) void tf_kernel(const TfRow *table, int n)
{
    __shared__ __attribute__((aligned(16))) float tile[TF_TILE + 4 * TF_DC];
    __shared__ double sc[TF_MAX_RB];
    const int t = threadIdx.x;
    const int li = first_run_above(table, &TfRow::unit_end, n, blockIdx.x);
    const TfRow L = table[li];
    const int unit = blockIdx.x - (li ? table[li - 1].unit_end : 0);
    if (L.kind == SRCNN_TRAIN_FOLD_DECONV2X2) {
        tf_deconv_unit<BWD>(L, unit, tile);
        return;
    }
    const int T = L.taps, RB = L.rb, CC = L.cc;
    const int rg = unit / L.nchunk, ch = unit - rg * L.nchunk;
    const int r0 = rg * RB, c0 = ch * CC;
    const int nr = min(RB, L.cout - r0), nc = min(CC, L.cin - c0);
    const bool bn = L.bn_g != nullptr;

    // the rows' BN scales, and (first channel chunk only) their biases
    if (t < nr) {
        const int row = r0 + t;
        int p, co;
        part_of_row(L.nparts, L.rows, row, p, co);
        const double s = bn ? bn_scale(L.bn_g, L.bn_v, co) : 1.0;
        sc[t] = s;
        if (ch == 0 && L.eng_b) {
            if (!BWD) L.eng_b[row] = bn ? tf_bias(L, co, s) : L.part_b[p][co];
            else L.part_b[p][co] = bn ? bn_mul(L.eng_b[row], s) : L.eng_b[row];
        }
    }
    __syncthreads();
    if (!L.eng_w) return;

    const int per_row = nc * T;                 // floats of one row of this unit: contiguous on the parameter side, 4 | per_row
    const int q_row = per_row >> 2, qc = nc >> 2;
    const size_t eng_row = (size_t)T * L.cin;
    // parameter side: float4 j of row rl; engine side: tap `tap`, channels cl .. cl + 3 of row rl (LDS: stride T)
    auto param_side = [&](int q, float *&g, float *&s, int &rl) {
        rl = q / q_row;
        const int j = (q - rl * q_row) << 2;
        int p, co;
        part_of_row(L.nparts, L.rows, r0 + rl, p, co);
        g = L.part_w[p] + ((size_t)co * L.cin + c0) * T + j;
        s = tile + rl * per_row + j;
    };
    auto engine_side = [&](int q, float *&g, float *&s) {
        const int rl = q / (T * qc), r = q - rl * (T * qc), tap = r / qc, cl = (r - tap * qc) << 2;
        g = L.eng_w + (size_t)(r0 + rl) * eng_row + (size_t)tap * L.cin + c0 + cl;
        s = tile + rl * per_row + cl * T + tap;
    };
    float *g, *s;
    int rl;
    if (!BWD) {
        for (int q = t; q < nr * q_row; q += TF_THREADS) {
            param_side(q, g, s, rl);
            float4 v = *reinterpret_cast<const float4 *>(g);
            if (bn) v = tf_mul4(v, sc[rl]);
            *reinterpret_cast<float4 *>(s) = v;
        }
        __syncthreads();
        for (int q = t; q < nr * T * qc; q += TF_THREADS) {
            engine_side(q, g, s);
            *reinterpret_cast<float4 *>(g) = make_float4(s[0], s[T], s[2 * T], s[3 * T]);
        }
    } else {
        for (int q = t; q < nr * T * qc; q += TF_THREADS) {
            engine_side(q, g, s);
            const float4 v = *reinterpret_cast<const float4 *>(g);
            s[0] = v.x, s[T] = v.y, s[2 * T] = v.z, s[3 * T] = v.w;
        }
        __syncthreads();
        for (int q = t; q < nr * q_row; q += TF_THREADS) {
            param_side(q, g, s, rl);
            float4 v = *reinterpret_cast<const float4 *>(s);
            if (bn) v = tf_mul4(v, sc[rl]);
            *reinterpret_cast<float4 *>(g) = v;
        }
    }
}

// nullptr, or what is wrong with the layer; dw / db: the backward's gradients of the folded tensors (forward: unused)
static const char *tf_check_layer(const srcnn_train_fold_desc &L, bool backward, const float *dw, const float *db)
{
    if (L.kind != SRCNN_TRAIN_FOLD_CONV && L.kind != SRCNN_TRAIN_FOLD_LINEAR && L.kind != SRCNN_TRAIN_FOLD_DECONV2X2)
        return "unknown layout kind (SRCNN_TRAIN_FOLD_*)";
    if (L.n_parts < 1 || L.n_parts > 3) return "n_parts must be 1, 2 or 3";
    if (L.Cout <= 0 || L.KH <= 0 || L.KW <= 0 || L.Cin <= 0) return "bad shape: sizes must be positive";
    if (L.Cin % 32 != 0) return "Cin must be a positive multiple of 32";
    if (L.KH * (long long)L.KW > TF_MAX_TAPS) return "bad shape: KH KW above 128";
    if (L.kind == SRCNN_TRAIN_FOLD_LINEAR && (L.KH != 1 || L.KW != 1)) return "bad shape: the linear kind is 1x1";
    if (L.kind == SRCNN_TRAIN_FOLD_DECONV2X2 && (L.KH != 2 || L.KW != 2 || L.n_parts != 1)) return "bad shape: the deconvolution kind is one 2x2 part";
    long long rows = 0;
    for (int p = 0; p < L.n_parts; ++p) {
        if (L.rows[p] <= 0) return "bad shape: the rows of a part must be positive";
        rows += L.rows[p];
    }
    if (rows != L.Cout) return "the rows of the parts do not sum to Cout";
    if ((long long)L.Cout * L.KH * L.KW * L.Cin >= (1LL << 31)) return "bad shape: a layer of 2^31 elements or more";
    const bool any_bn = L.bn_weight || L.bn_bias || L.bn_mean || L.bn_var, bn = L.bn_weight && L.bn_bias && L.bn_mean && L.bn_var;
    if (any_bn && !bn) return "null pointer: a frozen BN needs all of bn_weight, bn_bias, bn_mean, bn_var";
    if (bn && (L.n_parts != 1 || L.kind == SRCNN_TRAIN_FOLD_DECONV2X2)) return "a frozen BN folds into a single convolution part";
    if (!aligned_to(L.bn_weight, 4) || !aligned_to(L.bn_bias, 4) || !aligned_to(L.bn_mean, 4) || !aligned_to(L.bn_var, 4))
        return "the BN tensors must be 4-byte aligned";
    const bool bias = L.bias[0] != nullptr;
    for (int p = 0; p < L.n_parts; ++p) {
        if (!backward) {                                    // the backward reads no weight
            if (!L.w[p]) return "null pointer: w of a part";
            if (!aligned_to(L.w[p], 16)) return "w must be 16-byte aligned (vector loads)";
        }
        if ((L.bias[p] != nullptr) != bias) return "every part carries a bias, or none";
        if (!aligned_to(L.bias[p], 4)) return "bias must be 4-byte aligned";
        if (backward && dw) {
            if (!L.grad_w[p]) return "null pointer: grad_w of a part";
            if (!aligned_to(L.grad_w[p], 16)) return "grad_w must be 16-byte aligned (vector stores)";
        }
        if (backward && db && bias) {
            if (!L.grad_b[p]) return "null pointer: grad_b of a part";
            if (!aligned_to(L.grad_b[p], 4)) return "grad_b must be 4-byte aligned";
        }
    }
    if (!backward) {
        if (!L.dst_w) return "null pointer: dst_w";
        if (!aligned_to(L.dst_w, 16)) return "dst_w must be 16-byte aligned (vector stores)";
        if ((bn || bias) && !L.dst_b) return "null pointer: dst_b (a BN or a bias leaves a folded bias)";
        if (!bn && !bias && L.dst_b) return "dst_b without a BN or a bias";
        if (!aligned_to(L.dst_b, 4)) return "dst_b must be 4-byte aligned";
    } else {
        if (!aligned_to(dw, 16)) return "dw_folded must be 16-byte aligned (vector loads)";
        if (!aligned_to(db, 4)) return "db_folded must be 4-byte aligned";
        if (db && L.kind == SRCNN_TRAIN_FOLD_DECONV2X2) return "db_folded of a deconvolution is not taken: its bias stays the caller's repeat(4)";
    }
    return nullptr;
}

static int tf_run(const char *who, const srcnn_train_fold_desc *layers_host, int n_layers, bool backward, const float *const *dw,
                  const float *const *db, void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    SRCNN_REQUIRE_AS(who, layers_host != nullptr, "null layers_host");
    SRCNN_REQUIRE_AS(who, n_layers >= 1, "n_layers must be >= 1");
    SRCNN_REQUIRE_AS(who, workspace != nullptr, "null workspace");
    SRCNN_REQUIRE_AS(who, aligned_to(workspace, 16), "workspace must be 16-byte aligned");
    SRCNN_REQUIRE_AS(who, !backward || (dw && db), "null dw_folded_host / db_folded_host (the arrays; their entries may be null)");
    for (int i = 0; i < n_layers; ++i) {
        const char *m = tf_check_layer(layers_host[i], backward, backward ? dw[i] : nullptr, backward ? db[i] : nullptr);
        if (m) {
            set_error("%s: layer %d: %s", who, i, m);
            return SRCNN_ERR_ARG;
        }
    }
    if (workspace_bytes < srcnn_train_fold_workspace_bytes(n_layers)) {
        set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, srcnn_train_fold_workspace_bytes(n_layers));
        return SRCNN_ERR_WORKSPACE;
    }

    // two passes over the list: the unit counts (so that an over-long list is refused before the first launch), then the launches
    hipStream_t st = as_stream(stream);
    TfRow *table = static_cast<TfRow *>(workspace);
    long long units = 0;
    for (int pass = 0; pass < 2; ++pass) {
        RowBlock<TfRow, TF_LPL> b;
        b.n = 0, b.base = 0;
        long long run = 0;
        for (int i = 0; i < n_layers; ++i) {
            const srcnn_train_fold_desc &L = layers_host[i];
            TfRow &r = b.r[b.n];
            const bool bias = L.bias[0] != nullptr;
            for (int p = 0; p < 3; ++p) {
                const bool in = p < L.n_parts;
                r.part_w[p] = !in ? nullptr : backward ? L.grad_w[p] : const_cast<float *>(L.w[p]);
                r.part_b[p] = !in ? nullptr : backward ? L.grad_b[p] : const_cast<float *>(L.bias[p]);
                r.rows[p] = in ? L.rows[p] : 0;
            }
            r.bn_g = L.bn_weight, r.bn_b = L.bn_bias, r.bn_m = L.bn_mean, r.bn_v = L.bn_var;
            r.eng_w = backward ? const_cast<float *>(dw[i]) : L.dst_w;
            r.eng_b = backward ? (bias ? const_cast<float *>(db[i]) : nullptr) : L.dst_b;
            r.nparts = L.n_parts, r.kind = L.kind, r.cout = L.Cout, r.cin = L.Cin, r.taps = L.KH * L.KW;
            long long u;
            if (L.kind == SRCNN_TRAIN_FOLD_DECONV2X2) {
                r.rb = r.cc = TF_DC, r.nchunk = L.Cin / TF_DC;
                u = (long long)cdiv(L.Cout, TF_DC) * r.nchunk;
            } else {
                int cc = std::min(L.Cin, TF_TILE / r.taps / 32 * 32), rb = 1;
                if (cc == L.Cin) rb = std::max(1, std::min({TF_TILE / (cc * r.taps), TF_MAX_RB, L.Cout}));
                r.rb = rb, r.cc = cc, r.nchunk = cdiv(L.Cin, cc);
                u = (long long)cdiv(L.Cout, rb) * r.nchunk;
            }
            if (!r.eng_w && !r.eng_b) u = 0;                // (backward) a layer without gradients
            run += u;
            r.unit_end = (int)run;
            push_row<false>(b, i == n_layers - 1, pass == 1 ? table : nullptr, st);
        }
        if (pass == 0) {
            units = run;
            SRCNN_REQUIRE_AS(who, units < (1LL << 31), "bad shape: the list is too large for one grid");
            if (units == 0) return SRCNN_OK;                // nothing asked for: nothing launched
        }
    }
    if (backward) SRCNN_LAUNCH(tf_kernel<true>, dim3((unsigned)units), dim3(TF_THREADS), 0, st, (const TfRow *)table, n_layers);
    else SRCNN_LAUNCH(tf_kernel<false>, dim3((unsigned)units), dim3(TF_THREADS), 0, st, (const TfRow *)table, n_layers);
    return check_launch(who);
}

}  // namespace srcnn

extern "C" {

size_t srcnn_train_fold_workspace_bytes(int n_layers)
{
    return n_layers > 0 ? srcnn::align_up((size_t)n_layers * sizeof(srcnn::TfRow), 256) : 0;
}

int srcnn_train_weights_fold(const srcnn_train_fold_desc *layers_host, int n_layers, void *workspace, size_t workspace_bytes,
                             srcnn_stream_t stream)
{
    return srcnn::tf_run("srcnn_train_weights_fold", layers_host, n_layers, false, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int srcnn_train_weights_fold_backward(const srcnn_train_fold_desc *layers_host, int n_layers, const float *const *dw_folded_host,
                                      const float *const *db_folded_host, void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    return srcnn::tf_run("srcnn_train_weights_fold_backward", layers_host, n_layers, true, dw_folded_host, db_folded_host, workspace,
                         workspace_bytes, stream);
}

}  // extern "C"
