// Weight preparation on the device (gfx950): everything engine.prep_* + ConvW.split_f16x3 + head_fragments do with eager torch ops,
// for a LIST of layers in one call and into caller-supplied destinations -- the in-place refresh of an inference plan's weights
// from live (trained) parameters, without a host read inside the call.
//
// Per layer (include/srcnn_hip.h, "weight preparation", states the forms):
//   pass A  prep_fold_kernel   frozen-BN fold in float64 (one rounding per operation, no contraction), stored float32, written in
//                              the engine's layout; the bias; max |w'| of the layer
//   pass B  prep_split_kernel  k from the exponent and mantissa of the max, hi = f16(w' 2^k), lo = f16(w' 2^k - hi), the fragment
//                              layout of a fused head from the same hi / lo, k to the caller's device array
// The layer descriptors travel in the kernels' argument blocks, at most SRCNN_PREP_LAYERS_PER_LAUNCH per launch (layer_list.h): no
// device table, no upload.
//
// Pass A's unit of work is RB destination rows x CC input channels with RB * CC * taps <= PREP_TILE floats: the source of such a
// unit is contiguous per row ((Cout, Cin, KH, KW): CC * taps floats from channel c0 on), it is read in source order -- 16 bytes
// per lane where the layer's sizes and pointers allow -- folded, and parked in LDS; the unit is then written in destination order
// ((Cout, KH, KW, Cin): per tap a run of CC floats), again 16 bytes per lane where possible.  The LDS read of the second half has
// stride `taps` floats (9, 49: odd, conflict free; 1: the identity).  This is conv_backward.hip's bwd_weight_relayout with the
// tile cut along the source's contiguous side.
//
// The max is an integer max over the bit patterns of |w'| (they order like the values, and every NaN pattern lies above +inf, so
// a NaN wins as it does in torch.max): lanes, then the four wavefronts through LDS, then one integer atomicMax per workgroup on the
// layer's word of the workspace -- order independent, so the same bits on every run; no float atomics anywhere.
#include "bn_fold.h"
#include "layer_list.h"

#include <hip/hip_fp16.h>

#include <cstdint>

namespace srcnn {

constexpr int PREP_THREADS = 256;
constexpr int PREP_TILE = 4096;                    // floats of one pass-A unit in LDS (16 KB), elements of one pass-B chunk
constexpr int PREP_MAX_RB = 64;                    // rows of one unit (their BN scales sit in LDS)
constexpr int PREP_LPL = SRCNN_PREP_LAYERS_PER_LAUNCH;
constexpr int PREP_VEC_IN = 1, PREP_VEC_OUT = 2;   // PrepArgs::vec bits

struct PrepArgs {
    srcnn_prep_layer l[PREP_LPL];
    int block_end[PREP_LPL];    // workgroups of layers 0..i of this launch
    short rb[PREP_LPL];         // pass A: rows per unit
    short cc[PREP_LPL];         // pass A: channels per unit
    unsigned char vec[PREP_LPL];
    int n, layer_base;          // layer_base: number of this launch's first layer in the whole list
    unsigned *maxbits;          // one word per layer of the whole list
    int *k_out;
};
static_assert(sizeof(PrepArgs) <= 4096, "the layer list must fit HIP's kernel-argument block");

__host__ __device__ inline int prep_rows(const srcnn_prep_layer &L)
{
    if (L.form == SRCNN_PREP_DECONV2X2) return 4 * L.cout[0];
    int r = 0;
    for (int s = 0; s < L.n_src; ++s) r += L.cout[s];
    return L.form == SRCNN_PREP_CONV ? r : L.cout[0];
}

// channels the units of a layer are cut along, taps per channel in the SOURCE, floats of a DESTINATION row
__host__ __device__ inline int prep_chan(const srcnn_prep_layer &L) { return L.form == SRCNN_PREP_SHORTCUT ? L.cin + L.cin2 : L.cin; }
__host__ __device__ inline int prep_taps(const srcnn_prep_layer &L)
{
    return L.form == SRCNN_PREP_CONV ? L.kh * L.kw : L.form == SRCNN_PREP_STEM ? 49 : 1;
}
__host__ __device__ inline long long prep_row_len(const srcnn_prep_layer &L)
{
    return L.form == SRCNN_PREP_STEM ? 224 : (long long)prep_chan(L) * prep_taps(L);
}

// BN `which` of the layer through bn_fold.h: the scale of row co (1 without a BN), its folded bias, a folded weight
__device__ __forceinline__ double bn_scale(const srcnn_prep_layer &L, int which, int co)
{
    return L.bn_g[which] ? bn_scale(L.bn_g[which], L.bn_v[which], co) : 1.0;
}

__device__ __forceinline__ float bn_bias(const srcnn_prep_layer &L, int which, int co, double s)
{
    return (float)bn_shift(L.bn_b[which], L.bn_m[which], co, s);
}

__device__ __forceinline__ float fold(float w, double s, bool bn) { return bn ? bn_mul(w, s) : w; }

// source tensor and row inside it of destination row `row` of a CONV layer (sources concatenated along Cout): layer_list.h's
// part_of_row RESTATED, because calling it moves prep_fold_kernel's instruction stream (profiles/train_list_helpers_ab.txt)
__device__ __forceinline__ void conv_source(const srcnn_prep_layer &L, int row, int &s, int &co)
{
    s = 0, co = row;
    if (L.n_src > 1 && co >= L.cout[0]) {
        co -= L.cout[0], s = 1;
        if (L.n_src > 2 && co >= L.cout[1]) co -= L.cout[1], s = 2;
    }
}

__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

__global__ __launch_bounds__(PREP_THREADS) void prep_fold_kernel(const PrepArgs a)
{
    __shared__ __attribute__((aligned(16))) float tile[PREP_TILE];
    __shared__ double sc[2][PREP_MAX_RB];
    __shared__ unsigned wmax[PREP_THREADS / 64];
    const int t = threadIdx.x;
    const int li = first_run_above(a.block_end, a.n, blockIdx.x);
    const srcnn_prep_layer &L = a.l[li];
    const int unit = blockIdx.x - (li ? a.block_end[li - 1] : 0);
    const int form = L.form, rows = prep_rows(L), chan = prep_chan(L), T = prep_taps(L);
    const int RB = a.rb[li], CC = a.cc[li];
    const int nchunk = (chan + CC - 1) / CC;
    const int rg = unit / nchunk, ch = unit - rg * nchunk;
    const int r0 = rg * RB, c0 = ch * CC;
    const int nr = min(RB, rows - r0), nc = min(CC, chan - c0);
    const bool bn = L.bn_g[0] != nullptr;
    const int cout0 = L.cout[0];

    // the rows' BN scales, and (first channel chunk only) their biases
    if (t < nr) {
        const int row = r0 + t;
        if (form == SRCNN_PREP_DECONV2X2) {
            if (ch == 0 && row < cout0 && L.dst_b) L.dst_b[row] = L.b[0][row];
        } else if (form == SRCNN_PREP_SHORTCUT) {
            const double s0 = bn_scale(L, 0, row), s1 = bn_scale(L, 1, row);
            sc[0][t] = s0, sc[1][t] = s1;
            if (ch == 0) {
#pragma clang fp contract(off)
                const float b0 = bn_bias(L, 0, row, s0), b1 = bn_bias(L, 1, row, s1);
                L.dst_b[row] = (float)((double)b0 + (double)b1);
            }
        } else {
            int s, co;
            conv_source(L, row, s, co);
            const double s0 = bn ? bn_scale(L, 0, co) : 1.0;
            sc[0][t] = s0;
            if (ch == 0 && L.dst_b) L.dst_b[row] = bn ? bn_bias(L, 0, co, s0) : L.b[s][co];
        }
    }
    __syncthreads();

    // ---- source order -> LDS
    const int per_row = nc * T;                 // floats of one row of this unit, contiguous in the source (not DECONV)
    const int total = nr * per_row;
    unsigned mx = 0;
    if ((a.vec[li] & PREP_VEC_IN) && form != SRCNN_PREP_DECONV2X2) {
        const int q_row = per_row >> 2;         // per_row % 4 == 0 here
        for (int q = t; q < nr * q_row; q += PREP_THREADS) {
            const int rl = q / q_row, j = (q - rl * q_row) << 2;
            const int row = r0 + rl;
            const float *src;
            double s;
            if (form == SRCNN_PREP_SHORTCUT) {
                const int col = c0 + j;         // cin % 4 == 0: a group of four lies in one of the two sources
                const bool second = col >= L.cin;
                src = second ? L.w[1] + (size_t)row * L.cin2 + (col - L.cin) : L.w[0] + (size_t)row * L.cin + col;
                s = sc[second ? 1 : 0][rl];
            } else {
                int si, co;
                conv_source(L, row, si, co);
                src = L.w[si] + ((size_t)co * chan + c0) * T + j;
                s = sc[0][rl];
            }
            float4 v = *reinterpret_cast<const float4 *>(src);
            v.x = fold(v.x, s, bn), v.y = fold(v.y, s, bn), v.z = fold(v.z, s, bn), v.w = fold(v.w, s, bn);
            mx = max(max(mx, abs_bits(v.x)), max(abs_bits(v.y), max(abs_bits(v.z), abs_bits(v.w))));
            *reinterpret_cast<float4 *>(tile + rl * per_row + j) = v;
        }
    } else {
        for (int i = t; i < total; i += PREP_THREADS) {
            const int rl = i / per_row, j = i - rl * per_row;
            const int row = r0 + rl;
            float v;
            if (form == SRCNN_PREP_DECONV2X2) {          // (Cin, Cout, 2, 2) -> row (i, j, co), column ci
                const int ij = row / cout0, co = row - ij * cout0;
                v = L.w[0][((size_t)(c0 + j) * cout0 + co) * 4 + ij];
            } else if (form == SRCNN_PREP_SHORTCUT) {
                const int col = c0 + j;
                const bool second = col >= L.cin;
                const float w = second ? L.w[1][(size_t)row * L.cin2 + (col - L.cin)] : L.w[0][(size_t)row * L.cin + col];
                v = fold(w, sc[second ? 1 : 0][rl], bn);
            } else {
                int si, co;
                conv_source(L, row, si, co);
                v = fold(L.w[si][((size_t)co * chan + c0) * T + j], sc[0][rl], bn);
            }
            mx = max(mx, abs_bits(v));
            tile[i] = v;
        }
    }

    // ---- max |w'| of the unit -> the layer's word
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
    if ((t & 63) == 0) wmax[t >> 6] = mx;
    __syncthreads();                                        // (also: the tile is complete)
    if (t == 0) atomicMax(a.maxbits + a.layer_base + li, max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));

    // ---- LDS -> destination order
    float *dst = L.dst_w;
    if (form == SRCNN_PREP_STEM) {
        // row (kh 7, pixel 8, NHWC4): the 7 x 7 x 3 taps, zero in pixel 7 and channel 3; one float4 = one pixel
        for (int q = t; q < nr * 56; q += PREP_THREADS) {
            const int rl = q / 56, r = q - rl * 56, kh = r >> 3, p = r & 7;
            const float *s = tile + rl * 147 + kh * 7 + p;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < 7) v.x = s[0], v.y = s[49], v.z = s[98];
            float *d = dst + (size_t)(r0 + rl) * 224 + r * 4;
            if (a.vec[li] & PREP_VEC_OUT) *reinterpret_cast<float4 *>(d) = v;
            else d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
        return;
    }
    const size_t row_len = (size_t)chan * T;
    if (a.vec[li] & PREP_VEC_OUT) {             // chan % 4 == 0, CC % 4 == 0: nc % 4 == 0
        const int qc = nc >> 2;
        for (int q = t; q < nr * T * qc; q += PREP_THREADS) {
            const int rl = q / (T * qc), r = q - rl * (T * qc), tap = r / qc, cl = (r - tap * qc) << 2;
            const float *s = tile + rl * per_row + cl * T + tap;
            const float4 v = make_float4(s[0], s[T], s[2 * T], s[3 * T]);
            *reinterpret_cast<float4 *>(dst + (size_t)(r0 + rl) * row_len + (size_t)tap * chan + c0 + cl) = v;
        }
    } else {
        for (int o = t; o < total; o += PREP_THREADS) {
            const int rl = o / per_row, r = o - rl * per_row, tap = r / nc, cl = r - tap * nc;
            dst[(size_t)(r0 + rl) * row_len + (size_t)tap * chan + c0 + cl] = tile[rl * per_row + cl * T + tap];
        }
    }
}

// k = floor(log2(16384 / m)) from the bits of m = f 2^e, 1 <= f < 2: 14 - e where f == 1, 13 - e otherwise (16384 / m lies strictly
// between 2^(13 - e) and 2^(14 - e) then, by more than float64's rounding of the quotient and of log2 can bridge); 0 for m == 0
// and for a NaN max (the eager path's `m > 0` is false for both).  An infinite max has no eager value (math.log2(0) raises): 0.
__device__ __forceinline__ int split_exponent(unsigned bits)
{
    if (bits == 0 || bits >= 0x7f800000u) return 0;
    int e = (int)(bits >> 23) - 127;
    unsigned man = bits & 0x7fffffu;
    if (bits < 0x00800000u) {                   // subnormal: normalise
        const int lz = __clz(man) - 8;          // shifts that bring the leading one to bit 23
        e = -126 - lz;
        man = (man << lz) & 0x7fffffu;
    }
    return man == 0 ? 14 - e : 13 - e;
}

// float32(2.0 ** k) as the eager path's `weight * (2.0 ** k)` uses it (the Python float becomes a float32 scalar)
__device__ __forceinline__ float split_scale(int k) { return (float)ldexp(1.0, k); }

__device__ __forceinline__ void split_one(float w, float scale, __half &hi, __half &lo)
{
#pragma clang fp contract(off)
    const float ws = w * scale;
    hi = __float2half_rn(ws);
    lo = __float2half_rn(ws - __half2float(hi));
}

struct alignas(16) Half8 {
    __half h[8];
};

__global__ __launch_bounds__(PREP_THREADS) void prep_split_kernel(const PrepArgs a)
{
    const int t = threadIdx.x;
    const int li = first_run_above(a.block_end, a.n, blockIdx.x);
    const srcnn_prep_layer &L = a.l[li];
    const int unit = blockIdx.x - (li ? a.block_end[li - 1] : 0);
    const int g = a.layer_base + li;
    const int k = split_exponent(a.maxbits[L.alias_of >= 0 ? L.alias_of : g]);
    if (unit == 0 && t == 0) a.k_out[g] = k;
    if (!L.dst_hi) return;
    const float scale = split_scale(k);
    const long long numel = (long long)prep_rows(L) * prep_row_len(L);
    const int wchunks = (int)((numel + PREP_TILE - 1) / PREP_TILE);
    const float *w = L.dst_w;
    if (unit < wchunks) {
        __half *hi = static_cast<__half *>(L.dst_hi), *lo = static_cast<__half *>(L.dst_lo);
        const long long base = (long long)unit * PREP_TILE;
        const int left = (int)min((long long)PREP_TILE, numel - base);
        for (int e = t * 8; e < left; e += PREP_THREADS * 8) {
            if ((a.vec[li] & PREP_VEC_OUT) && e + 8 <= left) {          // 16 bytes of hi and of lo per lane
                const float4 v0 = *reinterpret_cast<const float4 *>(w + base + e), v1 = *reinterpret_cast<const float4 *>(w + base + e + 4);
                const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                Half8 h, l;
#pragma unroll
                for (int q = 0; q < 8; ++q) split_one(v[q], scale, h.h[q], l.h[q]);
                *reinterpret_cast<Half8 *>(hi + base + e) = h;
                *reinterpret_cast<Half8 *>(lo + base + e) = l;
            } else {
                for (int q = 0; q < 8 && e + q < left; ++q) split_one(w[base + e + q], scale, hi[base + e + q], lo[base + e + q]);
            }
        }
        return;
    }
    // head_fragments: (C / 16 steps, hi | lo, k group 0 | 1, frag_rows, 8 halves), element (s, h, g, n, i) = W_h[n][16 s + 8 g + i],
    // rows n >= Cout zero.  One lane = one run of 8 halves.
    const int C = (int)prep_row_len(L), n2 = prep_rows(L), FR = L.frag_rows;
    const long long runs = (long long)(C / 16) * 4 * FR;
    __half *frag = static_cast<__half *>(L.dst_frag);
    const long long rbase = (long long)(unit - wchunks) * (PREP_TILE / 8);
    for (long long r = rbase + t; r < min(runs, rbase + PREP_TILE / 8); r += PREP_THREADS) {
        const int n = (int)(r % FR);
        const long long r1 = r / FR;
        const int kg = (int)(r1 & 1), h = (int)((r1 >> 1) & 1), s = (int)(r1 >> 2);
        Half8 out;
#pragma unroll
        for (int q = 0; q < 8; ++q) out.h[q] = __float2half_rn(0.f);
        if (n < n2) {
            const float *src = w + (size_t)n * C + 16 * s + 8 * kg;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                __half vh, vl;
                split_one(src[q], scale, vh, vl);
                out.h[q] = h ? vl : vh;
            }
        }
        if (a.vec[li] & PREP_VEC_OUT) *reinterpret_cast<Half8 *>(frag + r * 8) = out;
        else
            for (int q = 0; q < 8; ++q) frag[r * 8 + q] = out.h[q];
    }
}

// nullptr, or what is wrong with layer i of the list
static const char *check_layer(const srcnn_prep_layer *all, int i)
{
    const srcnn_prep_layer &L = all[i];
    if (L.form < SRCNN_PREP_CONV || L.form > SRCNN_PREP_DECONV2X2) return "unknown form (SRCNN_PREP_*)";
    if (!L.dst_w) return "null dst_w";
    if ((L.dst_hi == nullptr) != (L.dst_lo == nullptr)) return "dst_hi and dst_lo go together";
    if (L.dst_frag && !L.dst_hi) return "dst_frag needs dst_hi / dst_lo";
    if (!aligned_to(L.dst_w, 4) || !aligned_to(L.dst_b, 4) || !aligned_to(L.dst_hi, 2) || !aligned_to(L.dst_lo, 2)
        || !aligned_to(L.dst_frag, 2))
        return "misaligned destination";
    const int nsrc_want = L.form == SRCNN_PREP_SHORTCUT ? 2 : (L.form == SRCNN_PREP_CONV ? 0 : 1);
    if (L.n_src < 1 || L.n_src > 3 || (nsrc_want && L.n_src != nsrc_want)) return "n_src does not fit the form";
    if (L.cin < 1) return "cin must be >= 1";
    for (int s = 0; s < L.n_src; ++s)
        if (L.cout[s] < 1) return "cout must be >= 1";
    const bool bn0 = L.bn_g[0] != nullptr, bn1 = L.bn_g[1] != nullptr;
    for (int q = 0; q < 2; ++q) {
        const bool any = L.bn_g[q] || L.bn_b[q] || L.bn_m[q] || L.bn_v[q], all4 = L.bn_g[q] && L.bn_b[q] && L.bn_m[q] && L.bn_v[q];
        if (any && !all4) return "a frozen BN needs all of weight, bias, running_mean, running_var";
    }
    switch (L.form) {
    case SRCNN_PREP_CONV:
        if (L.kh < 1 || L.kw < 1 || L.kh * L.kw > PREP_TILE) return "kernel size out of range";
        if (L.cin2 != 0) return "cin2 belongs to the shortcut form";
        if (bn1 || (bn0 && L.n_src != 1)) return "a frozen BN folds into a single source";
        break;
    case SRCNN_PREP_SHORTCUT:
        if (L.kh != 1 || L.kw != 1) return "the shortcut form is 1x1";
        if (L.cin2 < 1) return "the shortcut form needs cin2";
        if (L.cout[0] != L.cout[1]) return "size mismatch: both sources of the shortcut form have Cout rows";
        if (!bn0 || !bn1) return "the shortcut form folds two frozen BNs";
        break;
    case SRCNN_PREP_STEM:
        if (L.kh != 7 || L.kw != 7 || L.cin != 3) return "the stem form is 7x7 over 3 channels";
        if (L.cin2 != 0) return "cin2 belongs to the shortcut form";
        if (!bn0 || bn1) return "the stem form folds one frozen BN";
        break;
    default:
        if (L.kh != 2 || L.kw != 2) return "the deconvolution form is 2x2";
        if (L.cin2 != 0) return "cin2 belongs to the shortcut form";
        if (bn0 || bn1) return "the deconvolution form has no BN";
        if (!L.b[0] || !L.dst_b) return "the deconvolution form carries a bias";
    }
    if (L.alias_of >= 0) {
        if (L.alias_of >= i) return "alias_of must name an earlier layer of the list";
        const srcnn_prep_layer &O = all[L.alias_of];
        if (O.alias_of >= 0 || O.dst_w != L.dst_w || O.form != L.form || prep_rows(O) != prep_rows(L) || prep_row_len(O) != prep_row_len(L))
            return "size mismatch: an alias shares dst_w and the shape of the layer it names";
    } else {
        for (int s = 0; s < L.n_src; ++s) {
            if (!L.w[s]) return "null source weight";
            if (!aligned_to(L.w[s], 4) || !aligned_to(L.b[s], 4)) return "misaligned source";
        }
        if (L.form == SRCNN_PREP_CONV && !bn0) {
            for (int s = 1; s < L.n_src; ++s)
                if ((L.b[s] != nullptr) != (L.b[0] != nullptr)) return "size mismatch: every source carries a bias, or none";
            if ((L.b[0] != nullptr) != (L.dst_b != nullptr)) return "dst_b goes with the sources' bias";
        } else if (L.form != SRCNN_PREP_DECONV2X2 && !L.dst_b) {
            return "null dst_b (a folded BN leaves a bias)";
        }
    }
    const long long numel = (long long)prep_rows(L) * prep_row_len(L);
    if (numel >= (1ll << 31)) return "a layer of 2^31 elements or more";
    if (L.dst_frag) {
        if (prep_taps(L) != 1 || L.form != SRCNN_PREP_CONV || L.cin % 16 != 0) return "fragments: a 1x1 layer with Cin a multiple of 16";
        if (L.frag_rows < prep_rows(L) || L.frag_rows % 8 != 0) return "size mismatch: frag_rows is Cout rounded up to a multiple of 8";
    }
    return nullptr;
}

}  // namespace srcnn

extern "C" {

size_t srcnn_prep_weights_workspace_bytes(int n_layers)
{
    return n_layers > 0 ? srcnn::align_up((size_t)n_layers * sizeof(unsigned), 256) : 0;
}

int srcnn_prep_weights(const srcnn_prep_layer *layers_host, int n_layers, int *k_out, void *workspace, size_t workspace_bytes,
                       srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(layers_host, "null layers_host");
    SRCNN_REQUIRE(n_layers >= 1, "n_layers must be >= 1");
    SRCNN_REQUIRE(k_out && workspace, "null k_out / workspace");
    SRCNN_REQUIRE(aligned_to(k_out, 4) && aligned_to(workspace, 4), "k_out / workspace not 4-byte aligned");
    for (int i = 0; i < n_layers; ++i) {
        const char *m = check_layer(layers_host, i);
        if (m) {
            set_error("srcnn_prep_weights: layer %d: %s", i, m);
            return SRCNN_ERR_ARG;
        }
    }
    if (workspace_bytes < srcnn_prep_weights_workspace_bytes(n_layers)) {
        set_error("srcnn_prep_weights: workspace too small (srcnn_prep_weights_workspace_bytes)");
        return SRCNN_ERR_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    unsigned *maxbits = static_cast<unsigned *>(workspace);
    SRCNN_HIP_TRY(memset_async(maxbits, 0, (size_t)n_layers * sizeof(unsigned), st));
    for (int pass = 0; pass < 2; ++pass) {
        for (int base = 0; base < n_layers; base += PREP_LPL) {
            PrepArgs a;
            a.n = n_layers - base < PREP_LPL ? n_layers - base : PREP_LPL;
            a.layer_base = base, a.maxbits = maxbits, a.k_out = k_out;
            long long blocks = 0;
            for (int i = 0; i < a.n; ++i) {
                const srcnn_prep_layer &L = a.l[i] = layers_host[base + i];
                const int rows = prep_rows(L), chan = prep_chan(L), T = prep_taps(L);
                int cc = PREP_TILE / T < chan ? PREP_TILE / T : chan;
                if (cc < chan && cc >= 4) cc &= ~3;
                int rb = 1;
                if (cc == chan) {
                    const int per_row = L.form == SRCNN_PREP_STEM ? 224 : chan * T;       // the stem's units are sized by their destination rows
                    rb = PREP_TILE / per_row;
                    rb = rb < 1 ? 1 : rb > PREP_MAX_RB ? PREP_MAX_RB : rb;
                    if (rb > rows) rb = rows;
                }
                a.rb[i] = (short)rb, a.cc[i] = (short)cc;
                bool in16 = L.alias_of < 0, out16 = aligned_to(L.dst_w, 16) && aligned_to(L.dst_hi, 16) && aligned_to(L.dst_lo, 16)
                                                   && aligned_to(L.dst_frag, 16);
                for (int s = 0; s < L.n_src && in16; ++s) in16 = aligned_to(L.w[s], 16);
                if (L.form == SRCNN_PREP_SHORTCUT) {
                    in16 = in16 && L.cin % 4 == 0 && L.cin2 % 4 == 0 && cc % 4 == 0;
                    out16 = out16 && L.cin % 4 == 0 && L.cin2 % 4 == 0 && cc % 4 == 0;
                } else if (L.form == SRCNN_PREP_STEM) {
                    in16 = false;                                                         // rows of 147 floats
                } else {
                    in16 = in16 && (chan * T) % 4 == 0 && (cc * T) % 4 == 0;
                    out16 = out16 && chan % 4 == 0 && cc % 4 == 0;
                }
                a.vec[i] = (unsigned char)((in16 ? PREP_VEC_IN : 0) | (out16 ? PREP_VEC_OUT : 0));
                if (pass == 0) {
                    if (L.alias_of < 0) blocks += (long long)cdiv(rows, rb) * cdiv(chan, cc);
                } else {
                    const long long numel = (long long)rows * prep_row_len(L);
                    long long b = 1;
                    if (L.dst_hi) {
                        b = (numel + PREP_TILE - 1) / PREP_TILE;
                        if (L.dst_frag) b += ((long long)(L.cin / 16) * 4 * L.frag_rows + PREP_TILE / 8 - 1) / (PREP_TILE / 8);
                    }
                    blocks += b;
                }
                a.block_end[i] = (int)blocks;
            }
            if (blocks == 0) continue;              // (pass A over aliases only)
            if (pass == 0) SRCNN_LAUNCH(prep_fold_kernel, (unsigned)blocks, PREP_THREADS, 0, st, a);
            else SRCNN_LAUNCH(prep_split_kernel, (unsigned)blocks, PREP_THREADS, 0, st, a);
        }
    }
    return check_launch("srcnn_prep_weights");
}

}  // extern "C"
