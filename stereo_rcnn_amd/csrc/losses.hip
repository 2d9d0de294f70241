// Training losses (gfx950): cross-entropy over rows and smooth L1, forward and backward, fused.
//
// Reference: lib/model/rpn/stereo_rpn.py:113-136, lib/model/stereo_rcnn/stereo_rcnn.py:274-311 and _smooth_l1_loss in
// lib/model/utils/net_utils.py:79-99 -- about thirty eager tensor operations per step, one nonzero() and three
// `torch.sum(weight).data[0] < 1` reads that make the host wait for the device.  Here each family is a forward of two launches
// (per-workgroup partials, then one workgroup that adds them) and a backward of one elementwise launch; the ignore rule, the
// `W < 1` rule and the class-slice selection are evaluated on the device and nothing is ever read back.
//
// DEFINED SUMMATION ORDER (include/srcnn_hip.h states it for callers): no atomics, the same bits on every run.
//   stage 1  workgroup b owns rows [b * RPW, (b + 1) * RPW), RPW = SRCNN_LOSS_ROWS_PER_WG, 256 threads:
//            every thread adds its (at most 4, smooth L1: 4 groups of D) terms in ascending row order starting from 0, a wavefront
//            adds its 64 lanes with an xor butterfly (offsets 32, 16, .. 1; a + b == b + a, so all lanes agree), thread 0 adds
//            the four wavefront sums ((w0 + w1) + w2) + w3 and writes the pair {sum, normaliser sum} to workspace[b];
//   stage 2  one workgroup: thread t adds workspace[t], workspace[t + 256], .. in that order starting from 0, then the same
//            butterfly and the same four-term sum; thread 0 normalises and writes the loss and the normaliser.
#include "common.h"

namespace srcnn {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_RPW = SRCNN_LOSS_ROWS_PER_WG;        // rows of a stage-1 workgroup: fixed, whatever the device
constexpr int LOSS_PER_THREAD = LOSS_RPW / LOSS_THREADS;
constexpr int CE_VPL = SRCNN_CE_MAX_COLS / 64;          // logits a lane holds when a row spans a whole wavefront
static_assert(LOSS_RPW % LOSS_THREADS == 0 && LOSS_THREADS == 256 && CE_VPL * 64 == SRCNN_CE_MAX_COLS, "loss tiling");

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// the sum of (a, b) over the workgroup, valid in thread 0 (fixed order: lanes by butterfly, then wavefronts 0..3)
__device__ __forceinline__ void block_sum2(float &a, float &b)
{
    __shared__ float red[LOSS_THREADS / 64][2];
    a = wave_sum(a);
    b = wave_sum(b);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) red[tid >> 6][0] = a, red[tid >> 6][1] = b;
    __syncthreads();
    if (tid == 0) {
        a = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        b = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
}

// what the forward divides by and the backward divides by again, from the normaliser sum n the forward left on the device
__device__ __forceinline__ float effective_norm(int mode, float n)
{
    if (mode == SRCNN_CE_WEIGHTED) return n < 1.0f ? 1.0f : n;      // stereo_rcnn.py:295-298: `if sum(w) < 1` on the device
    return n > 0.0f ? n : 1.0f;                                      // nothing kept: loss 0, gradient 0 (not NaN)
}

// stage 2 of both families.  mode < 0: smooth L1, the normaliser is the host's divisor.
__global__ __launch_bounds__(LOSS_THREADS) void loss_finish_kernel(const float2 *__restrict__ partial, long long count, int mode,
                                                                    float divisor, float *__restrict__ loss, float *__restrict__ norm)
{
    float s = 0.0f, n = 0.0f;
    for (long long i = threadIdx.x; i < count; i += LOSS_THREADS) {
        const float2 p = partial[i];
        s = s + p.x, n = n + p.y;
    }
    block_sum2(s, n);
    if (threadIdx.x == 0) {
        if (mode < 0) n = divisor;
        *loss = s / (mode < 0 ? n : effective_norm(mode, n));
        *norm = n;
    }
}

// ---------------------------------------------------------------------------------------------------------- cross-entropy
// A row's loss is log(sum_c exp(x_c - m)) + (m - x_label) with m the row maximum; the first maximum's own term is exactly 1,
// so the logarithm is log1p of the OTHER terms: a confident row (loss ~ 1e-6) keeps its relative accuracy.
struct CeSoft {
    float m, s1;        // row maximum; sum of exp(x_c - m) over every column but the first maximum
    int arg;            // column of the first maximum
};

// cols == 2: one row per lane.  VEC: the row is read as one float2 (even stride, 8-byte aligned base).
template <bool VEC>
__device__ __forceinline__ void ce_load2(const float *p, float &x0, float &x1)
{
    if (VEC) {
        const float2 v = *reinterpret_cast<const float2 *>(p);
        x0 = v.x, x1 = v.y;
    } else {
        x0 = p[0], x1 = p[1];
    }
}

template <bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void ce2_forward_kernel(const float *__restrict__ x, long long rows, long long stride,
                                                                    const int *__restrict__ labels, const float *__restrict__ weights,
                                                                    float2 *__restrict__ partial)
{
    const long long row0 = (long long)blockIdx.x * LOSS_RPW;
    float s = 0.0f, n = 0.0f;
#pragma unroll
    for (int j = 0; j < LOSS_PER_THREAD; ++j) {
        const long long r = row0 + j * LOSS_THREADS + threadIdx.x;
        if (r >= rows) continue;
        const int label = labels[r];
        if (label < 0 || label >= 2) continue;                           // ignored: never an index, nothing loaded
        float x0, x1;
        ce_load2<VEC>(x + (size_t)r * (size_t)stride, x0, x1);
        const float m = fmaxf(x0, x1);
        const float l = log1pf(expf(-fabsf(x0 - x1))) + (m - (label ? x1 : x0));
        const float w = weights ? weights[r] : 1.0f;
        s = s + l * w, n = n + w;
    }
    block_sum2(s, n);
    if (threadIdx.x == 0) partial[blockIdx.x] = make_float2(s, n);
}

template <bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void ce2_backward_kernel(const float *__restrict__ x, long long rows, long long stride,
                                                                     const int *__restrict__ labels, const float *__restrict__ weights,
                                                                     int mode, const float *__restrict__ norm,
                                                                     const float *__restrict__ upstream, float *__restrict__ grad,
                                                                     long long grad_stride)
{
    const long long row0 = (long long)blockIdx.x * LOSS_RPW;
    const float scale = *upstream / effective_norm(mode, *norm);
#pragma unroll
    for (int j = 0; j < LOSS_PER_THREAD; ++j) {
        const long long r = row0 + j * LOSS_THREADS + threadIdx.x;
        if (r >= rows) continue;
        const int label = labels[r];
        float g0 = 0.0f, g1 = 0.0f;
        if (label >= 0 && label < 2) {
            float x0, x1;
            ce_load2<VEC>(x + (size_t)r * (size_t)stride, x0, x1);
            const float m = fmaxf(x0, x1);
            const float e0 = expf(x0 - m), e1 = expf(x1 - m), sum = e0 + e1;
            const float c = (weights ? weights[r] : 1.0f) * scale;
            g0 = (e0 / sum - (label == 0 ? 1.0f : 0.0f)) * c;
            g1 = (e1 / sum - (label == 1 ? 1.0f : 0.0f)) * c;
        }
        float *g = grad + (size_t)r * (size_t)grad_stride;
        if (VEC) *reinterpret_cast<float2 *>(g) = make_float2(g0, g1);
        else g[0] = g0, g[1] = g1;
    }
}

// cols != 2: a row lies on `lpr` adjacent lanes (a power of two, 2..64), lane `sub` of them holding columns sub, sub + lpr, ..;
// pass p of a workgroup takes rows p * (256 / lpr) + group.  Every shuffle is executed by all lanes; rows that are out of
// range or ignored load nothing and their values are discarded by a select.
__device__ __forceinline__ CeSoft ce_row_soft(const float (&v)[CE_VPL], int sub, int lpr, int cols)
{
    CeSoft r;
    r.m = -INFINITY;
#pragma unroll
    for (int k = 0; k < CE_VPL; ++k) r.m = fmaxf(r.m, v[k]);
    for (int o = lpr >> 1; o > 0; o >>= 1) r.m = fmaxf(r.m, __shfl_xor(r.m, o, 64));
    r.arg = 0x7fffffff;
#pragma unroll
    for (int k = CE_VPL - 1; k >= 0; --k)
        if (sub + k * lpr < cols && v[k] == r.m) r.arg = sub + k * lpr;
    for (int o = lpr >> 1; o > 0; o >>= 1) r.arg = min(r.arg, __shfl_xor(r.arg, o, 64));
    r.s1 = 0.0f;
#pragma unroll
    for (int k = 0; k < CE_VPL; ++k) {
        const int c = sub + k * lpr;
        if (c < cols && c != r.arg) r.s1 = r.s1 + expf(v[k] - r.m);
    }
    for (int o = lpr >> 1; o > 0; o >>= 1) r.s1 = r.s1 + __shfl_xor(r.s1, o, 64);
    return r;
}

__global__ __launch_bounds__(LOSS_THREADS) void ce_forward_kernel(const float *__restrict__ x, long long rows, int cols,
                                                                   long long stride, int lpr, const int *__restrict__ labels,
                                                                   const float *__restrict__ weights, float2 *__restrict__ partial)
{
    const long long row0 = (long long)blockIdx.x * LOSS_RPW;
    const int tid = threadIdx.x, sub = tid & (lpr - 1), group = tid / lpr, groups = LOSS_THREADS / lpr;
    float s = 0.0f, n = 0.0f;
    for (int p = 0; p < LOSS_RPW / groups; ++p) {
        if (row0 + p * groups >= rows) break;                             // (uniform) the workgroup's last rows lie behind
        const long long r = row0 + p * groups + group;
        const int label = r < rows ? labels[r] : -1;
        const bool kept = label >= 0 && label < cols;
        float v[CE_VPL];
#pragma unroll
        for (int k = 0; k < CE_VPL; ++k) {
            const int c = sub + k * lpr;
            v[k] = kept && c < cols ? x[(size_t)r * (size_t)stride + c] : -INFINITY;
        }
        const CeSoft soft = ce_row_soft(v, sub, lpr, cols);
        float xl = 0.0f;                                                  // x_label: one lane holds it, the others add 0
#pragma unroll
        for (int k = 0; k < CE_VPL; ++k)
            if (sub + k * lpr == label) xl = v[k];
        for (int o = lpr >> 1; o > 0; o >>= 1) xl = xl + __shfl_xor(xl, o, 64);
        // the row's lanes all hold its loss; lane p mod lpr of them carries it into the sum, so that a lane adds at most
        // LOSS_PER_THREAD rows whatever lpr is
        if (kept && sub == (p & (lpr - 1))) {
            const float l = log1pf(soft.s1) + (soft.m - xl);
            const float w = weights ? weights[r] : 1.0f;
            s = s + l * w, n = n + w;
        }
    }
    block_sum2(s, n);
    if (tid == 0) partial[blockIdx.x] = make_float2(s, n);
}

__global__ __launch_bounds__(LOSS_THREADS) void ce_backward_kernel(const float *__restrict__ x, long long rows, int cols,
                                                                    long long stride, int lpr, const int *__restrict__ labels,
                                                                    const float *__restrict__ weights, int mode,
                                                                    const float *__restrict__ norm, const float *__restrict__ upstream,
                                                                    float *__restrict__ grad, long long grad_stride)
{
    const long long row0 = (long long)blockIdx.x * LOSS_RPW;
    const int tid = threadIdx.x, sub = tid & (lpr - 1), group = tid / lpr, groups = LOSS_THREADS / lpr;
    const float scale = *upstream / effective_norm(mode, *norm);
    for (int p = 0; p < LOSS_RPW / groups; ++p) {
        if (row0 + p * groups >= rows) break;
        const long long r = row0 + p * groups + group;
        const bool live = r < rows;
        const int label = live ? labels[r] : -1;
        const bool kept = label >= 0 && label < cols;
        float v[CE_VPL];
#pragma unroll
        for (int k = 0; k < CE_VPL; ++k) {
            const int c = sub + k * lpr;
            v[k] = kept && c < cols ? x[(size_t)r * (size_t)stride + c] : -INFINITY;
        }
        const CeSoft soft = ce_row_soft(v, sub, lpr, cols);
        const float sum = 1.0f + soft.s1;
        const float coef = kept ? (weights ? weights[r] : 1.0f) * scale : 0.0f;
#pragma unroll
        for (int k = 0; k < CE_VPL; ++k) {
            const int c = sub + k * lpr;
            if (live && c < cols)
                grad[(size_t)r * (size_t)grad_stride + c] = kept ? (expf(v[k] - soft.m) / sum - (c == label ? 1.0f : 0.0f)) * coef : 0.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- smooth L1
struct SmoothL1Args {
    const float *pred, *target, *w_in, *w_out;
    const int *selector;
    long long rows;
    int D, n_sel, w_in_per_row, w_out_per_row;
    float thr, half_s2, lin_off, s2;       // (float)(1 / sigma^2), (float)(sigma^2 / 2), (float)(0.5 / sigma^2), (float)sigma^2
};

// d = w_in * (pred - target) of element (row r, column c) and its outside weight; false: the row's selector is out of range
__device__ __forceinline__ bool smooth_l1_diff(const SmoothL1Args &a, long long r, int c, float &d, float &win, float &wout)
{
    int sel = 0;
    if (a.selector) {
        sel = a.selector[r];
        if (sel < 0 || sel >= a.n_sel) return false;
    }
    const size_t e = (size_t)r * a.D + c;
    win = a.w_in ? (a.w_in_per_row ? a.w_in[r] : a.w_in[e]) : 1.0f;
    wout = a.w_out ? (a.w_out_per_row ? a.w_out[r] : a.w_out[e]) : 1.0f;
    d = a.pred[((size_t)r * a.n_sel + sel) * a.D + c] - a.target[e];
    if (a.w_in) d = win * d;
    return true;
}

// Workgroup b owns the RPW * D elements of its rows; thread t takes local elements t, t + 256, ..: 4 groups of D terms, a
// group added in ascending order from 0, the 4 group sums added in ascending order from 0.
__global__ __launch_bounds__(LOSS_THREADS) void smooth_l1_forward_kernel(SmoothL1Args a, float2 *__restrict__ partial)
{
    const long long row0 = (long long)blockIdx.x * LOSS_RPW;
    const unsigned D = a.D;
    float s = 0.0f;
    for (int j = 0; j < LOSS_PER_THREAD; ++j) {
        float sj = 0.0f;
        for (unsigned q = 0; q < D; ++q) {
            const unsigned i = (j * D + q) * LOSS_THREADS + threadIdx.x;      // < RPW * D <= 2^16
            const unsigned lr = i / D;
            const long long r = row0 + lr;
            if (r >= a.rows) continue;
            float d, win, wout;
            if (!smooth_l1_diff(a, r, (int)(i - lr * D), d, win, wout)) continue;
            const float ad = fabsf(d);
            float v = ad < a.thr ? (d * d) * a.half_s2 : ad - a.lin_off;      // net_utils.py:88-90
            if (a.w_out) v = wout * v;
            sj = sj + v;
        }
        s = s + sj;
    }
    float n = 0.0f;
    block_sum2(s, n);
    if (threadIdx.x == 0) partial[blockIdx.x] = make_float2(s, 0.0f);
}

// every element of the (rows, n_sel * D) gradient: zeros in the slices the selector does not pick
__global__ __launch_bounds__(LOSS_THREADS) void smooth_l1_backward_kernel(SmoothL1Args a, const float *__restrict__ norm,
                                                                           const float *__restrict__ upstream, float *__restrict__ grad)
{
    const long long row0 = (long long)blockIdx.x * LOSS_RPW;
    const unsigned D = a.D, width = a.n_sel * D;                              // width <= 2^20: RPW * width fits 32 bits
    const float scale = *upstream / *norm;
    const long long left = a.rows - row0;
    const unsigned count = (unsigned)(left < LOSS_RPW ? left : LOSS_RPW) * width;
    for (unsigned i = threadIdx.x; i < count; i += LOSS_THREADS) {
        const unsigned lr = i / width, col = i - lr * width, sel = col / D;
        const long long r = row0 + lr;
        float g = 0.0f, d, win, wout;
        const int want = a.selector ? a.selector[r] : 0;
        if ((int)sel == want && smooth_l1_diff(a, r, (int)(col - sel * D), d, win, wout)) {
            g = fabsf(d) < a.thr ? a.s2 * d : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
            if (a.w_in) g = g * win;
            if (a.w_out) g = g * wout;
            g = g * scale;
        }
        grad[(size_t)r * width + col] = g;
    }
}

static size_t loss_partials(long long rows) { return (size_t)((rows + LOSS_RPW - 1) / LOSS_RPW); }

static int ce_lanes_per_row(int cols)
{
    int lpr = 2;
    while (lpr < cols && lpr < 64) lpr *= 2;
    return lpr;
}


static int smooth_l1_args(SmoothL1Args &a, const char *who, const float *pred, const int *selector, int n_sel, const float *target,
                          const float *w_in, int w_in_per_row, const float *w_out, int w_out_per_row, long long rows, int D, float sigma)
{
    if (!(rows >= 0 && D >= 1 && D <= SRCNN_SMOOTH_L1_MAX_D && n_sel >= 1 && n_sel <= SRCNN_SMOOTH_L1_MAX_SEL)) {
        set_error("%s: rows must be >= 0, D 1..%d, n_sel 1..%d", who, SRCNN_SMOOTH_L1_MAX_D, SRCNN_SMOOTH_L1_MAX_SEL);
        return SRCNN_ERR_ARG;
    }
    if (!selector && n_sel != 1) {
        set_error("%s: n_sel > 1 needs a selector", who);
        return SRCNN_ERR_ARG;
    }
    if (!(sigma > 0.0f)) {
        set_error("%s: sigma must be > 0", who);
        return SRCNN_ERR_ARG;
    }
    if (rows > 0 && (!pred || !target)) {
        set_error("%s: null pred / target", who);
        return SRCNN_ERR_ARG;
    }
    const double s2 = (double)sigma * (double)sigma;
    a.pred = pred, a.target = target, a.w_in = w_in, a.w_out = w_out, a.selector = selector;
    a.rows = rows, a.D = D, a.n_sel = n_sel, a.w_in_per_row = w_in_per_row, a.w_out_per_row = w_out_per_row;
    a.thr = (float)(1.0 / s2), a.half_s2 = (float)(s2 / 2.0), a.lin_off = (float)(0.5 / s2), a.s2 = (float)s2;
    return SRCNN_OK;
}

}  // namespace srcnn

extern "C" {

size_t srcnn_loss_workspace_bytes(long long rows)
{
    using namespace srcnn;
    if (rows < 0) return 0;
    return align_up((loss_partials(rows) > 0 ? loss_partials(rows) : 1) * sizeof(float2), 256);
}

int srcnn_cross_entropy(const float *logits, long long rows, int cols, long long row_stride, const int *labels, const float *weights,
                        int mode, float *loss_out, float *norm_out, void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(rows >= 0, "rows must be >= 0");
    SRCNN_REQUIRE(cols >= 1 && cols <= SRCNN_CE_MAX_COLS, "cols must be 1..256 (SRCNN_CE_MAX_COLS)");
    SRCNN_REQUIRE(row_stride >= cols, "row stride smaller than cols");
    SRCNN_REQUIRE(mode == SRCNN_CE_MEAN_KEPT || mode == SRCNN_CE_WEIGHTED, "mode must be SRCNN_CE_MEAN_KEPT or SRCNN_CE_WEIGHTED");
    SRCNN_REQUIRE(loss_out && norm_out && workspace, "null loss_out / norm_out / workspace");
    SRCNN_REQUIRE(rows == 0 || (logits && labels), "null logits / labels");
    SRCNN_REQUIRE(rows <= (long long)LOSS_RPW * 0x7fffffffLL, "too many rows");
    if (workspace_bytes < srcnn_loss_workspace_bytes(rows)) {
        set_error("srcnn_cross_entropy: workspace too small (srcnn_loss_workspace_bytes)");
        return SRCNN_ERR_WORKSPACE;
    }
    float2 *partial = static_cast<float2 *>(workspace);
    const size_t blocks = loss_partials(rows);
    hipStream_t st = as_stream(stream);
    if (blocks > 0) {
        if (cols == 2) {
            if (row_stride % 2 == 0 && aligned_to(logits, 8))
                SRCNN_LAUNCH(ce2_forward_kernel<true>, (unsigned)blocks, LOSS_THREADS, 0, st, logits, rows, row_stride, labels, weights, partial);
            else
                SRCNN_LAUNCH(ce2_forward_kernel<false>, (unsigned)blocks, LOSS_THREADS, 0, st, logits, rows, row_stride, labels, weights, partial);
        } else {
            SRCNN_LAUNCH(ce_forward_kernel, (unsigned)blocks, LOSS_THREADS, 0, st, logits, rows, cols, row_stride, ce_lanes_per_row(cols),
                         labels, weights, partial);
        }
    }
    SRCNN_LAUNCH(loss_finish_kernel, 1, LOSS_THREADS, 0, st, (const float2 *)partial, (long long)blocks, mode, 0.0f, loss_out, norm_out);
    return check_launch("srcnn_cross_entropy");
}

int srcnn_cross_entropy_backward(const float *logits, long long rows, int cols, long long row_stride, const int *labels,
                                 const float *weights, int mode, const float *norm, const float *grad_loss, float *grad_logits,
                                 long long grad_stride, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(rows >= 0, "rows must be >= 0");
    SRCNN_REQUIRE(cols >= 1 && cols <= SRCNN_CE_MAX_COLS, "cols must be 1..256 (SRCNN_CE_MAX_COLS)");
    SRCNN_REQUIRE(row_stride >= cols && grad_stride >= cols, "row stride smaller than cols");
    SRCNN_REQUIRE(mode == SRCNN_CE_MEAN_KEPT || mode == SRCNN_CE_WEIGHTED, "mode must be SRCNN_CE_MEAN_KEPT or SRCNN_CE_WEIGHTED");
    SRCNN_REQUIRE(norm && grad_loss, "null norm / grad_loss");
    SRCNN_REQUIRE(rows == 0 || (logits && labels && grad_logits), "null logits / labels / grad_logits");
    SRCNN_REQUIRE(rows <= (long long)LOSS_RPW * 0x7fffffffLL, "too many rows");
    const size_t blocks = loss_partials(rows);
    if (blocks == 0) return SRCNN_OK;
    hipStream_t st = as_stream(stream);
    if (cols == 2) {
        if (row_stride % 2 == 0 && grad_stride % 2 == 0 && aligned_to(logits, 8) && aligned_to(grad_logits, 8))
            SRCNN_LAUNCH(ce2_backward_kernel<true>, (unsigned)blocks, LOSS_THREADS, 0, st, logits, rows, row_stride, labels, weights, mode, norm,
                         grad_loss, grad_logits, grad_stride);
        else
            SRCNN_LAUNCH(ce2_backward_kernel<false>, (unsigned)blocks, LOSS_THREADS, 0, st, logits, rows, row_stride, labels, weights, mode, norm,
                         grad_loss, grad_logits, grad_stride);
    } else {
        SRCNN_LAUNCH(ce_backward_kernel, (unsigned)blocks, LOSS_THREADS, 0, st, logits, rows, cols, row_stride, ce_lanes_per_row(cols), labels,
                     weights, mode, norm, grad_loss, grad_logits, grad_stride);
    }
    return check_launch("srcnn_cross_entropy_backward");
}

int srcnn_smooth_l1(const float *pred, const int *selector, int n_sel, const float *target, const float *w_in, int w_in_per_row,
                    const float *w_out, int w_out_per_row, long long rows, int D, float sigma, float divisor, float *loss_out,
                    float *norm_out, void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    using namespace srcnn;
    SmoothL1Args a;
    const int rc = smooth_l1_args(a, "srcnn_smooth_l1", pred, selector, n_sel, target, w_in, w_in_per_row, w_out, w_out_per_row, rows, D, sigma);
    if (rc != SRCNN_OK) return rc;
    SRCNN_REQUIRE(divisor > 0.0f, "divisor must be > 0");
    SRCNN_REQUIRE(loss_out && norm_out && workspace, "null loss_out / norm_out / workspace");
    SRCNN_REQUIRE(rows <= (long long)LOSS_RPW * 0x7fffffffLL, "too many rows");
    if (workspace_bytes < srcnn_loss_workspace_bytes(rows)) {
        set_error("srcnn_smooth_l1: workspace too small (srcnn_loss_workspace_bytes)");
        return SRCNN_ERR_WORKSPACE;
    }
    float2 *partial = static_cast<float2 *>(workspace);
    const size_t blocks = loss_partials(rows);
    hipStream_t st = as_stream(stream);
    if (blocks > 0) SRCNN_LAUNCH(smooth_l1_forward_kernel, (unsigned)blocks, LOSS_THREADS, 0, st, a, partial);
    SRCNN_LAUNCH(loss_finish_kernel, 1, LOSS_THREADS, 0, st, (const float2 *)partial, (long long)blocks, -1, divisor, loss_out, norm_out);
    return check_launch("srcnn_smooth_l1");
}

int srcnn_smooth_l1_backward(const float *pred, const int *selector, int n_sel, const float *target, const float *w_in, int w_in_per_row,
                             const float *w_out, int w_out_per_row, long long rows, int D, float sigma, const float *norm,
                             const float *grad_loss, float *grad_pred, srcnn_stream_t stream)
{
    using namespace srcnn;
    SmoothL1Args a;
    const int rc = smooth_l1_args(a, "srcnn_smooth_l1_backward", pred, selector, n_sel, target, w_in, w_in_per_row, w_out, w_out_per_row, rows,
                                  D, sigma);
    if (rc != SRCNN_OK) return rc;
    SRCNN_REQUIRE(norm && grad_loss, "null norm / grad_loss");
    SRCNN_REQUIRE(rows == 0 || grad_pred, "null grad_pred");
    SRCNN_REQUIRE(rows <= (long long)LOSS_RPW * 0x7fffffffLL, "too many rows");
    const size_t blocks = loss_partials(rows);
    if (blocks == 0) return SRCNN_OK;
    SRCNN_LAUNCH(smooth_l1_backward_kernel, (unsigned)blocks, LOSS_THREADS, 0, as_stream(stream), a, norm, grad_loss, grad_pred);
    return check_launch("srcnn_smooth_l1_backward");
}

}  // extern "C"
