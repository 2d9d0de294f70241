// Training: the optimiser step (gfx950) -- global gradient norm with the clip coefficient, and SGD with momentum, over lists of tensors.
//
// Reference: clip_gradient (lib/model/utils/net_utils.py:37-49: one norm() per parameter, a Python sum, np.sqrt of a device value
// -- the host waits --, then p.grad.mul_(norm) over every gradient) followed by torch.optim.SGD.step() (trainval_net.py:158-168,
// 224-227: weight decay, momentum, update as separate passes).  Here: srcnn_grad_norm reads every gradient once and leaves
// {norm, clip_norm / max(norm, clip_norm)} on the device; srcnn_sgd_step reads p, g, m once and writes p, m, multiplying the
// gradient by that coefficient on the way, so the gradients are never rewritten and nothing is read back.
//
// The tensor list travels in the kernel's argument block (by value, at most SRCNN_OPT_TENSORS_PER_LAUNCH entries, tensors without
// elements left out on the host): no device-side table, no upload.  A tensor is cut into chunks of SRCNN_OPT_CHUNK elements, a
// workgroup takes one chunk at a time and finds the chunk's tensor by layer_list.h's search over the running chunk counts (uniform
// over the workgroup).  Thread t of 256 owns the local elements 4 (256 j + t) + k, j, k = 0..3: one float4 per j where every
// pointer of the tensor is 16-byte aligned (chunk starts are multiples of 4096 elements, so a chunk is aligned as its tensor is),
// single floats otherwise and where a float4 would cross the tensor's end.
//
// DEFINED SUMMATION ORDER of the norm (include/srcnn_hip.h states it for callers): no atomics, the same bits on every run, on
// every grid and for every alignment.
//   stage 1  float32: a thread adds the squares of its 16 elements in ascending (j, k) order starting from 0 (elements past the
//            tensor's end add nothing), a wavefront adds its 64 lanes with an xor butterfly (offsets 32 .. 1), thread 0 adds the
//            four wavefront sums ((w0 + w1) + w2) + w3 and writes workspace[chunk number in the whole list];
//   stage 2  one workgroup, float64: thread t adds workspace[t], workspace[t + 256], .. in that order starting from 0, the same
//            butterfly and four-term sum in double; thread 0 writes (float)sqrt(sum) and the coefficient.
//
// srcnn_grad_norm_guarded / srcnn_sgd_step_guarded (include/srcnn_optim_guard.h) are the same two passes over gradients that
// several backward passes summed: every gradient enters as g * grad_scale, the norm leaves a third word (1 where it is finite), and
// the update runs only under that word, so one Inf or NaN in a gradient costs one step and not the run.
#include "layer_list.h"

#include "../../include/srcnn_optim_guard.h"

#include <climits>
#include <cmath>

namespace srcnn {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = SRCNN_OPT_CHUNK;
constexpr int OPT_TPL = SRCNN_OPT_TENSORS_PER_LAUNCH;
constexpr int OPT_PER_THREAD = OPT_CHUNK / (OPT_THREADS * 4);      // float4 groups of a thread in one chunk
constexpr int OPT_MAX_GRID = 2048;                                  // 256 CUs x 8 workgroups: a streaming kernel loops over the rest
static_assert(OPT_PER_THREAD * OPT_THREADS * 4 == OPT_CHUNK && OPT_THREADS == 256, "optimiser chunking");

constexpr int OPT_VEC = 1, OPT_CLIPPED = 2;                         // StepTensor::flags

struct GradTensor {
    float *g;
    long long numel;
};

struct GradArgs {
    GradTensor t[OPT_TPL];
    int chunk_end[OPT_TPL];     // chunks of tensors 0..i of this launch
    int vec[OPT_TPL];           // g is 16-byte aligned
    int n;
    long long chunk_base;       // number of this launch's first chunk in the whole list
};

struct StepTensor {
    float *p;
    const float *g;
    float *m;
    long long numel;
    float lr, wd;
    int flags, pad;
};

struct StepArgs {
    StepTensor t[OPT_TPL];
    int chunk_end[OPT_TPL];
    int n, first_step;
    float momentum;
    const float *coef;
};

static_assert(sizeof(GradArgs) <= 4096 && sizeof(StepArgs) <= 4096, "the tensor list must fit HIP's kernel-argument block");

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float wave_sum_f32(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(OPT_THREADS) void grad_norm_partial_kernel(GradArgs a, float *__restrict__ partial)
{
    __shared__ float red[OPT_THREADS / 64];
    const int tid = threadIdx.x;
    const int total = a.chunk_end[a.n - 1];
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        const int i = first_run_above(a.chunk_end, a.n, c);
        const long long start = (long long)(c - (i ? a.chunk_end[i - 1] : 0)) * OPT_CHUNK;
        const float *g = a.t[i].g + start;
        const long long left = a.t[i].numel - start;                 // >= 1: the elements from the chunk's start to the tensor's end
        const bool vec = a.vec[i] != 0;
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < OPT_PER_THREAD; ++j) {
            const int e = (j * OPT_THREADS + tid) * 4;
            if (vec && e + 4 <= left) {
                const float4 v = *reinterpret_cast<const float4 *>(g + e);
                s = __fadd_rn(s, __fmul_rn(v.x, v.x));
                s = __fadd_rn(s, __fmul_rn(v.y, v.y));
                s = __fadd_rn(s, __fmul_rn(v.z, v.z));
                s = __fadd_rn(s, __fmul_rn(v.w, v.w));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e + k < left) {
                        const float x = g[e + k];
                        s = __fadd_rn(s, __fmul_rn(x, x));
                    }
            }
        }
        s = wave_sum_f32(s);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) partial[a.chunk_base + c] = __fadd_rn(__fadd_rn(__fadd_rn(red[0], red[1]), red[2]), red[3]);
        __syncthreads();                                             // red is reused by the workgroup's next chunk
    }
}

__global__ __launch_bounds__(OPT_THREADS) void grad_norm_finish_kernel(const float *__restrict__ partial, long long count, float clip_norm,
                                                                        float *__restrict__ out)
{
    __shared__ double red[OPT_THREADS / 64];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long i = tid; i < count; i += OPT_THREADS) s = s + (double)partial[i];
    s = wave_sum_f64(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const float norm = (float)sqrt(((red[0] + red[1]) + red[2]) + red[3]);
        out[0] = norm;
        out[1] = __fdiv_rn(clip_norm, norm > clip_norm ? norm : clip_norm);      // net_utils.py:46
    }
}

__global__ __launch_bounds__(OPT_THREADS) void grad_scale_kernel(GradArgs a, const float *__restrict__ coef)
{
    const float k = *coef;
    if (k == 1.0f) return;                                           // not clipped: every product would be its own operand
    const int tid = threadIdx.x;
    const int total = a.chunk_end[a.n - 1];
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        const int i = first_run_above(a.chunk_end, a.n, c);
        const long long start = (long long)(c - (i ? a.chunk_end[i - 1] : 0)) * OPT_CHUNK;
        float *g = a.t[i].g + start;
        const long long left = a.t[i].numel - start;
        const bool vec = a.vec[i] != 0;
#pragma unroll
        for (int j = 0; j < OPT_PER_THREAD; ++j) {
            const int e = (j * OPT_THREADS + tid) * 4;
            if (vec && e + 4 <= left) {
                float4 v = *reinterpret_cast<const float4 *>(g + e);
                v.x = __fmul_rn(v.x, k), v.y = __fmul_rn(v.y, k), v.z = __fmul_rn(v.z, k), v.w = __fmul_rn(v.w, k);
                *reinterpret_cast<float4 *>(g + e) = v;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (e + q < left) g[e + q] = __fmul_rn(g[e + q], k);
            }
        }
    }
}

struct SgdScalars {
    float coef, wd, momentum, lr;
    bool clip, decay, use_m, first;
};

// one element of the step: every operation rounded once (torch.optim.SGD, dampening 0, no Nesterov)
__device__ __forceinline__ void sgd_element(const SgdScalars &s, float &p, float g, float &m)
{
    float d = s.clip ? __fmul_rn(g, s.coef) : g;
    if (s.decay) d = __fadd_rn(d, __fmul_rn(s.wd, p));
    if (s.use_m) {
        m = s.first ? d : __fadd_rn(__fmul_rn(s.momentum, m), d);
        d = m;
    }
    p = __fsub_rn(p, __fmul_rn(s.lr, d));
}

__global__ __launch_bounds__(OPT_THREADS) void sgd_step_kernel(StepArgs a)
{
    const int tid = threadIdx.x;
    const int total = a.chunk_end[a.n - 1];
    const float coef = a.coef ? *a.coef : 1.0f;
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        const int i = first_run_above(a.chunk_end, a.n, c);
        const long long start = (long long)(c - (i ? a.chunk_end[i - 1] : 0)) * OPT_CHUNK;
        const long long left = a.t[i].numel - start;
        const int flags = a.t[i].flags;
        SgdScalars s;
        s.coef = coef, s.wd = a.t[i].wd, s.momentum = a.momentum, s.lr = a.t[i].lr;
        s.clip = a.coef != nullptr && (flags & OPT_CLIPPED), s.decay = s.wd != 0.0f, s.use_m = a.momentum != 0.0f, s.first = a.first_step != 0;
        float *p = a.t[i].p + start;
        const float *g = a.t[i].g + start;
        float *m = s.use_m ? a.t[i].m + start : nullptr;
        const bool vec = (flags & OPT_VEC) != 0;
#pragma unroll
        for (int j = 0; j < OPT_PER_THREAD; ++j) {
            const int e = (j * OPT_THREADS + tid) * 4;
            if (vec && e + 4 <= left) {
                float4 pv = *reinterpret_cast<const float4 *>(p + e);
                const float4 gv = *reinterpret_cast<const float4 *>(g + e);
                float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (s.use_m && !s.first) mv = *reinterpret_cast<const float4 *>(m + e);
                sgd_element(s, pv.x, gv.x, mv.x);
                sgd_element(s, pv.y, gv.y, mv.y);
                sgd_element(s, pv.z, gv.z, mv.z);
                sgd_element(s, pv.w, gv.w, mv.w);
                if (s.use_m) *reinterpret_cast<float4 *>(m + e) = mv;
                *reinterpret_cast<float4 *>(p + e) = pv;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (e + q < left) {
                        float pe = p[e + q], me = (s.use_m && !s.first) ? m[e + q] : 0.0f;
                        sgd_element(s, pe, g[e + q], me);
                        if (s.use_m) m[e + q] = me;
                        p[e + q] = pe;
                    }
            }
        }
    }
}

// ---- the guarded pair (include/srcnn_optim_guard.h): the kernels above with g * scale in the place of g, the norm's finiteness
// as a third word, and the update under that word.  They stand beside the kernels above, which keep their code.

__global__ __launch_bounds__(OPT_THREADS) void grad_norm_guarded_partial_kernel(GradArgs a, float scale, float *__restrict__ partial)
{
    __shared__ float red[OPT_THREADS / 64];
    const int tid = threadIdx.x;
    const int total = a.chunk_end[a.n - 1];
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        const int i = first_run_above(a.chunk_end, a.n, c);
        const long long start = (long long)(c - (i ? a.chunk_end[i - 1] : 0)) * OPT_CHUNK;
        const float *g = a.t[i].g + start;
        const long long left = a.t[i].numel - start;
        const bool vec = a.vec[i] != 0;
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < OPT_PER_THREAD; ++j) {
            const int e = (j * OPT_THREADS + tid) * 4;
            if (vec && e + 4 <= left) {
                float4 v = *reinterpret_cast<const float4 *>(g + e);
                v.x = __fmul_rn(v.x, scale), v.y = __fmul_rn(v.y, scale), v.z = __fmul_rn(v.z, scale), v.w = __fmul_rn(v.w, scale);
                s = __fadd_rn(s, __fmul_rn(v.x, v.x));
                s = __fadd_rn(s, __fmul_rn(v.y, v.y));
                s = __fadd_rn(s, __fmul_rn(v.z, v.z));
                s = __fadd_rn(s, __fmul_rn(v.w, v.w));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e + k < left) {
                        const float x = __fmul_rn(g[e + k], scale);
                        s = __fadd_rn(s, __fmul_rn(x, x));
                    }
            }
        }
        s = wave_sum_f32(s);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) partial[a.chunk_base + c] = __fadd_rn(__fadd_rn(__fadd_rn(red[0], red[1]), red[2]), red[3]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(OPT_THREADS) void grad_norm_guarded_finish_kernel(const float *__restrict__ partial, long long count,
                                                                                float clip_norm, float *__restrict__ out)
{
    __shared__ double red[OPT_THREADS / 64];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long i = tid; i < count; i += OPT_THREADS) s = s + (double)partial[i];
    s = wave_sum_f64(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const float norm = (float)sqrt(((red[0] + red[1]) + red[2]) + red[3]);
        out[0] = norm;
        // clip_norm = +inf says "do not clip": inf / inf would be NaN
        out[1] = isinf(clip_norm) ? 1.0f : __fdiv_rn(clip_norm, norm > clip_norm ? norm : clip_norm);
        out[2] = isfinite(norm) ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void sgd_step_guarded_kernel(StepArgs a, float scale, const float *__restrict__ ok,
                                                                        unsigned *skipped)
{
    const int tid = threadIdx.x;
    const int total = a.chunk_end[a.n - 1];
    const bool use_m = a.momentum != 0.0f, first = a.first_step != 0;
    if (*ok == 0.0f) {                                               // the same word for every thread of the grid: a uniform branch
        if (skipped && blockIdx.x == 0 && tid == 0) *skipped = *skipped + 1u;
        if (!(use_m && first)) return;
        // uninitialised momentum buffers: zeros, so that the next step's momentum * m + d is the d a first step stores
        for (int c = blockIdx.x; c < total; c += gridDim.x) {
            const int i = first_run_above(a.chunk_end, a.n, c);
            const long long start = (long long)(c - (i ? a.chunk_end[i - 1] : 0)) * OPT_CHUNK;
            const long long left = a.t[i].numel - start;
            float *m = a.t[i].m + start;
            const bool vec = (a.t[i].flags & OPT_VEC) != 0;
#pragma unroll
            for (int j = 0; j < OPT_PER_THREAD; ++j) {
                const int e = (j * OPT_THREADS + tid) * 4;
                if (vec && e + 4 <= left) {
                    *reinterpret_cast<float4 *>(m + e) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (e + q < left) m[e + q] = 0.0f;
                }
            }
        }
        return;
    }
    const float coef = a.coef ? *a.coef : 1.0f;
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        const int i = first_run_above(a.chunk_end, a.n, c);
        const long long start = (long long)(c - (i ? a.chunk_end[i - 1] : 0)) * OPT_CHUNK;
        const long long left = a.t[i].numel - start;
        const int flags = a.t[i].flags;
        SgdScalars s;
        s.coef = coef, s.wd = a.t[i].wd, s.momentum = a.momentum, s.lr = a.t[i].lr;
        s.clip = a.coef != nullptr && (flags & OPT_CLIPPED), s.decay = s.wd != 0.0f, s.use_m = use_m, s.first = first;
        float *p = a.t[i].p + start;
        const float *g = a.t[i].g + start;
        float *m = s.use_m ? a.t[i].m + start : nullptr;
        const bool vec = (flags & OPT_VEC) != 0;
#pragma unroll
        for (int j = 0; j < OPT_PER_THREAD; ++j) {
            const int e = (j * OPT_THREADS + tid) * 4;
            if (vec && e + 4 <= left) {
                float4 pv = *reinterpret_cast<const float4 *>(p + e);
                const float4 gv = *reinterpret_cast<const float4 *>(g + e);
                float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (s.use_m && !s.first) mv = *reinterpret_cast<const float4 *>(m + e);
                sgd_element(s, pv.x, __fmul_rn(gv.x, scale), mv.x);
                sgd_element(s, pv.y, __fmul_rn(gv.y, scale), mv.y);
                sgd_element(s, pv.z, __fmul_rn(gv.z, scale), mv.z);
                sgd_element(s, pv.w, __fmul_rn(gv.w, scale), mv.w);
                if (s.use_m) *reinterpret_cast<float4 *>(m + e) = mv;
                *reinterpret_cast<float4 *>(p + e) = pv;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (e + q < left) {
                        float pe = p[e + q], me = (s.use_m && !s.first) ? m[e + q] : 0.0f;
                        sgd_element(s, pe, __fmul_rn(g[e + q], scale), me);
                        if (s.use_m) m[e + q] = me;
                        p[e + q] = pe;
                    }
            }
        }
    }
}

static long long chunks_of(long long numel) { return (numel + OPT_CHUNK - 1) / OPT_CHUNK; }

// the list's chunk count, or -1: a null list, n_tensors <= 0, a negative numel, more than INT_MAX chunks
static long long list_chunks(int n_tensors, const long long *numel)
{
    if (!numel || n_tensors <= 0) return -1;
    long long total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0) return -1;
        total += chunks_of(numel[i]);
        if (total > INT_MAX) return -1;
    }
    return total;
}

static unsigned grid_of(int chunks) { return (unsigned)(chunks < OPT_MAX_GRID ? chunks : OPT_MAX_GRID); }

// validation shared by the three entry points; `who` arrives through SRCNN_REQUIRE's __func__ in the callers
static const char *check_list(int n_tensors, const long long *numel)
{
    if (n_tensors <= 0) return "n_tensors must be >= 1";
    if (!numel) return "null numel_host";
    for (int i = 0; i < n_tensors; ++i)
        if (numel[i] < 0) return "negative numel";
    if (list_chunks(n_tensors, numel) < 0) return "too many chunks (more than 2^31 - 1)";
    return nullptr;
}

static const char *check_pointers(const void *const *ptrs, const long long *numel, int n_tensors, const char *null_msg, const char *align_msg)
{
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] == 0) continue;
        if (!ptrs[i]) return null_msg;
        if (!aligned_to(ptrs[i], 4)) return align_msg;
    }
    return nullptr;
}

#define SRCNN_OPT_CHECK(expr)                         \
    do {                                              \
        const char *_m = (expr);                      \
        SRCNN_REQUIRE(_m == nullptr, _m);             \
    } while (0)

// fills GradArgs launch by launch over the non-empty tensors of the list and calls launch(args) for each
template <typename F>
static void for_each_grad_launch(float *const *g, const long long *numel, int n_tensors, F launch)
{
    GradArgs a;
    a.n = 0, a.chunk_base = 0;
    int chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] == 0) continue;
        chunks += (int)chunks_of(numel[i]);
        a.t[a.n].g = g[i], a.t[a.n].numel = numel[i];
        a.vec[a.n] = aligned_to(g[i], 16) ? 1 : 0;
        a.chunk_end[a.n] = chunks;
        if (++a.n == OPT_TPL) {
            launch(a);
            a.chunk_base += chunks;
            a.n = 0, chunks = 0;
        }
    }
    if (a.n > 0) launch(a);
}

}  // namespace srcnn

extern "C" {

size_t srcnn_grad_norm_workspace_bytes(int n_tensors, const long long *numel_host)
{
    using namespace srcnn;
    const long long chunks = list_chunks(n_tensors, numel_host);
    if (chunks < 0) return 0;
    return align_up((size_t)(chunks > 0 ? chunks : 1) * sizeof(float), 256);
}

int srcnn_grad_norm(const float *const *g_host, const long long *numel_host, int n_tensors, float clip_norm, float *out, void *workspace,
                    size_t workspace_bytes, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_OPT_CHECK(check_list(n_tensors, numel_host));
    SRCNN_REQUIRE(g_host, "null g_host");
    SRCNN_OPT_CHECK(check_pointers(reinterpret_cast<const void *const *>(g_host), numel_host, n_tensors, "null gradient pointer",
                                   "gradient pointer not 4-byte aligned"));
    SRCNN_REQUIRE(clip_norm > 0.0f && std::isfinite(clip_norm), "clip_norm must be > 0 and finite");
    SRCNN_REQUIRE(out && workspace, "null out / workspace");
    SRCNN_REQUIRE(aligned_to(out, 4) && aligned_to(workspace, 4), "out / workspace not 4-byte aligned");
    if (workspace_bytes < srcnn_grad_norm_workspace_bytes(n_tensors, numel_host)) {
        set_error("srcnn_grad_norm: workspace too small (srcnn_grad_norm_workspace_bytes)");
        return SRCNN_ERR_WORKSPACE;
    }
    float *partial = static_cast<float *>(workspace);
    hipStream_t st = as_stream(stream);
    for_each_grad_launch(const_cast<float *const *>(reinterpret_cast<const float *const *>(g_host)), numel_host, n_tensors, [&](const GradArgs &a) {
        SRCNN_LAUNCH(grad_norm_partial_kernel, grid_of(a.chunk_end[a.n - 1]), OPT_THREADS, 0, st, a, partial);
    });
    SRCNN_LAUNCH(grad_norm_finish_kernel, 1, OPT_THREADS, 0, st, (const float *)partial, list_chunks(n_tensors, numel_host), clip_norm, out);
    return check_launch("srcnn_grad_norm");
}

int srcnn_grad_scale(float *const *g_host, const long long *numel_host, int n_tensors, const float *coef, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_OPT_CHECK(check_list(n_tensors, numel_host));
    SRCNN_REQUIRE(g_host, "null g_host");
    SRCNN_OPT_CHECK(check_pointers(reinterpret_cast<const void *const *>(g_host), numel_host, n_tensors, "null gradient pointer",
                                   "gradient pointer not 4-byte aligned"));
    SRCNN_REQUIRE(coef && aligned_to(coef, 4), "null or misaligned coef");
    hipStream_t st = as_stream(stream);
    for_each_grad_launch(g_host, numel_host, n_tensors, [&](const GradArgs &a) {
        SRCNN_LAUNCH(grad_scale_kernel, grid_of(a.chunk_end[a.n - 1]), OPT_THREADS, 0, st, a, coef);
    });
    return check_launch("srcnn_grad_scale");
}

int srcnn_sgd_step(float *const *p_host, const float *const *g_host, float *const *m_host, const long long *numel_host, const float *lr_host,
                   const float *weight_decay_host, const int *clipped_host, int n_tensors, float momentum, int first_step, const float *coef,
                   srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_OPT_CHECK(check_list(n_tensors, numel_host));
    SRCNN_REQUIRE(p_host && g_host && lr_host && weight_decay_host, "null p_host / g_host / lr_host / weight_decay_host");
    SRCNN_REQUIRE(momentum >= 0.0f && std::isfinite(momentum), "momentum must be >= 0 and finite");
    SRCNN_REQUIRE(momentum == 0.0f || m_host, "momentum != 0 needs m_host (the momentum buffers)");
    SRCNN_OPT_CHECK(check_pointers(reinterpret_cast<const void *const *>(p_host), numel_host, n_tensors, "null parameter pointer",
                                   "parameter pointer not 4-byte aligned"));
    SRCNN_OPT_CHECK(check_pointers(reinterpret_cast<const void *const *>(g_host), numel_host, n_tensors, "null gradient pointer",
                                   "gradient pointer not 4-byte aligned"));
    if (momentum != 0.0f)
        SRCNN_OPT_CHECK(check_pointers(reinterpret_cast<const void *const *>(m_host), numel_host, n_tensors,
                                       "null momentum buffer pointer (momentum != 0)", "momentum buffer pointer not 4-byte aligned"));
    SRCNN_REQUIRE(aligned_to(coef, 4), "coef not 4-byte aligned");
    hipStream_t st = as_stream(stream);
    StepArgs a;
    a.n = 0, a.first_step = first_step, a.momentum = momentum, a.coef = coef;
    int chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel_host[i] == 0) continue;
        StepTensor &t = a.t[a.n];
        t.p = p_host[i], t.g = g_host[i], t.m = momentum != 0.0f ? m_host[i] : nullptr;
        t.numel = numel_host[i], t.lr = lr_host[i], t.wd = weight_decay_host[i], t.pad = 0;
        const bool vec = aligned_to(t.p, 16) && aligned_to(t.g, 16) && aligned_to(t.m, 16);
        t.flags = (vec ? OPT_VEC : 0) | ((!clipped_host || clipped_host[i]) ? OPT_CLIPPED : 0);
        chunks += (int)chunks_of(numel_host[i]);
        a.chunk_end[a.n] = chunks;
        if (++a.n == OPT_TPL) {
            SRCNN_LAUNCH(sgd_step_kernel, grid_of(chunks), OPT_THREADS, 0, st, a);
            a.n = 0, chunks = 0;
        }
    }
    if (a.n > 0) SRCNN_LAUNCH(sgd_step_kernel, grid_of(chunks), OPT_THREADS, 0, st, a);
    return check_launch("srcnn_sgd_step");
}

int srcnn_grad_norm_guarded(const float *const *g_host, const long long *numel_host, int n_tensors, float clip_norm, float grad_scale,
                            float *out, void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_OPT_CHECK(check_list(n_tensors, numel_host));
    SRCNN_REQUIRE(g_host, "null g_host");
    SRCNN_OPT_CHECK(check_pointers(reinterpret_cast<const void *const *>(g_host), numel_host, n_tensors, "null gradient pointer",
                                   "gradient pointer not 4-byte aligned"));
    SRCNN_REQUIRE(clip_norm > 0.0f, "clip_norm must be > 0 (+infinity: do not clip)");
    SRCNN_REQUIRE(grad_scale > 0.0f && std::isfinite(grad_scale), "grad_scale must be > 0 and finite");
    SRCNN_REQUIRE(out && workspace, "null out / workspace");
    SRCNN_REQUIRE(aligned_to(out, 4) && aligned_to(workspace, 4), "out / workspace not 4-byte aligned");
    if (workspace_bytes < srcnn_grad_norm_workspace_bytes(n_tensors, numel_host)) {
        set_error("srcnn_grad_norm_guarded: workspace too small (srcnn_grad_norm_workspace_bytes)");
        return SRCNN_ERR_WORKSPACE;
    }
    float *partial = static_cast<float *>(workspace);
    hipStream_t st = as_stream(stream);
    for_each_grad_launch(const_cast<float *const *>(reinterpret_cast<const float *const *>(g_host)), numel_host, n_tensors, [&](const GradArgs &a) {
        SRCNN_LAUNCH(grad_norm_guarded_partial_kernel, grid_of(a.chunk_end[a.n - 1]), OPT_THREADS, 0, st, a, grad_scale, partial);
    });
    SRCNN_LAUNCH(grad_norm_guarded_finish_kernel, 1, OPT_THREADS, 0, st, (const float *)partial, list_chunks(n_tensors, numel_host), clip_norm,
                 out);
    return check_launch("srcnn_grad_norm_guarded");
}

int srcnn_sgd_step_guarded(float *const *p_host, const float *const *g_host, float *const *m_host, const long long *numel_host,
                           const float *lr_host, const float *weight_decay_host, const int *clipped_host, int n_tensors, float momentum,
                           int first_step, float grad_scale, const float *coef, const float *ok, unsigned *skipped, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_OPT_CHECK(check_list(n_tensors, numel_host));
    SRCNN_REQUIRE(p_host && g_host && lr_host && weight_decay_host, "null p_host / g_host / lr_host / weight_decay_host");
    SRCNN_REQUIRE(momentum >= 0.0f && std::isfinite(momentum), "momentum must be >= 0 and finite");
    SRCNN_REQUIRE(momentum == 0.0f || m_host, "momentum != 0 needs m_host (the momentum buffers)");
    SRCNN_OPT_CHECK(check_pointers(reinterpret_cast<const void *const *>(p_host), numel_host, n_tensors, "null parameter pointer",
                                   "parameter pointer not 4-byte aligned"));
    SRCNN_OPT_CHECK(check_pointers(reinterpret_cast<const void *const *>(g_host), numel_host, n_tensors, "null gradient pointer",
                                   "gradient pointer not 4-byte aligned"));
    if (momentum != 0.0f)
        SRCNN_OPT_CHECK(check_pointers(reinterpret_cast<const void *const *>(m_host), numel_host, n_tensors,
                                       "null momentum buffer pointer (momentum != 0)", "momentum buffer pointer not 4-byte aligned"));
    SRCNN_REQUIRE(grad_scale > 0.0f && std::isfinite(grad_scale), "grad_scale must be > 0 and finite");
    SRCNN_REQUIRE(aligned_to(coef, 4), "coef not 4-byte aligned");
    SRCNN_REQUIRE(ok && aligned_to(ok, 4), "null or misaligned ok");
    SRCNN_REQUIRE(aligned_to(skipped, 4), "skipped not 4-byte aligned");
    hipStream_t st = as_stream(stream);
    StepArgs a;
    a.n = 0, a.first_step = first_step, a.momentum = momentum, a.coef = coef;
    int chunks = 0;
    unsigned *count = skipped;                                       // the call's first launch counts a skipped step, no other one
    for (int i = 0; i < n_tensors; ++i) {
        if (numel_host[i] == 0) continue;
        StepTensor &t = a.t[a.n];
        t.p = p_host[i], t.g = g_host[i], t.m = momentum != 0.0f ? m_host[i] : nullptr;
        t.numel = numel_host[i], t.lr = lr_host[i], t.wd = weight_decay_host[i], t.pad = 0;
        const bool vec = aligned_to(t.p, 16) && aligned_to(t.g, 16) && aligned_to(t.m, 16);
        t.flags = (vec ? OPT_VEC : 0) | ((!clipped_host || clipped_host[i]) ? OPT_CLIPPED : 0);
        chunks += (int)chunks_of(numel_host[i]);
        a.chunk_end[a.n] = chunks;
        if (++a.n == OPT_TPL) {
            SRCNN_LAUNCH(sgd_step_guarded_kernel, grid_of(chunks), OPT_THREADS, 0, st, a, grad_scale, ok, count);
            count = nullptr;
            a.n = 0, chunks = 0;
        }
    }
    if (a.n > 0) SRCNN_LAUNCH(sgd_step_guarded_kernel, grid_of(chunks), OPT_THREADS, 0, st, a, grad_scale, ok, count);
    return check_launch("srcnn_sgd_step_guarded");
}

}  // extern "C"
