// Training: the optimiser step (gfx950) -- global gradient norm with the clip coefficient, and SGD with momentum, over lists of tensors.
//
// Reference: clip_gradient (lib/model/utils/net_utils.py:37-49: one norm() per parameter, a Python sum, np.sqrt of a device value
// -- the host waits --, then p.grad.mul_(norm) over every gradient) followed by torch.optim.SGD.step() (trainval_net.py:158-168,
// 224-227: weight decay, momentum, update as separate passes).  Here: srcnn_grad_norm reads every gradient once and leaves
// {norm, clip_norm / max(norm, clip_norm)} on the device; srcnn_sgd_step reads p, g, m once and writes p, m, multiplying the
// gradient by that coefficient on the way, so the gradients are never rewritten and nothing is read back.
//
// The tensor list travels in the kernel's argument block (by value, at most SRCNN_OPT_TENSORS_PER_LAUNCH entries, tensors without
// elements left out on the host): no device-side table, no upload.
//
// THE WALK, the one way every kernel here goes over a list.  for_each_chunk: a tensor is cut into chunks of SRCNN_OPT_CHUNK
// elements, a workgroup takes one chunk at a time (grid stride) and finds the chunk's tensor by layer_list.h's search over the
// running chunk counts (uniform over the workgroup).  for_each_quad: thread t of 256 owns the chunk's local elements
// 4 (256 j + t) + k, j, k = 0..3, and visits them in ascending j: as one float4 where every pointer of the tensor is 16-byte
// aligned (chunk starts are multiples of 4096 elements, so a chunk is aligned as its tensor is) and the four lie inside the
// tensor, otherwise as the `count` (at most 4) single floats that do.  A kernel is the walk plus its element work, stated once
// for an element and applied to the float4's four or to the single floats.
//
// DEFINED SUMMATION ORDER of the norm (include/srcnn_hip.h states it for callers): no atomics, the same bits on every run, on
// every grid and for every alignment.
//   stage 1  float32: a thread adds the squares of its 16 elements in ascending (j, k) order starting from 0 (elements past the
//            tensor's end add nothing), a wavefront adds its 64 lanes with an xor butterfly (offsets 32 .. 1), thread 0 adds the
//            four wavefront sums ((w0 + w1) + w2) + w3 and writes workspace[chunk number in the whole list];
//   stage 2  one workgroup, float64: thread t adds workspace[t], workspace[t + 256], .. in that order starting from 0, the same
//            butterfly and four-term sum in double; thread 0 writes (float)sqrt(sum) and the coefficient.
//
// srcnn_grad_norm_guarded / srcnn_sgd_step_guarded (include/srcnn_hip.h, "skipped when not finite") are the same two passes over gradients that
// several backward passes summed: every gradient enters as g * grad_scale, the norm leaves a third word (1 where it is finite), and
// the update runs only under that word, so one Inf or NaN in a gradient costs one step and not the run.  They are the same code:
// grad_norm_partial_kernel<SCALED> and sgd_step_kernel<GUARDED> hold the one statement of the summation and of the update, and
// the plain instantiations compile without the multiplication, the word and the branch.
#include "layer_list.h"

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

// what srcnn_sgd_step_guarded adds to the step's arguments; the plain step carries none of it
template <bool GUARDED>
struct StepGuard {};

template <>
struct StepGuard<true> {
    float scale;
    const float *ok;
    unsigned *skipped;
};

// per_chunk(c, i, start, left) for every chunk c of the launch that this workgroup takes: tensor i of the list, the chunk's first
// element in it, and the elements from there to the tensor's end (>= 1)
template <typename Args, typename PerChunk>
__device__ __forceinline__ void for_each_chunk(const Args &a, PerChunk per_chunk)
{
    const int total = a.chunk_end[a.n - 1];
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        const int i = first_run_above(a.chunk_end, a.n, c);
        const long long start = (long long)(c - (i ? a.chunk_end[i - 1] : 0)) * OPT_CHUNK;
        per_chunk(c, i, start, a.t[i].numel - start);
    }
}

// body(e, quad, count) for the thread's four groups of a chunk in ascending j: e the group's first local element; quad: all four
// exist and are one aligned float4 (count is 4); otherwise the first `count` of them exist (count <= 0: none)
template <typename Body>
__device__ __forceinline__ void for_each_quad(bool vec, long long left, Body body)
{
#pragma unroll
    for (int j = 0; j < OPT_PER_THREAD; ++j) {
        const int e = (j * OPT_THREADS + (int)threadIdx.x) * 4;
        if (vec && e + 4 <= left) body(e, true, 4);
        else body(e, false, left - e < 4 ? (int)(left - e) : 4);
    }
}

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

// stage 1 of the norm.  SCALED: every gradient enters as g * scale (one rounding); otherwise `scale` is not read
template <bool SCALED>
__global__ __launch_bounds__(OPT_THREADS) void grad_norm_partial_kernel(GradArgs a, float scale, float *__restrict__ partial)
{
    __shared__ float red[OPT_THREADS / 64];
    const int tid = threadIdx.x;
    for_each_chunk(a, [&](int c, int i, long long start, long long left) {
        const float *g = a.t[i].g + start;
        float s = 0.0f;
        auto add_square = [&](float x) {
            if constexpr (SCALED) x = __fmul_rn(x, scale);
            s = __fadd_rn(s, __fmul_rn(x, x));
        };
        for_each_quad(a.vec[i] != 0, left, [&](int e, bool quad, int count) {
            if (quad) {
                const float4 v = *reinterpret_cast<const float4 *>(g + e);
                add_square(v.x), add_square(v.y), add_square(v.z), add_square(v.w);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < count) add_square(g[e + k]);
            }
        });
        s = wave_sum_f32(s);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) partial[a.chunk_base + c] = __fadd_rn(__fadd_rn(__fadd_rn(red[0], red[1]), red[2]), red[3]);
        __syncthreads();                                             // red is reused by the workgroup's next chunk
    });
}

// stage 2 of the norm.  words: 2, or 3 with out[2] = the norm is finite (srcnn_grad_norm_guarded)
__global__ __launch_bounds__(OPT_THREADS) void grad_norm_finish_kernel(const float *__restrict__ partial, long long count, float clip_norm,
                                                                        int words, float *__restrict__ out)
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
        // net_utils.py:46.  clip_norm = +inf says "do not clip" (inf / inf would be NaN); only the guarded entry lets it through
        out[1] = isinf(clip_norm) ? 1.0f : __fdiv_rn(clip_norm, norm > clip_norm ? norm : clip_norm);
        if (words > 2) out[2] = isfinite(norm) ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void grad_scale_kernel(GradArgs a, const float *__restrict__ coef)
{
    const float k = *coef;
    if (k == 1.0f) return;                                           // not clipped: every product would be its own operand
    for_each_chunk(a, [&](int, int i, long long start, long long left) {
        float *g = a.t[i].g + start;
        for_each_quad(a.vec[i] != 0, left, [&](int e, bool quad, int count) {
            if (quad) {
                float4 v = *reinterpret_cast<const float4 *>(g + e);
                v.x = __fmul_rn(v.x, k), v.y = __fmul_rn(v.y, k), v.z = __fmul_rn(v.z, k), v.w = __fmul_rn(v.w, k);
                *reinterpret_cast<float4 *>(g + e) = v;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < count) g[e + q] = __fmul_rn(g[e + q], k);
            }
        });
    });
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

// the update.  GUARDED: under the word *gd.ok, on g * gd.scale (one rounding, first)
template <bool GUARDED>
__global__ __launch_bounds__(OPT_THREADS) void sgd_step_kernel(StepArgs a, StepGuard<GUARDED> gd)
{
    const bool use_m = a.momentum != 0.0f, first = a.first_step != 0;
    if constexpr (GUARDED) {
        if (*gd.ok == 0.0f) {                                        // the same word for every thread of the grid: a uniform branch
            if (gd.skipped && blockIdx.x == 0 && threadIdx.x == 0) *gd.skipped = *gd.skipped + 1u;
            if (!(use_m && first)) return;
            // uninitialised momentum buffers: zeros, so that the next step's momentum * m + d is the d a first step stores
            for_each_chunk(a, [&](int, int i, long long start, long long left) {
                float *m = a.t[i].m + start;
                for_each_quad((a.t[i].flags & OPT_VEC) != 0, left, [&](int e, bool quad, int count) {
                    if (quad) {
                        *reinterpret_cast<float4 *>(m + e) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (q < count) m[e + q] = 0.0f;
                    }
                });
            });
            return;
        }
    }
    const float coef = a.coef ? *a.coef : 1.0f;
    for_each_chunk(a, [&](int, int i, long long start, long long left) {
        const int flags = a.t[i].flags;
        SgdScalars s;
        s.coef = coef, s.wd = a.t[i].wd, s.momentum = a.momentum, s.lr = a.t[i].lr;
        s.clip = a.coef != nullptr && (flags & OPT_CLIPPED), s.decay = s.wd != 0.0f, s.use_m = use_m, s.first = first;
        float *p = a.t[i].p + start;
        const float *g = a.t[i].g + start;
        float *m = use_m ? a.t[i].m + start : nullptr;
        auto element = [&](float &pe, float ge, float &me) {
            if constexpr (GUARDED) ge = __fmul_rn(ge, gd.scale);
            sgd_element(s, pe, ge, me);
        };
        for_each_quad((flags & OPT_VEC) != 0, left, [&](int e, bool quad, int count) {
            if (quad) {
                float4 pv = *reinterpret_cast<const float4 *>(p + e);
                const float4 gv = *reinterpret_cast<const float4 *>(g + e);
                float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (use_m && !first) mv = *reinterpret_cast<const float4 *>(m + e);
                element(pv.x, gv.x, mv.x), element(pv.y, gv.y, mv.y), element(pv.z, gv.z, mv.z), element(pv.w, gv.w, mv.w);
                if (use_m) *reinterpret_cast<float4 *>(m + e) = mv;
                *reinterpret_cast<float4 *>(p + e) = pv;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < count) {
                        float pe = p[e + q], me = (use_m && !first) ? m[e + q] : 0.0f;
                        element(pe, g[e + q], me);
                        if (use_m) m[e + q] = me;
                        p[e + q] = pe;
                    }
            }
        });
    });
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

// The validation helpers return the refusal's text or nullptr; the entry points pass it on under their own name (SRCNN_OPT_CHECK).
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

#define SRCNN_OPT_TRY(expr)                           \
    do {                                              \
        if (const char *_m = (expr)) return _m;       \
    } while (0)

// a list of gradients: the norm's entries and srcnn_grad_scale
static const char *check_grad_list(const float *const *g, const long long *numel, int n_tensors)
{
    SRCNN_OPT_TRY(check_list(n_tensors, numel));
    if (!g) return "null g_host";
    return check_pointers(reinterpret_cast<const void *const *>(g), numel, n_tensors, "null gradient pointer",
                          "gradient pointer not 4-byte aligned");
}

// the lists of the step's two entries
static const char *check_step_lists(float *const *p, const float *const *g, float *const *m, const long long *numel, const float *lr,
                                    const float *wd, int n_tensors, float momentum)
{
    SRCNN_OPT_TRY(check_list(n_tensors, numel));
    if (!(p && g && lr && wd)) return "null p_host / g_host / lr_host / weight_decay_host";
    if (!(momentum >= 0.0f && std::isfinite(momentum))) return "momentum must be >= 0 and finite";
    if (!(momentum == 0.0f || m)) return "momentum != 0 needs m_host (the momentum buffers)";
    SRCNN_OPT_TRY(check_pointers(reinterpret_cast<const void *const *>(p), numel, n_tensors, "null parameter pointer",
                                 "parameter pointer not 4-byte aligned"));
    SRCNN_OPT_TRY(check_pointers(reinterpret_cast<const void *const *>(g), numel, n_tensors, "null gradient pointer",
                                 "gradient pointer not 4-byte aligned"));
    if (momentum == 0.0f) return nullptr;
    return check_pointers(reinterpret_cast<const void *const *>(m), numel, n_tensors, "null momentum buffer pointer (momentum != 0)",
                          "momentum buffer pointer not 4-byte aligned");
}

#define SRCNN_OPT_CHECK_AS(who, expr)                 \
    do {                                              \
        const char *_m = (expr);                      \
        SRCNN_REQUIRE_AS(who, _m == nullptr, _m);     \
    } while (0)
#define SRCNN_OPT_CHECK(expr) SRCNN_OPT_CHECK_AS(__func__, expr)

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

// its sibling for the step: fills StepArgs launch by launch over the non-empty tensors and calls launch(args) for each
template <typename F>
static void for_each_step_launch(float *const *p, const float *const *g, float *const *m, const long long *numel, const float *lr,
                                 const float *wd, const int *clipped, int n_tensors, float momentum, int first_step, const float *coef,
                                 F launch)
{
    StepArgs a;
    a.n = 0, a.first_step = first_step, a.momentum = momentum, a.coef = coef;
    int chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] == 0) continue;
        StepTensor &t = a.t[a.n];
        t.p = p[i], t.g = g[i], t.m = momentum != 0.0f ? m[i] : nullptr;
        t.numel = numel[i], t.lr = lr[i], t.wd = wd[i], t.pad = 0;
        const bool vec = aligned_to(t.p, 16) && aligned_to(t.g, 16) && aligned_to(t.m, 16);
        t.flags = (vec ? OPT_VEC : 0) | ((!clipped || clipped[i]) ? OPT_CLIPPED : 0);
        chunks += (int)chunks_of(numel[i]);
        a.chunk_end[a.n] = chunks;
        if (++a.n == OPT_TPL) {
            launch(a);
            a.n = 0, chunks = 0;
        }
    }
    if (a.n > 0) launch(a);
}

// both norm entries under the name `who`: GUARDED takes clip_norm = +inf, scales by grad_scale and writes three words
template <bool GUARDED>
static int grad_norm(const char *who, const float *const *g_host, const long long *numel_host, int n_tensors, float clip_norm,
                     float grad_scale, float *out, void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    SRCNN_OPT_CHECK_AS(who, check_grad_list(g_host, numel_host, n_tensors));
    if (GUARDED) {
        SRCNN_REQUIRE_AS(who, clip_norm > 0.0f, "clip_norm must be > 0 (+infinity: do not clip)");
        SRCNN_REQUIRE_AS(who, grad_scale > 0.0f && std::isfinite(grad_scale), "grad_scale must be > 0 and finite");
    } else {
        SRCNN_REQUIRE_AS(who, clip_norm > 0.0f && std::isfinite(clip_norm), "clip_norm must be > 0 and finite");
    }
    SRCNN_REQUIRE_AS(who, out && workspace, "null out / workspace");
    SRCNN_REQUIRE_AS(who, aligned_to(out, 4) && aligned_to(workspace, 4), "out / workspace not 4-byte aligned");
    if (workspace_bytes < srcnn_grad_norm_workspace_bytes(n_tensors, numel_host)) {
        set_error("%s: workspace too small (srcnn_grad_norm_workspace_bytes)", who);
        return SRCNN_ERR_WORKSPACE;
    }
    float *partial = static_cast<float *>(workspace);
    hipStream_t st = as_stream(stream);
    for_each_grad_launch(const_cast<float *const *>(reinterpret_cast<const float *const *>(g_host)), numel_host, n_tensors, [&](const GradArgs &a) {
        SRCNN_LAUNCH(grad_norm_partial_kernel<GUARDED>, grid_of(a.chunk_end[a.n - 1]), OPT_THREADS, 0, st, a, grad_scale, partial);
    });
    SRCNN_LAUNCH(grad_norm_finish_kernel, 1, OPT_THREADS, 0, st, (const float *)partial, list_chunks(n_tensors, numel_host), clip_norm,
                 GUARDED ? 3 : 2, out);
    return check_launch(who);
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
    return srcnn::grad_norm<false>(__func__, g_host, numel_host, n_tensors, clip_norm, 1.0f, out, workspace, workspace_bytes, stream);
}

int srcnn_grad_norm_guarded(const float *const *g_host, const long long *numel_host, int n_tensors, float clip_norm, float grad_scale,
                            float *out, void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    return srcnn::grad_norm<true>(__func__, g_host, numel_host, n_tensors, clip_norm, grad_scale, out, workspace, workspace_bytes, stream);
}

int srcnn_grad_scale(float *const *g_host, const long long *numel_host, int n_tensors, const float *coef, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_OPT_CHECK(check_grad_list(g_host, numel_host, n_tensors));
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
    SRCNN_OPT_CHECK(check_step_lists(p_host, g_host, m_host, numel_host, lr_host, weight_decay_host, n_tensors, momentum));
    SRCNN_REQUIRE(aligned_to(coef, 4), "coef not 4-byte aligned");
    hipStream_t st = as_stream(stream);
    for_each_step_launch(p_host, g_host, m_host, numel_host, lr_host, weight_decay_host, clipped_host, n_tensors, momentum, first_step, coef,
                         [&](const StepArgs &a) {
                             SRCNN_LAUNCH(sgd_step_kernel<false>, grid_of(a.chunk_end[a.n - 1]), OPT_THREADS, 0, st, a, StepGuard<false>{});
                         });
    return check_launch("srcnn_sgd_step");
}

int srcnn_sgd_step_guarded(float *const *p_host, const float *const *g_host, float *const *m_host, const long long *numel_host,
                           const float *lr_host, const float *weight_decay_host, const int *clipped_host, int n_tensors, float momentum,
                           int first_step, float grad_scale, const float *coef, const float *ok, unsigned *skipped, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_OPT_CHECK(check_step_lists(p_host, g_host, m_host, numel_host, lr_host, weight_decay_host, n_tensors, momentum));
    SRCNN_REQUIRE(grad_scale > 0.0f && std::isfinite(grad_scale), "grad_scale must be > 0 and finite");
    SRCNN_REQUIRE(aligned_to(coef, 4), "coef not 4-byte aligned");
    SRCNN_REQUIRE(ok && aligned_to(ok, 4), "null or misaligned ok");
    SRCNN_REQUIRE(aligned_to(skipped, 4), "skipped not 4-byte aligned");
    hipStream_t st = as_stream(stream);
    StepGuard<true> gd = {grad_scale, ok, skipped};                  // the call's first launch counts a skipped step, no other one
    for_each_step_launch(p_host, g_host, m_host, numel_host, lr_host, weight_decay_host, clipped_host, n_tensors, momentum, first_step, coef,
                         [&](const StepArgs &a) {
                             SRCNN_LAUNCH(sgd_step_kernel<true>, grid_of(a.chunk_end[a.n - 1]), OPT_THREADS, 0, st, a, gd);
                             gd.skipped = nullptr;
                         });
    return check_launch("srcnn_sgd_step_guarded");
}

}  // extern "C"
