// Legacy point-lattice ROIAlign (gfx950).
//
// Reference: lib/model/roi_align/src/roi_align_kernel.cu:15-91 (one thread per output
// element, NCHW) + modules/roi_align.py:26-29 (RoIAlignAvg = (A+1)^2 lattice, then
// avg_pool2d(2, stride 1)) + stereo_rcnn/stereo_rcnn.py:110-139 (pyramid level routing).
//
// Two entry points:
//   * roi_align_forward_cuda : the reference's operator, same layout/semantics (NCHW in,
//     (n,C,ah,aw) out), kept as the drop-in symbol and as the op-level parity target.
//   * srcnn_pyramid_roi_align: the MI355X-native fused form used by the forward pass:
//     NHWC maps (the 4 bilinear taps of a lattice point are 4 coalesced channel runs),
//     level routing on the device (no nonzero()/host sync), both lattice rows of an output
//     row in registers, 2x2 average fused, result written straight into the (left|right)
//     channel slice of the head's GEMM operand.
// The float/double promotion pattern of the reference kernel (its `1.` literals) is reproduced operation by operation; every
// piece of that arithmetic is stated once, in roi_align_geom.h (lattice_blend() explains the pattern).
#include "conv_common.h"
#include "roi_align_geom.h"
#include <cstdlib>

namespace srcnn {

// lattice_blend() for 8 consecutive channels
__device__ __forceinline__ float8 lattice_blend(const float8 &ul, const float8 &ur, const float8 &dl, const float8 &dr, float h_ratio,
                                                float w_ratio)
{
    float8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v.v[e] = lattice_blend(ul.v[e], ur.v[e], dl.v[e], dr.v[e], h_ratio, w_ratio);
    return v;
}

__device__ __forceinline__ float8 avg2x2(const float8 &a, const float8 &b, const float8 &c, const float8 &d)
{
    float8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = avg2x2(a.v[e], b.v[e], c.v[e], d.v[e]);
    return o;
}

// value of one lattice point; `at(y, x)` fetches the feature value: a float, or the float8 of 8 consecutive channels
template <typename Fetch>
__device__ __forceinline__ auto lattice_point(float h, float w, int height, int width, Fetch at) -> decltype(at(0, 0))
{
    int hstart, wstart;
    float h_ratio, w_ratio;
    const bool h_ok = lattice_axis(h, height, hstart, h_ratio);
    const bool w_ok = lattice_axis(w, width, wstart, w_ratio);
    if (!h_ok || !w_ok) return {};                                           // :54-55
    return lattice_blend(at(hstart, wstart), at(hstart, wstart + 1), at(hstart + 1, wstart), at(hstart + 1, wstart + 1), h_ratio,
                         w_ratio);
}

__global__ void roi_align_nchw_kernel(int total, const float *__restrict__ feat, float scale, int height,
                                      int width, int channels, int ah, int aw, const float *__restrict__ rois,
                                      float *__restrict__ out)
{
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += blockDim.x * gridDim.x) {
        int pw = idx % aw;
        int ph = (idx / aw) % ah;
        int c = (idx / aw / ah) % channels;
        int n = idx / aw / ah / channels;
        const float *r = rois + (size_t)n * 5;
        RoiGeom g = roi_geom(r, scale, ah, aw);
        // reference: int img_start = roi_batch_ind * channels * height * width (float product, :51)
        int img_start = (int)(r[0] * (float)channels * (float)height * (float)width);
        float h = (float)ph * g.bin_h + g.start_h;
        float w = (float)pw * g.bin_w + g.start_w;
        const float *plane = feat + img_start + (size_t)c * height * width;
        out[idx] = lattice_point(h, w, height, width,
                                 [&](int y, int x) { return plane[y * width + x]; });
    }
}

struct PyramidArgs {
    const float *maps[4];
    RoiLevels lv;
};

// grid (A, n); block = C threads (C multiple of 64, <= 1024). One output row per block.
template <int A>
__global__ void pyramid_roi_align_kernel(PyramidArgs pa, int channels, const float *__restrict__ rois,
                                         float *__restrict__ out, int out_cstride, int out_coffset, int mfmt, int ofmt)
{
    const int n = blockIdx.y, py = blockIdx.x, c = threadIdx.x;
    if (pa.lv.roi_limit && n >= *pa.lv.roi_limit) return;
    const RoiView v = roi_view(pa.lv, pa.maps, rois, n, A);
    auto at = [&](int y, int x) { return act_load(v.base, mfmt, v.img + (size_t)y * v.width + x, channels, c); };
    float top[A + 1], bot[A + 1];
    const float h0 = (float)py * v.geo.bin_h + v.geo.start_h;
    const float h1 = (float)(py + 1) * v.geo.bin_h + v.geo.start_h;
#pragma unroll
    for (int px = 0; px <= A; ++px) {
        float w = (float)px * v.geo.bin_w + v.geo.start_w;
        top[px] = lattice_point(h0, w, v.height, v.width, at);
        bot[px] = lattice_point(h1, w, v.height, v.width, at);
    }
#pragma unroll
    for (int px = 0; px < A; ++px)
        act_store(out, ofmt, (size_t)(n * A + py) * A + px, out_cstride, out_coffset + c,
                  avg2x2(top[px], top[px + 1], bot[px], bot[px + 1]));
}

// The row-pair form (behind SRCNN_ROI_ALIGN_FORM=0): one thread per (roi, output row, 8-channel group), block (C/8, rows) of one
// or two wavefronts, grid (ceil(A/rows), n).
// A thread walks the A+1 lattice columns of its two lattice rows, keeps the previous column, and emits one 32-byte output
// group per step: every tap is a 32-byte load (both activation formats), every store 2 x 16 bytes, and the 32 groups of a
// row read 1 KB contiguous per tap.  (The per-channel kernel above issued 2-byte accesses: 8x the memory instructions.)
template <int A>
__global__ void pyramid_roi_align8_kernel(PyramidArgs pa, int channels, const float *__restrict__ rois,
                                          float *__restrict__ out, int out_cstride, int out_coffset, int mfmt, int ofmt)
{
    const int n = blockIdx.y, py = blockIdx.x * blockDim.y + threadIdx.y, g = threadIdx.x;
    if (py >= A || (pa.lv.roi_limit && n >= *pa.lv.roi_limit)) return;
    const RoiView v = roi_view(pa.lv, pa.maps, rois, n, A);
    auto at8 = [&](int y, int x) { return act_load8(v.base, mfmt, v.img + (size_t)y * v.width + x, channels, g); };
    const float h0 = (float)py * v.geo.bin_h + v.geo.start_h;
    const float h1 = (float)(py + 1) * v.geo.bin_h + v.geo.start_h;
    const float w0 = (float)0 * v.geo.bin_w + v.geo.start_w;                     // the reference's expression at px = 0
    float8 top_prev = lattice_point(h0, w0, v.height, v.width, at8);
    float8 bot_prev = lattice_point(h1, w0, v.height, v.width, at8);
#pragma unroll 2
    for (int px = 1; px <= A; ++px) {
        const float w = (float)px * v.geo.bin_w + v.geo.start_w;
        const float8 top = lattice_point(h0, w, v.height, v.width, at8);
        const float8 bot = lattice_point(h1, w, v.height, v.width, at8);
        act_store8(out, ofmt, (size_t)(n * A + py) * A + (px - 1), out_cstride, (out_coffset >> 3) + g,
                   avg2x2(top_prev, top, bot_prev, bot));
        top_prev = top;
        bot_prev = bot;
    }
}

// The form the forward uses: ONE workgroup per roi, thread (g, ry) = 8-channel group g of LATTICE row ry (A+1 rows).
// Every lattice point is computed once (the row-pair form above computes each lattice row twice, for the output rows above and
// below it: twice the tap loads and twice the double-precision blends); neighbouring rows meet through a double-buffered LDS
// slot per lattice column, behind a barrier that leaves global loads in flight, and the taps of column px + 1 are requested
// before column px is blended.  Same arithmetic per lattice point and the same sum order as above: bit-identical output.
struct LatticeTaps {
    float8 ul, ur, dl, dr;
    float w_ratio;
    bool ok;
};

template <int A>
__global__ __launch_bounds__(32 * (A + 1)) void pyramid_roi_align8_roi_kernel(PyramidArgs pa, int channels, const float *__restrict__ rois,
                                                                              float *__restrict__ out, int out_cstride, int out_coffset,
                                                                              int mfmt, int ofmt)
{
    __shared__ float4 lat[2][A + 1][32][2];                     // [column parity][lattice row][group][8 floats]
    const int n = blockIdx.x, ry = threadIdx.y, g = threadIdx.x;
    if (pa.lv.roi_limit && n >= *pa.lv.roi_limit) return;       // (uniform: the whole workgroup leaves)
    const RoiView v = roi_view(pa.lv, pa.maps, rois, n, A);
    const bool live = g * 8 < channels;                          // (channels < 256: the upper groups only keep the barriers company)
    // a point outside the map reads the map's first pixels and drops them: its taps start at 0, its blend is not used
    int hs;
    float h_ratio;
    const bool h_ok = lattice_axis((float)ry * v.geo.bin_h + v.geo.start_h, v.height, hs, h_ratio);
    const int hstart = h_ok ? hs : 0;
    auto request = [&](int px) {
        LatticeTaps t;
        int ws;
        const bool w_ok = lattice_axis((float)px * v.geo.bin_w + v.geo.start_w, v.width, ws, t.w_ratio);
        t.ok = h_ok && w_ok;                                     // roi_align_kernel.cu:54-55
        const int wstart = t.ok ? ws : 0;
        const size_t p0 = v.img + (size_t)hstart * v.width + wstart;
        const int gl = live ? g : 0;
        t.ul = act_load8(v.base, mfmt, p0, channels, gl);
        t.ur = act_load8(v.base, mfmt, p0 + 1, channels, gl);
        t.dl = act_load8(v.base, mfmt, p0 + v.width, channels, gl);
        t.dr = act_load8(v.base, mfmt, p0 + v.width + 1, channels, gl);
        return t;
    };
    auto blend = [&](const LatticeTaps &t) {                     // (h_ratio's part of lattice_blend is loop-invariant: hoisted)
        float8 b;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float p = lattice_blend(t.ul.v[e], t.ur.v[e], t.dl.v[e], t.dr.v[e], h_ratio, t.w_ratio);
            b.v[e] = t.ok ? p : 0.0f;
        }
        return b;
    };
    LatticeTaps cur = request(0);
    float8 top_prev = {}, bot_prev = {};
#pragma unroll 1
    for (int px = 0; px <= A; ++px) {
        LatticeTaps nxt = cur;
        if (px < A) nxt = request(px + 1);                       // in flight across the barrier below
        const float8 top = blend(cur);
        float4 *slot = &lat[px & 1][ry][g][0];
        slot[0] = make_float4(top.v[0], top.v[1], top.v[2], top.v[3]);
        slot[1] = make_float4(top.v[4], top.v[5], top.v[6], top.v[7]);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // LDS visibility only: the next column's taps stay in flight
        if (ry < A) {
            const float4 b0 = lat[px & 1][ry + 1][g][0], b1 = lat[px & 1][ry + 1][g][1];
            const float8 bot = {{b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w}};
            if (px >= 1 && live)
                act_store8(out, ofmt, (size_t)(n * A + ry) * A + (px - 1), out_cstride, (out_coffset >> 3) + g,
                           avg2x2(top_prev, top, bot_prev, bot));
            bot_prev = bot;
        }
        top_prev = top;
        cur = nxt;
    }
}

}  // namespace srcnn

// avg_pool2d / max_pool2d (kernel 2, stride 1) over the (planes, h, w) lattice of the legacy op: the reduction behind
// RoIAlignAvg / RoIAlignMax (modules/roi_align.py:26-29, 41-44): avg2x2() / first_max4().
__global__ void pool2x2_s1_kernel(const float *__restrict__ x, size_t planes, int h, int w, float *__restrict__ y, int take_max)
{
    const int oh = h - 1, ow = w - 1;
    const size_t total = planes * oh * ow;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int px = (int)(idx % ow);
        const int py = (int)((idx / ow) % oh);
        const size_t pl = idx / ((size_t)ow * oh);
        const float *q = x + (pl * h + py) * w + px;
        const float a = q[0], b = q[1], c = q[w], d = q[w + 1];
        y[idx] = take_max ? srcnn::first_max4(a, b, c, d).value : srcnn::avg2x2(a, b, c, d);
    }
}

extern "C" {

int srcnn_pool2x2_s1(const float *x, long long planes, int h, int w, float *y, int take_max, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(x && y && planes >= 0 && h >= 2 && w >= 2, "bad args (the lattice must be at least 2 x 2)");
    const size_t total = (size_t)planes * (h - 1) * (w - 1);
    if (total == 0) return SRCNN_OK;
    SRCNN_LAUNCH(pool2x2_s1_kernel, dim3(grid_for(total, 256, 65535)), dim3(256), 0, as_stream(stream), x, (size_t)planes, h, w, y,
                 take_max);
    return check_launch("srcnn_pool2x2_s1");
}

int roi_align_forward_cuda(int aligned_height, int aligned_width, float spatial_scale, const float *features,
                           int batch, int channels, int height, int width, const float *rois, int num_rois,
                           int roi_cols, float *output, srcnn_stream_t stream)
{
    using namespace srcnn;
    (void)batch;
    if (roi_cols != 5) return 0;   // roi_align_cuda.c:19-22
    const long long total = (long long)num_rois * aligned_height * aligned_width * channels;
    if (total == 0) return 1;
    if (total > 0x7fffffffLL) {
        set_error("roi_align_forward_cuda: output too large");
        return 0;
    }
    const int threads = 256;
    const int blocks = (int)((total + threads - 1) / threads);
    SRCNN_LAUNCH(roi_align_nchw_kernel, dim3(blocks), dim3(threads), 0, as_stream(stream), (int)total,
                       features, spatial_scale, height, width, channels, aligned_height, aligned_width, rois,
                       output);
    return check_launch("roi_align_forward_cuda") == SRCNN_OK ? 1 : 0;
}

int srcnn_pyramid_roi_align(const float *const *maps_host, const int *mh_host, const int *mw_host, int channels,
                            float im_height, const float *rois, int num_rois, int A, float *out, int out_cstride,
                            int out_coffset, int maps_format, int out_format, const int *roi_limit, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(channels % 64 == 0 && channels <= 1024, "channels must be a multiple of 64, <= 1024");
    SRCNN_REQUIRE(A == 7 || A == 14, "A must be 7 or 14");
    SRCNN_REQUIRE((unsigned)maps_format <= 1 && (unsigned)out_format <= 1, "bad format");
    if (out_format == 1) SRCNN_REQUIRE(out_cstride % 8 == 0 && out_coffset % 8 == 0, "SPLIT16 output alignment");
    if (num_rois == 0) return SRCNN_OK;
    PyramidArgs pa;
    for (int l = 0; l < 4; ++l) pa.maps[l] = maps_host[l];
    pa.lv = roi_levels(mh_host, mw_host, im_height, roi_limit);
    static const int roi_form = [] { const char *e = std::getenv("SRCNN_ROI_ALIGN_FORM"); return e ? std::atoi(e) : 1; }();   // A/B switch
    // the form: a kernel template (for A = 7 and 14) with its grid and block
    void (*k7)(PyramidArgs, int, const float *, float *, int, int, int, int);
    decltype(k7) k14;
    dim3 grid, block;
    if (out_cstride % 8 != 0 || out_coffset % 8 != 0) {
        // per channel: one output row per block
        k7 = pyramid_roi_align_kernel<7>, k14 = pyramid_roi_align_kernel<14>;
        grid = dim3(A, num_rois), block = dim3(channels);
    } else if (roi_form && channels <= 256) {
        // one workgroup per roi, one thread row per lattice row: every lattice point computed once
        k7 = pyramid_roi_align8_roi_kernel<7>, k14 = pyramid_roi_align8_roi_kernel<14>;
        grid = dim3(num_rois), block = dim3(32, A + 1);
    } else {
        // row pairs
        const int G = channels / 8, rows = G <= 32 ? 64 / G : 1;   // one or two wavefronts per block: thousands of small blocks
        k7 = pyramid_roi_align8_kernel<7>, k14 = pyramid_roi_align8_kernel<14>;
        grid = dim3((A + rows - 1) / rows, num_rois), block = dim3(G, rows);
    }
    SRCNN_LAUNCH(A == 7 ? k7 : k14, grid, block, 0, as_stream(stream), pa, channels, rois, out, out_cstride, out_coffset, maps_format,
                 out_format);
    return check_launch("srcnn_pyramid_roi_align");
}

}  // extern "C"
