// ROIAlign backward (gfx950): the adjoint of roi_align.hip with respect to the feature maps.
//
// Reference: lib/model/roi_align/src/roi_align_kernel.cu:94-143 -- one thread per lattice point, four float atomicAdd()s into a
// zeroed map, so its result depends on the order in which the atomics arrive.  Here the sum is a GATHER with a defined
// order: a workgroup owns a tile of map pixels, lists the rois that reach the tile in roi order (ballot compaction into
// LDS), and every (pixel, channel) adds its contributions in ascending (roi, ph, pw) order, starting from 0, and is written
// exactly once: no atomics, no zero fill, run-to-run bit-equal.  The value of one contribution is the reference's
// expression with its float/double promotions (:137-140); geometry, the level table and the adjoint of the 2x2 window come
// from roi_align_geom.h, shared with the forward.
//
// Entry points:
//   * roi_align_backward_cuda          : the reference's operator (NCHW, one map), the drop-in symbol;
//   * srcnn_pool2x2_s1_backward        : adjoint of srcnn_pool2x2_s1 (RoIAlignAvg / RoIAlignMax);
//   * srcnn_pyramid_roi_align_backward : adjoint of srcnn_pyramid_roi_align: NHWC, four levels in one launch, the 2x2
//     average folded in (the lattice gradient is formed in registers).
#include "common.h"
#include "roi_align_geom.h"

namespace srcnn {

constexpr int BWD_TH = 4;             // tile rows = wavefronts of a workgroup (one map row each)
constexpr int BWD_TW = 8;             // tile columns, walked by the row's wavefront
constexpr int BWD_CHUNK = 1024;       // rois tested per chunk (4 per thread); a chunk's hits always fit the LDS list

struct RoiBwdArgs {
    float *maps[4];
    RoiLevels lv;                     // (roi_limit: the rois from it on contribute nothing)
    int row0[5];                      // blockIdx.y range of each level's tile rows
    int route;                        // 1: pyramid level routing; 0: every roi belongs to level 0
};

struct RoiHit {
    float start_w, start_h, bin_w, bin_h;
    int n;
    unsigned ranges;                  // ph_lo | ph_hi << 8 | pw_lo << 16 | pw_hi << 24
};

template <int VEC>
struct Vec;
template <>
struct Vec<1> {
    float v[1];
    __device__ __forceinline__ void load(const float *p) { v[0] = *p; }
    __device__ __forceinline__ void store(float *p) const { *p = v[0]; }
};
template <>
struct Vec<4> {
    float v[4];
    __device__ __forceinline__ void load(const float *p)
    {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    }
    __device__ __forceinline__ void store(float *p) const { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// Block (64, BWD_TH); grid (tile columns of the widest level, tile rows of all levels, batch x channel blocks).
// lanes = channels (VEC consecutive ones each).  Element (c, pixel p) of a map lies at c * map_cs + p * map_ps behind the
// image's start; the gradient of lattice / output point q of roi n, channel c, at n * g_ns + q * g_ps + c * g_cs.
// FUSED: g is the gradient of the A x A average-pooled output (A = ah - 1 = aw - 1) and the lattice gradient of a point is
// window2x2_adjoint() of it; otherwise g is the lattice gradient itself.
template <int VEC, bool FUSED>
__global__ __launch_bounds__(64 * BWD_TH) void roi_align_backward_kernel(RoiBwdArgs ba, const float *__restrict__ rois, int num_rois,
                                                                         int ah, int aw, const float *__restrict__ g, long long g_ns,
                                                                         int g_ps, int g_cs, int channels, int ncb, long long map_cs,
                                                                         int map_ps)
{
    __shared__ RoiHit hits[BWD_CHUNK];
    __shared__ int wave_hits[BWD_TH];
    const int lane = threadIdx.x, wave = threadIdx.y;
    // (level, tile row) from blockIdx.y, (image, channel block) from blockIdx.z: scalar compares, no division
    int l = 0;
    while (l < 3 && (int)blockIdx.y >= ba.row0[l + 1]) ++l;
    const int height = ba.lv.mh[l], width = ba.lv.mw[l];
    const int x0 = blockIdx.x * BWD_TW, y0 = ((int)blockIdx.y - ba.row0[l]) * BWD_TH;
    if (x0 >= width) return;                                        // (uniform: the grid is as wide as the widest level)
    int b = 0, cb = blockIdx.z;
    while (cb >= ncb) cb -= ncb, ++b;
    const int c = (cb * 64 + lane) * VEC;
    const bool live = c < channels;
    const int y = y0 + wave;
    const bool row_live = y < height;
    const float scale = ba.lv.scale[l];
    const int limit = ba.lv.roi_limit ? min(*ba.lv.roi_limit, num_rois) : num_rois;
    float *out = ba.maps[l] + ((size_t)b * channels * height * width) + (size_t)c * map_cs;
    const int tid = wave * 64 + lane;

    for (int base = 0; base == 0 || base < limit; base += BWD_CHUNK) {
        // ---- phase 1: the rois of this chunk that reach the tile, compacted in roi order
        int count = 0;
        for (int sub = 0; sub < BWD_CHUNK / 256; ++sub) {
            const int n = base + sub * 256 + tid;
            bool hit = false;
            RoiHit e;
            if (n < limit) {
                const float *r = rois + (size_t)n * 5;
                // image and level first: most rois of a batch fail here, before any geometry (roi_geom's batch is (int)r[0])
                if ((int)r[0] == b && (!ba.route || pyramid_level(r) == l)) {
                    const RoiGeom geo = roi_geom(r, scale, ah, aw);
                    // lattice rows whose taps fall on tile rows [y0, y0 + TH): a contiguous range, bin_size >= 0
                    int ph_lo = ah, ph_hi = -1, pw_lo = aw, pw_hi = -1;
                    for (int ph = 0; ph < ah; ++ph) {
                        int s;
                        float ratio;
                        const float h = (float)ph * geo.bin_h + geo.start_h;
                        if (lattice_axis(h, height, s, ratio) && s + 1 >= y0 && s < y0 + BWD_TH) ph_lo = min(ph_lo, ph), ph_hi = ph;
                    }
                    for (int pw = 0; pw < aw; ++pw) {
                        int s;
                        float ratio;
                        const float w = (float)pw * geo.bin_w + geo.start_w;
                        if (lattice_axis(w, width, s, ratio) && s + 1 >= x0 && s < x0 + BWD_TW) pw_lo = min(pw_lo, pw), pw_hi = pw;
                    }
                    hit = ph_hi >= 0 && pw_hi >= 0;
                    e.start_w = geo.start_w, e.start_h = geo.start_h, e.bin_w = geo.bin_w, e.bin_h = geo.bin_h;
                    e.n = n;
                    e.ranges = (unsigned)ph_lo | (unsigned)ph_hi << 8 | (unsigned)pw_lo << 16 | (unsigned)pw_hi << 24;
                }
            }
            const unsigned long long mask = __ballot(hit);
            if (lane == 0) wave_hits[wave] = __popcll(mask);
            __syncthreads();
            int before = count;
            for (int wv = 0; wv < BWD_TH; ++wv) {
                const int k = wave_hits[wv];
                before += wv < wave ? k : 0;
                count += k;
            }
            if (hit) hits[before + __popcll(mask & ((1ull << lane) - 1ull))] = e;
            __syncthreads();                                          // (also: wave_hits may be rewritten)
        }
        // ---- phase 2: this wavefront's map row.  The BWD_TW running sums of a lane live in registers; a lattice point is
        // located once per row (not once per pixel), its gradient loaded once, and its two taps of this row added to the two
        // pixels they fall on.  For one pixel the additions still arrive in (roi, ph, pw) order.  The running sum of a later
        // chunk continues from the element this same thread wrote after the chunk before it.
        if (row_live && live) {
            float *row = out + (size_t)y * width * map_ps;
            Vec<VEC> acc[BWD_TW];
#pragma unroll
            for (int j = 0; j < BWD_TW; ++j) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[j].v[i] = 0.0f;
                if (base != 0 && x0 + j < width) acc[j].load(row + (size_t)(x0 + j) * map_ps);
            }
            for (int k = 0; k < count; ++k) {
                const RoiHit e = hits[k];
                const int ph_hi = (e.ranges >> 8) & 255, pw_lo = (e.ranges >> 16) & 255, pw_hi = e.ranges >> 24;
                const float *gn = g + (size_t)e.n * g_ns + (size_t)c * g_cs;
                for (int ph = e.ranges & 255; ph <= ph_hi; ++ph) {
                    int hstart;
                    float h_ratio;
                    const float h = (float)ph * e.bin_h + e.start_h;
                    if (!lattice_axis(h, height, hstart, h_ratio)) continue;
                    const int dy = y - hstart;                        // 0: this row is the point's upper tap row, 1: its lower
                    if (dy != 0 && dy != 1) continue;
                    for (int pw = pw_lo; pw <= pw_hi; ++pw) {
                        int wstart;
                        float w_ratio;
                        const float w = (float)pw * e.bin_w + e.start_w;
                        if (!lattice_axis(w, width, wstart, w_ratio)) continue;
                        const int px = wstart - x0;                   // tile column of the left tap; the right one is px + 1
                        if (px < -1 || px >= BWD_TW) continue;
                        Vec<VEC> gv;
                        if (FUSED) {
                            // the lattice point's gradient from the (up to four) outputs that averaged it
                            const int A = aw - 1;
                            window2x2_adjoint(gv.v, ph, pw, A, A, true,
                                              [&](int oy, int ox) {
                                                  Vec<VEC> t;
                                                  t.load(gn + (size_t)(oy * A + ox) * g_ps);
                                                  return t;
                                              },
                                              [](int, int) { return true; });
                        } else {
                            gv.load(gn + (size_t)(ph * aw + pw) * g_ps);
                        }
                        // roi_align_kernel.cu:137-140: `1.` is a double, `1 - w_ratio` a float
                        const float wl = 1.f - w_ratio;
                        Vec<VEC> left, right;
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            if (dy == 0) {
                                const double up = (double)gv.v[i] * (1. - (double)h_ratio);
                                left.v[i] = (float)(up * (double)wl);
                                right.v[i] = (float)(up * (double)w_ratio);
                            } else {
                                const float down = gv.v[i] * h_ratio;
                                left.v[i] = down * wl;
                                right.v[i] = down * w_ratio;
                            }
                        }
#pragma unroll
                        for (int j = 0; j < BWD_TW; ++j) {
                            if (j == px) {
#pragma unroll
                                for (int i = 0; i < VEC; ++i) acc[j].v[i] = acc[j].v[i] + left.v[i];
                            } else if (j == px + 1) {
#pragma unroll
                                for (int i = 0; i < VEC; ++i) acc[j].v[i] = acc[j].v[i] + right.v[i];
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < BWD_TW; ++j)
                if (x0 + j < width) acc[j].store(row + (size_t)(x0 + j) * map_ps);
        }
        __syncthreads();                                              // the list is rebuilt by the next chunk
    }
}

// adjoint of pool2x2_s1_kernel: one thread per lattice element, window2x2_adjoint() of the outputs' gradient.
// Grid (planes, row groups), block (columns, rows): indices come from the grid, no integer division.  The maximum recomputes
// the argmax of each of those outputs' windows (up to 16 loads of x per element): an op-level drop-in, not a fast path.
__global__ void pool2x2_s1_backward_kernel(const float *__restrict__ gy, const float *__restrict__ x, int h, int w,
                                           float *__restrict__ gx, int take_max)
{
    const int oh = h - 1, ow = w - 1;
    const size_t pl = blockIdx.x;
    const int i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= h) return;
    for (int j = threadIdx.x; j < w; j += blockDim.x) {
        float s[1] = {0.0f};
        window2x2_adjoint(s, i, j, oh, ow, !take_max,
                          [&](int oy, int ox) { return Vec<1>{{gy[(pl * oh + oy) * ow + ox]}}; },
                          [&](int oy, int ox) {
                              if (!take_max) return true;
                              // the output's value came from this element: first_max4 of its window (pool2x2_s1_kernel)
                              const float *p = x + (pl * h + oy) * w + ox;
                              const int arg = first_max4(p[0], p[1], p[w], p[w + 1]).index;
                              return oy + (arg >> 1) == i && ox + (arg & 1) == j;
                          });
        gx[(pl * h + i) * w + j] = s[0];
    }
}

}  // namespace srcnn

extern "C" {

int srcnn_pool2x2_s1_backward(const float *grad_y, const float *x, long long planes, int h, int w, float *grad_x, int take_max,
                              srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(grad_y && grad_x && planes >= 0 && h >= 2 && w >= 2, "bad args (the lattice must be at least 2 x 2)");
    SRCNN_REQUIRE(!take_max || x, "the maximum needs the forward's input x");
    SRCNN_REQUIRE(planes <= 0x7fffffffLL, "too many planes");
    if (planes == 0) return SRCNN_OK;
    int bx = 8;                                                   // columns of a block: a power of two covering w, at most 256
    while (bx < w && bx < 256) bx *= 2;
    const int by = 256 / bx;
    SRCNN_REQUIRE(cdiv(h, by) <= 65535, "lattice too high");
    SRCNN_LAUNCH(pool2x2_s1_backward_kernel, dim3((unsigned)planes, cdiv(h, by)), dim3(bx, by), 0, as_stream(stream), grad_y, x, h, w,
                 grad_x, take_max);
    return check_launch("srcnn_pool2x2_s1_backward");
}

int roi_align_backward_cuda(int aligned_height, int aligned_width, float spatial_scale, const float *top_grad, const float *rois,
                            int num_rois, int roi_cols, float *bottom_grad, int batch, int channels, int height, int width,
                            srcnn_stream_t stream)
{
    using namespace srcnn;
    if (roi_cols != 5) return 0;   // roi_align_cuda.c:54-57
    if (aligned_height < 1 || aligned_width < 1 || aligned_height > 255 || aligned_width > 255 || num_rois < 0 || batch < 0 ||
        channels < 0 || height < 0 || width < 0) {
        set_error("roi_align_backward_cuda: bad sizes (the lattice is 1..255 points a side)");
        return 0;
    }
    if ((long long)batch * channels * height * width == 0) return 1;
    RoiBwdArgs ba = {};
    ba.maps[0] = bottom_grad;
    ba.lv.mh[0] = height, ba.lv.mw[0] = width;
    ba.lv.scale[0] = spatial_scale;
    const int tile_rows = cdiv(height, BWD_TH), ncb = cdiv(channels, 64);
    ba.row0[0] = 0;
    for (int l = 1; l <= 4; ++l) ba.row0[l] = tile_rows;
    if (tile_rows > 65535 || (long long)batch * ncb > 65535) {
        set_error("roi_align_backward_cuda: map too large");
        return 0;
    }
    dim3 grid(cdiv(width, BWD_TW), tile_rows, batch * ncb), block(64, BWD_TH);
    const int q = aligned_height * aligned_width;
    SRCNN_LAUNCH((roi_align_backward_kernel<1, false>), grid, block, 0, as_stream(stream), ba, rois, num_rois, aligned_height,
                 aligned_width, top_grad, (long long)channels * q, 1, q, channels, ncb, (long long)height * width, 1);
    return check_launch("roi_align_backward_cuda") == SRCNN_OK ? 1 : 0;
}

int srcnn_pyramid_roi_align_backward(const float *grad_out, int out_cstride, int out_coffset, const float *rois, int num_rois, int A,
                                     int channels, float im_height, float *const *grad_maps_host, const int *mh_host,
                                     const int *mw_host, int batch, int maps_format, const int *roi_limit, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(maps_format == SRCNN_FMT_F32, "gradient maps are F32 only");
    SRCNN_REQUIRE(channels > 0 && channels % 64 == 0 && channels <= 1024, "channels must be a multiple of 64, <= 1024");
    SRCNN_REQUIRE(A == 7 || A == 14, "A must be 7 or 14");
    SRCNN_REQUIRE(out_cstride % 4 == 0 && out_coffset % 4 == 0 && out_coffset >= 0 && out_coffset + channels <= out_cstride,
                  "the channel slice must lie inside out_cstride, both multiples of 4");
    SRCNN_REQUIRE(num_rois >= 0 && batch >= 0 && grad_maps_host && mh_host && mw_host, "bad args");
    if (batch == 0) return SRCNN_OK;
    RoiBwdArgs ba = {};
    ba.lv = roi_levels(mh_host, mw_host, im_height, roi_limit);
    ba.route = 1;
    int wmax = 0;
    ba.row0[0] = 0;
    for (int l = 0; l < 4; ++l) {
        SRCNN_REQUIRE(grad_maps_host[l] && mh_host[l] > 0 && mw_host[l] > 0, "bad map");
        ba.maps[l] = grad_maps_host[l];
        ba.row0[l + 1] = ba.row0[l] + cdiv(mh_host[l], BWD_TH);
        wmax = mw_host[l] > wmax ? mw_host[l] : wmax;
    }
    const int ncb = cdiv(channels, 256);
    SRCNN_REQUIRE(ba.row0[4] <= 65535 && (long long)batch * ncb <= 65535, "maps too large");
    dim3 grid(cdiv(wmax, BWD_TW), ba.row0[4], batch * ncb), block(64, BWD_TH);
    SRCNN_LAUNCH((roi_align_backward_kernel<4, true>), grid, block, 0, as_stream(stream), ba, rois, num_rois, A + 1, A + 1,
                 grad_out + out_coffset, (long long)A * A * out_cstride, out_cstride, 1, channels, ncb, 1LL, channels);
    return check_launch("srcnn_pyramid_roi_align_backward");
}

}  // extern "C"
