// Result visualisation (include/srcnn_hip.h, "result visualisation"):
//   srcnn_render_overlay   demo.py:225-333 -- the left image over the right image with the 2-D boxes (net_utils.vis_detections),
//                          the projected 3-D wireframes (vis_3d_utils.vis_single_box_in_img) and the bird's-eye view with the 3-D
//                          boxes (vis_box_in_bev), drawn from one detection record that never leaves the device;
//   srcnn_bev_lidar        kitti_utils.get_point_cloud + vis_3d_utils.vis_lidar_in_bev -- the gray plane behind the bird's-eye view.
// Two launches: overlay_segments_kernel turns the record into a list of segments at FIXED slots (26 per record row, dead ones
// flagged), overlay_pixels_kernel is a gather over the panel -- a thread owns pixels and asks every segment whose bounding box
// meets its tile whether it covers them (the rasterisation rule is a closed-form membership test), the last one wins.  Every
// panel byte is written exactly once, no atomics: the panel is bit-repeatable whatever the launch geometry.
#include "common.h"
#include <climits>
#include <cmath>

namespace srcnn {

#define OVL_WG 256
#define OVL_TILE_W 64
#define OVL_COORD_LIMIT 1073741824.0          // 2^30

struct OverlayArgs {
    double p2[12];
    double res;
    int H, W, x_max, x_off, y_off, n, layers;
    float vis_thresh;
};

// slot layout: [0, 8 n) 2-D boxes (row r: left 8 r .. 8 r + 3, right 8 r + 4 .. 8 r + 7), [8 n, 20 n) wireframes, [20 n, 26 n)
// bird's-eye boxes: ascending slot = draw order on every target (the three targets do not overlap)
struct SegmentList {
    int4 *ends;       // x0, y0, x1, y1 in PANEL coordinates (|v| <= 2^30 + panel size)
    int4 *bbox;       // inclusive pixel bounds of the stamped segment clipped to its target, panel coordinates; dead: empty
    int *style;       // thickness | R << 8 | G << 16 | B << 24
};

// the reference's int(): clamp first (NaN -> -2^30), then truncate toward zero
__device__ __forceinline__ long long clamp_trunc(double v)
{
    v = v > -OVL_COORD_LIMIT ? v : -OVL_COORD_LIMIT;
    v = v < OVL_COORD_LIMIT ? v : OVL_COORD_LIMIT;
    return (long long)v;
}

__device__ __forceinline__ void dead_slot(const SegmentList &s, int slot)
{
    s.ends[slot] = make_int4(0, 0, 0, 0);
    s.bbox[slot] = make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN);
    s.style[slot] = 0;
}

// target rectangle: origin (ox, oy), size (tw, th) in panel coordinates; (x0, y0) - (x1, y1) in the target's own coordinates
__device__ void put_segment(const SegmentList &s, int slot, int ox, int oy, int tw, int th, long long x0, long long y0,
                            long long x1, long long y1, int thick, int rgb)
{
    const long long lo = -(thick / 2), hi = (thick - 1) / 2;
    const long long bx0 = max(min(x0, x1) + lo, 0ll), bx1 = min(max(x0, x1) + hi, (long long)tw - 1);
    const long long by0 = max(min(y0, y1) + lo, 0ll), by1 = min(max(y0, y1) + hi, (long long)th - 1);
    if (bx0 > bx1 || by0 > by1) {
        dead_slot(s, slot);
        return;
    }
    s.ends[slot] = make_int4((int)(x0 + ox), (int)(y0 + oy), (int)(x1 + ox), (int)(y1 + oy));
    s.bbox[slot] = make_int4((int)bx0 + ox, (int)by0 + oy, (int)bx1 + ox, (int)by1 + oy);
    s.style[slot] = thick | (rgb << 8);
}

#define OVL_RED (204 | (0 << 8) | (0 << 16))
#define OVL_GREEN (0 | (200 << 8) | (0 << 16))

// one thread per record row: its 26 slots, live or dead
__global__ __launch_bounds__(OVL_WG) void overlay_segments_kernel(const float *__restrict__ rec, OverlayArgs a, SegmentList s)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    const float cf = rec[0];
    const int count = cf > 0.f ? (cf < (float)a.n ? (int)cf : a.n) : 0;          // NaN -> 0
    const float *row = rec + (size_t)(r + 1) * SRCNN_REC_COLS;
    const bool shown = r < count && row[0] > a.vis_thresh;
    const int box_slot = 8 * r, wire_slot = 8 * a.n + 12 * r, bev_slot = 20 * a.n + 6 * r;

    if (shown && r < 100 && (a.layers & SRCNN_OVERLAY_BOXES)) {                    // net_utils.py:54-58
        for (int eye = 0; eye < 2; ++eye) {
            const float *b = row + 1 + 4 * eye;
            const long long x1 = clamp_trunc((double)rintf(b[0])), y1 = clamp_trunc((double)rintf(b[1]));
            const long long x2 = clamp_trunc((double)rintf(b[2])), y2 = clamp_trunc((double)rintf(b[3]));
            const int oy = eye * a.H, k = box_slot + 4 * eye;
            put_segment(s, k + 0, 0, oy, a.W, a.H, x1, y1, x2, y1, 1, OVL_RED);
            put_segment(s, k + 1, 0, oy, a.W, a.H, x2, y1, x2, y2, 1, OVL_RED);
            put_segment(s, k + 2, 0, oy, a.W, a.H, x2, y2, x1, y2, 1, OVL_RED);
            put_segment(s, k + 3, 0, oy, a.W, a.H, x1, y2, x1, y1, 1, OVL_RED);
        }
    } else {
        for (int k = 0; k < 8; ++k) dead_slot(s, box_slot + k);
    }

    const bool solid = shown && row[25] > 0.f;
    // the eight corners (vis_3d_utils.py:130-142), float64
    const double w = (double)row[9], h = (double)row[10], l = (double)row[11];
    const double px = (double)row[27], py = (double)row[28], pz = (double)row[29], theta = (double)row[30];
    const double c = cos(theta), sn = sin(theta);
    double cx[8], cy[8], cz[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double va = (i & 3) == 0 || (i & 3) == 1 ? -w : w;
        const double vd = (i & 3) == 0 || (i & 3) == 3 ? -l : l;
        const double vb = i < 4 ? 0.0 : -h * 2.0;
        cx[i] = px + (c * va + sn * vd) / 2.0;
        cy[i] = py + vb / 2.0;
        cz[i] = pz + (-sn * va + c * vd) / 2.0;
    }

    bool wire = solid && (a.layers & SRCNN_OVERLAY_WIREFRAMES);
    if (wire) {
#pragma unroll
        for (int i = 0; i < 8; ++i) wire = wire && !(cz[i] < 0.0);               // :146-147: one corner behind the camera drops the box
    }
    if (wire) {
        long long u[8], v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {                                              // Space2Image with P2[:, 0:3]
            const double un = a.p2[0] * cx[i] + a.p2[1] * cy[i] + a.p2[2] * cz[i];
            const double vn = a.p2[4] * cx[i] + a.p2[5] * cy[i] + a.p2[6] * cz[i];
            const double wn = a.p2[8] * cx[i] + a.p2[9] * cy[i] + a.p2[10] * cz[i];
            u[i] = clamp_trunc(un / wn);
            v[i] = clamp_trunc(vn / wn);
        }
        const int e0[12] = {0, 1, 2, 0, 4, 5, 6, 7, 4, 5, 6, 7}, e1[12] = {1, 2, 3, 3, 5, 6, 7, 4, 0, 1, 2, 3};
#pragma unroll
        for (int k = 0; k < 12; ++k)
            put_segment(s, wire_slot + k, 0, 0, a.W, a.H, u[e0[k]], v[e0[k]], u[e1[k]], v[e1[k]], 1, OVL_GREEN);
    } else {
        for (int k = 0; k < 12; ++k) dead_slot(s, wire_slot + k);
    }

    if (solid && a.x_max > 0 && (a.layers & SRCNN_OVERLAY_BEV_BOXES)) {            // vis_3d_utils.py:85-113
        const double tip = l * 2.0 / 3.0;
        long long bx[5], by[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const double X = i < 4 ? cx[i] : px + sn * tip, Z = i < 4 ? cz[i] : pz + c * tip;
            bx[i] = clamp_trunc(X / a.res) - a.x_off;                              // Space2Bev
            by[i] = clamp_trunc(-Z / a.res) + a.y_off;
        }
        const int e0[6] = {0, 1, 2, 0, 1, 2}, e1[6] = {1, 2, 3, 3, 4, 4};
#pragma unroll
        for (int k = 0; k < 6; ++k)
            put_segment(s, bev_slot + k, a.W, 0, a.x_max, 2 * a.H, bx[e0[k]], by[e0[k]], bx[e1[k]], by[e1[k]], 2, OVL_GREEN);
    } else {
        for (int k = 0; k < 6; ++k) dead_slot(s, bev_slot + k);
    }
}

// the rasterisation rule as a membership test: does the segment e, stamped with thickness t, cover pixel (px, py)?
// major / minor: the pixel's and the segment's coordinates along the longer and the shorter extent
__device__ __forceinline__ bool covers_major(long long m0, long long n0, long long dm, long long dn, int t, long long pm, long long pn)
{
    const unsigned long long am = (unsigned long long)(dm < 0 ? -dm : dm), an = (unsigned long long)(dn < 0 ? -dn : dn);
    const int lo = -(t / 2), hi = (t - 1) / 2;
    for (int d = lo; d <= hi; ++d) {
        const long long mi = pm - d;
        const long long i = dm >= 0 ? mi - m0 : m0 - mi;
        if (i < 0 || (unsigned long long)i > am) continue;
        unsigned long long step = 0;
        if (am != 0) {
            if ((am | an) < 32768ull)                                              // 2 i an + am < 2^31: one 32-bit division
                step = (2u * (unsigned)i * (unsigned)an + (unsigned)am) / (2u * (unsigned)am);
            else                                                                   // i, an <= am <= 2^31 + panel: below 2^64
                step = (2ull * (unsigned long long)i * an + am) / (2ull * am);
        }
        const long long ni = dn >= 0 ? n0 + (long long)step : n0 - (long long)step;
        const long long off = pn - ni;
        if (off >= lo && off <= hi) return true;
    }
    return false;
}

__device__ __forceinline__ bool covers(const int4 e, int t, int px, int py)
{
    const long long dx = (long long)e.z - e.x, dy = (long long)e.w - e.y;
    const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    return adx >= ady ? covers_major(e.x, e.y, dx, dy, t, px, py) : covers_major(e.y, e.x, dy, dx, t, py, px);
}

// A workgroup owns a tile of 64 x (4 RPT) panel pixels; wave v of it the rows v, v + 4, ...; a thread one column of those.
// Per chunk of 256 slots: every thread tests one slot's bounding box against the tile, the hits are compacted in slot order
// into LDS (wave ballots, no atomics), then every thread walks the hits for its RPT pixels.
template <int RPT>
__global__ __launch_bounds__(OVL_WG) void overlay_pixels_kernel(const unsigned char *__restrict__ left,
                                                                const unsigned char *__restrict__ right,
                                                                const unsigned char *__restrict__ plane, int H, int W, int x_max,
                                                                SegmentList s, int n_slots, unsigned char *__restrict__ panel)
{
    __shared__ int4 hit_ends[OVL_WG], hit_bbox[OVL_WG];
    __shared__ int hit_style[OVL_WG];
    __shared__ int wave_hits[OVL_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int PW = W + x_max, PH = 2 * H;
    const int tx0 = blockIdx.x * OVL_TILE_W, ty0 = blockIdx.y * (4 * RPT);
    const int tx1 = min(tx0 + OVL_TILE_W, PW) - 1, ty1 = min(ty0 + 4 * RPT, PH) - 1;
    const int px = tx0 + lane;
    int colour[RPT];
#pragma unroll
    for (int j = 0; j < RPT; ++j) colour[j] = 0;                                   // 0 = no segment (a live style has a thickness)

    for (int base = 0; base < n_slots; base += OVL_WG) {
        const int slot = base + tid;
        int4 bb = make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN);
        if (slot < n_slots) bb = s.bbox[slot];
        const bool hit = bb.x <= tx1 && bb.z >= tx0 && bb.y <= ty1 && bb.w >= ty0;
        const unsigned long long ballot = __ballot(hit);
        if (lane == 0) wave_hits[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int v = 0; v < OVL_WG / 64; ++v) {
            const int c = wave_hits[v];
            before += v < wave ? c : 0;
            total += c;
        }
        if (hit) {
            const int at = before + __popcll(ballot & ((1ull << lane) - 1ull));
            hit_ends[at] = s.ends[slot];
            hit_bbox[at] = bb;
            hit_style[at] = s.style[slot];
        }
        __syncthreads();
        for (int k = 0; k < total; ++k) {
            const int4 hb = hit_bbox[k];
            if (px < hb.x || px > hb.z) continue;
            const int4 e = hit_ends[k];
            const int st = hit_style[k];
#pragma unroll
            for (int j = 0; j < RPT; ++j) {
                const int py = ty0 + 4 * j + wave;
                if (py >= hb.y && py <= hb.w && covers(e, st & 255, px, py)) colour[j] = st;
            }
        }
        __syncthreads();                                                           // the lists are rewritten by the next chunk
    }

    if (px >= PW) return;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const int py = ty0 + 4 * j + wave;
        if (py >= PH) continue;
        unsigned char r, g, b;
        if (colour[j] != 0) {
            r = (unsigned char)(colour[j] >> 8);
            g = (unsigned char)(colour[j] >> 16);
            b = (unsigned char)(colour[j] >> 24);
        } else if (px < W) {
            const unsigned char *src = (py < H ? left + ((size_t)py * W + px) * 3 : right + ((size_t)(py - H) * W + px) * 3);
            r = src[0];
            g = src[1];
            b = src[2];
        } else {
            r = g = b = plane ? plane[(size_t)py * x_max + (px - W)] : (unsigned char)255;
        }
        unsigned char *dst = panel + ((size_t)py * PW + px) * 3;
        dst[0] = r;
        dst[1] = g;
        dst[2] = b;
    }
}

struct LidarArgs {
    double m[12];
    double res;
    int x_max, y_max, x_off, y_off;
};

__global__ __launch_bounds__(256) void bev_lidar_kernel(const float4 *__restrict__ points, int n, LidarArgs a,
                                                        unsigned char *__restrict__ plane)
{
    // 64-bit index: n may lie within one grid stride of INT_MAX
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float4 p = points[i];
        const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
        const double X = a.m[0] * x + a.m[1] * y + a.m[2] * z + a.m[3];            // kitti_utils.py:334-337, rows 0 and 2
        const double Z = a.m[8] * x + a.m[9] * y + a.m[10] * z + a.m[11];
        if (!(Z > 0.0 && Z < 70.0 && X > -20.0 && X < 20.0)) continue;             // vis_3d_utils.py:49-51 (NaN: dropped)
        long long xi = (long long)(X / a.res) - a.x_off, yi = (long long)(-Z / a.res) + a.y_off;      // :53-57
        xi = min(xi, (long long)a.x_max - 1);                                      // :62-63: the upper bound only
        yi = min(yi, (long long)a.y_max - 1);
        if (xi < 0 || yi < 0) continue;                                            // numpy would wrap; cannot occur (header)
        plane[(size_t)yi * a.x_max + (size_t)xi] = 100;
    }
}

static bool overlaps(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace srcnn

extern "C" {

size_t srcnn_overlay_workspace_bytes(int max_det)
{
    using namespace srcnn;
    const size_t slots = (size_t)SRCNN_OVERLAY_SLOTS_PER_ROW * (size_t)(max_det > 0 ? max_det : 0);
    return align_up(slots * sizeof(int4), 256) * 2 + align_up(slots * sizeof(int), 256) + 256;
}

int srcnn_render_overlay(const unsigned char *left, const unsigned char *right, int H, int W, const float *rec, int max_det,
                         int rec_cols, const double *p2_host, float vis_thresh, const unsigned char *bev_plane, double res,
                         int x_max, int y_max, int x_off, int y_off, int layers, int rows_per_thread, unsigned char *panel,
                         void *workspace, size_t workspace_bytes, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(left && right, "null image pointer");
    SRCNN_REQUIRE(rec, "null record");
    SRCNN_REQUIRE(p2_host, "null p2_host");
    SRCNN_REQUIRE(panel, "null panel");
    SRCNN_REQUIRE(workspace, "null workspace");
    SRCNN_REQUIRE(H > 0 && W > 0 && H <= 32768 && W <= 32768, "H and W must be 1..32768");
    SRCNN_REQUIRE(max_det >= 0 && max_det <= 4096, "max_det must be 0..4096");
    SRCNN_REQUIRE(rec_cols == SRCNN_REC_COLS, "rec_cols must be SRCNN_REC_COLS");
    SRCNN_REQUIRE(x_max >= 0 && x_max <= 65536, "x_max must be 0..65536");
    SRCNN_REQUIRE(x_max == 0 || y_max == 2 * H, "y_max must equal 2 H (the bird's-eye view stands beside both images)");
    SRCNN_REQUIRE(std::isfinite(res) && res > 0.0, "res must be finite and positive");
    SRCNN_REQUIRE(x_off >= -SRCNN_OVERLAY_MAX_OFFSET && x_off <= SRCNN_OVERLAY_MAX_OFFSET && y_off >= -SRCNN_OVERLAY_MAX_OFFSET &&
                      y_off <= SRCNN_OVERLAY_MAX_OFFSET,
                  "x_off and y_off must lie within +-SRCNN_OVERLAY_MAX_OFFSET");      // end points stay inside 32 bits
    SRCNN_REQUIRE(std::isfinite(vis_thresh), "vis_thresh must be finite");
    SRCNN_REQUIRE(layers >= 0 && layers <= 7, "layers must be 0..7");
    SRCNN_REQUIRE(rows_per_thread == 0 || rows_per_thread == 1 || rows_per_thread == 2 || rows_per_thread == 4 || rows_per_thread == 8,
                  "rows_per_thread must be 0, 1, 2, 4 or 8");
    const size_t image_bytes = (size_t)H * W * 3, panel_bytes = (size_t)2 * H * ((size_t)W + x_max) * 3;
    SRCNN_REQUIRE(!overlaps(panel, panel_bytes, left, image_bytes) && !overlaps(panel, panel_bytes, right, image_bytes),
                  "the panel overlaps an input image");
    SRCNN_REQUIRE(!overlaps(panel, panel_bytes, rec, (size_t)(max_det + 1) * SRCNN_REC_COLS * sizeof(float)),
                  "the panel overlaps the record");
    SRCNN_REQUIRE(!bev_plane || !overlaps(panel, panel_bytes, bev_plane, (size_t)y_max * x_max), "the panel overlaps the bev plane");
    if (workspace_bytes < srcnn_overlay_workspace_bytes(max_det)) {
        set_error("srcnn_render_overlay: workspace too small");
        return SRCNN_ERR_WORKSPACE;
    }
    SRCNN_REQUIRE(!overlaps(panel, panel_bytes, workspace, srcnn_overlay_workspace_bytes(max_det)), "the panel overlaps the workspace");

    OverlayArgs a;
    for (int i = 0; i < 12; ++i) a.p2[i] = p2_host[i];
    a.res = res;
    a.H = H;
    a.W = W;
    a.x_max = x_max;
    a.x_off = x_off;
    a.y_off = y_off;
    a.n = max_det;
    a.layers = layers;
    a.vis_thresh = vis_thresh;
    const size_t slots = (size_t)SRCNN_OVERLAY_SLOTS_PER_ROW * (size_t)max_det;
    Carver carve(workspace);
    SegmentList s;
    s.ends = carve.take<int4>(slots);
    s.bbox = carve.take<int4>(slots);
    s.style = carve.take<int>(slots);
    hipStream_t st = as_stream(stream);
    if (max_det > 0) SRCNN_LAUNCH(overlay_segments_kernel, dim3(cdiv(max_det, OVL_WG)), dim3(OVL_WG), 0, st, rec, a, s);
    const int rpt = rows_per_thread ? rows_per_thread : 4;
    const dim3 grid(cdiv(W + x_max, OVL_TILE_W), cdiv(2 * H, 4 * rpt));
    const unsigned char *plane = x_max > 0 ? bev_plane : nullptr;
    switch (rpt) {
    case 1: SRCNN_LAUNCH(overlay_pixels_kernel<1>, grid, dim3(OVL_WG), 0, st, left, right, plane, H, W, x_max, s, (int)slots, panel); break;
    case 2: SRCNN_LAUNCH(overlay_pixels_kernel<2>, grid, dim3(OVL_WG), 0, st, left, right, plane, H, W, x_max, s, (int)slots, panel); break;
    case 4: SRCNN_LAUNCH(overlay_pixels_kernel<4>, grid, dim3(OVL_WG), 0, st, left, right, plane, H, W, x_max, s, (int)slots, panel); break;
    default: SRCNN_LAUNCH(overlay_pixels_kernel<8>, grid, dim3(OVL_WG), 0, st, left, right, plane, H, W, x_max, s, (int)slots, panel); break;
    }
    return check_launch("srcnn_render_overlay");
}

int srcnn_bev_lidar(const float *points, int n_points, const double *velo_to_cam2_host, double res, int x_max, int y_max, int x_off,
                    int y_off, unsigned char *plane, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(plane, "null plane");
    SRCNN_REQUIRE(velo_to_cam2_host, "null velo_to_cam2_host");
    SRCNN_REQUIRE(n_points >= 0, "negative n_points");
    SRCNN_REQUIRE(n_points == 0 || points, "null points");
    SRCNN_REQUIRE((uintptr_t)points % 16 == 0, "points must be 16-byte aligned");
    SRCNN_REQUIRE(x_max > 0 && y_max > 0 && x_max <= 65536 && y_max <= 65536, "x_max and y_max must be 1..65536");
    SRCNN_REQUIRE(std::isfinite(res) && res > 0.0, "res must be finite and positive");
    SRCNN_REQUIRE(x_off >= -SRCNN_OVERLAY_MAX_OFFSET && x_off <= SRCNN_OVERLAY_MAX_OFFSET && y_off >= -SRCNN_OVERLAY_MAX_OFFSET &&
                      y_off <= SRCNN_OVERLAY_MAX_OFFSET,
                  "x_off and y_off must lie within +-SRCNN_OVERLAY_MAX_OFFSET");
    SRCNN_REQUIRE(n_points == 0 || !overlaps(plane, (size_t)x_max * y_max, points, (size_t)n_points * 16), "the plane overlaps the points");
    LidarArgs a;
    for (int i = 0; i < 12; ++i) a.m[i] = velo_to_cam2_host[i];
    a.res = res;
    a.x_max = x_max;
    a.y_max = y_max;
    a.x_off = x_off;
    a.y_off = y_off;
    hipStream_t st = as_stream(stream);
    SRCNN_HIP_TRY(memset_async(plane, 255, (size_t)x_max * y_max, st));
    if (n_points > 0)
        SRCNN_LAUNCH(bev_lidar_kernel, dim3(grid_for(n_points, 256, 2048)), dim3(256), 0, st, reinterpret_cast<const float4 *>(points),
                     n_points, a, plane);
    return check_launch("srcnn_bev_lidar");
}

}  // extern "C"
