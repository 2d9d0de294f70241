// KITTI object evaluation on the device (gfx950): the overlaps and the greedy per-frame matches of the KITTI object
// devkit (evaluate_object_3d_offline: boxoverlap / groundBoxOverlap / box3DOverlap and computeStatistics), restated.
//
//   * kitti_overlaps_kernel: one workgroup per frame, one thread per (gt, det) pair; 2-D IoU, rotated-rectangle BEV IoU
//     (Sutherland-Hodgman clipping of one 4-gon by the other, shoelace area) and 3-D IoU, plus the criterion-0 image overlap
//     of every (don't-care, det) pair.  float64 throughout, no "+1".
//   * kitti_match_kernel: one wavefront per (configuration, threshold slot, frame).  Ground truths are walked in file order;
//     the frame's detections lie across the lanes in 64-wide chunks and each greedy choice is a cross-lane reduction:
//       pass 1 (compute_fp = 0): the candidate with the highest score, ties to the lowest index;
//       pass 2 (compute_fp = 1): the non-ignored candidate with the largest overlap, ties to the lowest index, else the
//         lowest-index ignored candidate -- what the devkit's sequential `(overlap > max_iou || assigned_ignored_det)`
//         state machine reduces to (tests/kitti_eval_ref.py checks the reduction against the literal loop; the reduction over several
//         chunks per lane -- frames of more than 64 detections -- is checked on the device by tests/test_kitti_eval_crowded_gpu.py).
//     A lane keeps the "assigned" flags of its detections as bits of one 64-bit word (bit c = chunk c), which is what
//     bounds a frame to SRCNN_KITTI_MAX_DET = 64 x 64 detections.  Counts are integers, the similarity is summed in
//     ground-truth order by every lane alike: no atomics, the same bits on every run.
#include "common.h"
#include <climits>

namespace srcnn {

namespace {

constexpr int KC = SRCNN_KITTI_COLS;
static_assert(SRCNN_KITTI_MAX_DET <= 64 * 64, "assigned flags are one 64-bit word per lane");

// columns of a row
constexpr int C_X1 = 0, C_Y1 = 1, C_X2 = 2, C_Y2 = 3, C_H = 4, C_W = 5, C_L = 6, C_X = 7, C_Y = 8, C_Z = 9, C_RY = 10,
              C_ALPHA = 11, C_SCORE = 12;

struct Pt {
    double x, z;
};

__device__ inline double image_overlap(const double *a, const double *b, bool over_a)
{
    double x1 = fmax(a[C_X1], b[C_X1]), y1 = fmax(a[C_Y1], b[C_Y1]);
    double x2 = fmin(a[C_X2], b[C_X2]), y2 = fmin(a[C_Y2], b[C_Y2]);
    double w = x2 - x1, h = y2 - y1;
    if (w <= 0.0 || h <= 0.0) return 0.0;
    double inter = w * h;
    double area_a = (a[C_X2] - a[C_X1]) * (a[C_Y2] - a[C_Y1]);
    double area_b = (b[C_X2] - b[C_X1]) * (b[C_Y2] - b[C_Y1]);
    double den = over_a ? area_a : area_a + area_b - inter;
    return den > 0.0 ? inter / den : 0.0;
}

// ground-plane corners: (x, z) + R c, R = [[cos ry, sin ry], [-sin ry, cos ry]]
__device__ inline void footprint(const double *b, Pt *p)
{
    double c = cos(b[C_RY]), s = sin(b[C_RY]);
    double hl = b[C_L] / 2.0, hw = b[C_W] / 2.0;
    const double cx[4] = {hl, hl, -hl, -hl}, cz[4] = {hw, -hw, -hw, hw};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p[k].x = b[C_X] + (c * cx[k] + s * cz[k]);
        p[k].z = b[C_Z] + (-s * cx[k] + c * cz[k]);
    }
}

__device__ inline double signed_area(const Pt *p, int n)
{
    double a = 0.0;
    for (int k = 0; k < n; ++k) {
        const Pt &u = p[k], &v = p[k + 1 == n ? 0 : k + 1];
        a += u.x * v.z - v.x * u.z;
    }
    return a / 2.0;
}

constexpr int POLY_CAP = 16;   // a convex 4-gon clipped by 4 half-planes has at most 8 vertices

// area of the intersection of two convex quadrilaterals: `a` clipped by the four edge half-planes of `b`
__device__ inline double quad_intersection(const Pt *a, const Pt *b)
{
    double ob = signed_area(b, 4);
    if (ob == 0.0 || signed_area(a, 4) == 0.0) return 0.0;     // zero extent: no area to share
    double orient = ob > 0.0 ? 1.0 : -1.0;                        // inside = left of each edge for a counter-clockwise b
    Pt buf[2][POLY_CAP];
    int n = 4;
    for (int k = 0; k < 4; ++k) buf[0][k] = a[k];
    int cur = 0;
    for (int e = 0; e < 4 && n > 0; ++e) {
        const Pt p = b[e], q = b[e == 3 ? 0 : e + 1];
        const double ex = q.x - p.x, ez = q.z - p.z;
        const Pt *in = buf[cur];
        Pt *out = buf[cur ^ 1];
        int m = 0;
        for (int k = 0; k < n; ++k) {
            const Pt v = in[k], u = in[k == 0 ? n - 1 : k - 1];
            double sv = orient * (ex * (v.z - p.z) - ez * (v.x - p.x));
            double su = orient * (ex * (u.z - p.z) - ez * (u.x - p.x));
            if ((sv >= 0.0) != (su >= 0.0) && m < POLY_CAP) {     // the edge u -> v crosses the line: signs differ strictly
                double t = su / (su - sv);
                out[m].x = u.x + t * (v.x - u.x);
                out[m].z = u.z + t * (v.z - u.z);
                ++m;
            }
            if (sv >= 0.0 && m < POLY_CAP) out[m++] = v;
        }
        n = m;
        cur ^= 1;
    }
    return n >= 3 ? fabs(signed_area(buf[cur], n)) : 0.0;
}

__global__ __launch_bounds__(256) void kitti_overlaps_kernel(srcnn_kitti_split s)
{
    const int f = blockIdx.x;
    const int d0 = s.det_off[f], nd = s.det_off[f + 1] - d0;
    const int g0 = s.gt_off[f], ng = s.gt_off[f + 1] - g0;
    const int c0 = s.dc_off[f], nc = s.dc_off[f + 1] - c0;
    const long long pb = s.pair_off[f], cb = s.dcpair_off[f];
    for (int p = threadIdx.x; p < ng * nd; p += blockDim.x) {
        const int i = p / nd, j = p - i * nd;
        const double *d = s.det + (size_t)(d0 + j) * KC, *g = s.gt + (size_t)(g0 + i) * KC;
        s.ov_img[pb + p] = image_overlap(d, g, false);
        Pt pd[4], pg[4];
        footprint(d, pd);
        footprint(g, pg);
        double inter = quad_intersection(pd, pg);
        double area_d = d[C_L] * d[C_W], area_g = g[C_L] * g[C_W];
        double den = area_d + area_g - inter;
        s.ov_bev[pb + p] = den > 0.0 ? inter / den : 0.0;
        double ymax = fmin(d[C_Y], g[C_Y]), ymin = fmax(d[C_Y] - d[C_H], g[C_Y] - g[C_H]);
        double inter3 = inter * fmax(0.0, ymax - ymin);
        double vol_d = d[C_H] * d[C_W] * d[C_L], vol_g = g[C_H] * g[C_W] * g[C_L];
        double den3 = vol_d + vol_g - inter3;
        s.ov_3d[pb + p] = den3 > 0.0 ? inter3 / den3 : 0.0;
    }
    for (int p = threadIdx.x; p < nc * nd; p += blockDim.x) {
        const int k = p / nd, j = p - k * nd;
        s.ov_dc[cb + p] = image_overlap(s.det + (size_t)(d0 + j) * KC, s.dc + (size_t)(c0 + k) * KC, true);
    }
}

__device__ inline int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int WAVES = 4;

__global__ __launch_bounds__(64 * WAVES) void kitti_match_kernel(srcnn_kitti_split s, srcnn_kitti_match_desc m,
                                                                  long long n_items)
{
    const long long item = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (item >= n_items) return;                                  // wave-uniform
    const int f = (int)(item % s.n_frames);
    const long long r = item / s.n_frames;
    const int slot = (int)(r % m.n_slots), c = (int)(r / m.n_slots);
    const bool fp_mode = m.compute_fp != 0;
    const long long out = r * s.n_frames + f;
    const int d0 = s.det_off[f], nd = s.det_off[f + 1] - d0;
    const int g0 = s.gt_off[f], ng = s.gt_off[f + 1] - g0;
    const int metric = m.cfg_metric[c], fs = m.cfg_flags[c];
    const double min_ov = m.cfg_min_overlap[c];
    if (fp_mode && slot >= m.cfg_n_thresh[c]) {
        if (lane == 0) {
            m.tp[out] = 0; m.fp[out] = 0; m.fn[out] = 0; m.similarity[out] = 0.0;
        }
        return;
    }
    if (nd > SRCNN_KITTI_MAX_DET) {                               // the host refuses such a split; never write past a lane's flags
        if (lane == 0 && fp_mode) {
            m.tp[out] = -1; m.fp[out] = -1; m.fn[out] = -1; m.similarity[out] = 0.0;
        }
        return;
    }
    const double thresh = fp_mode ? m.thresholds[(long long)c * m.n_slots + slot] : -INFINITY;
    const double *ov = metric == 0 ? s.ov_img : metric == 1 ? s.ov_bev : s.ov_3d;
    ov += s.pair_off[f];
    const signed char *igt = m.ign_gt + (long long)fs * m.n_gt_total + g0;
    const signed char *idet = m.ign_det + (long long)fs * m.n_det_total + d0;
    const double *det = s.det + (size_t)d0 * KC;
    const int chunks = (nd + 63) >> 6;
    unsigned long long assigned = 0;
    int tp = 0, fn = 0;
    double sim = 0.0;

    for (int i = 0; i < ng; ++i) {
        const int ig = igt[i];
        double *score_slot = fp_mode ? nullptr : m.gt_score + (long long)c * m.n_gt_total + g0 + i;
        if (ig == -1) {
            if (score_slot && lane == 0) *score_slot = -INFINITY;
            continue;
        }
        const double *row = ov + (long long)i * nd;
        double bkey = -INFINITY;                                  // pass 1: score; pass 2: overlap of a non-ignored candidate
        int bidx = INT_MAX, ign_first = INT_MAX;
        for (int ch = 0; ch < chunks; ++ch) {
            const int j = (ch << 6) + lane;
            if (j >= nd || ((assigned >> ch) & 1ull)) continue;
            const int id = idet[j];
            if (id == -1) continue;
            const double sc = det[(size_t)j * KC + C_SCORE];
            if (fp_mode && sc < thresh) continue;
            const double o = row[j];
            if (!(o > min_ov)) continue;
            if (!fp_mode || id == 0) {
                const double key = fp_mode ? o : sc;
                if (bidx == INT_MAX || key > bkey) { bkey = key; bidx = j; }   // ascending j per lane: ties keep the first
            } else if (j < ign_first) {
                ign_first = j;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ok = __shfl_xor(bkey, o, 64);
            const int oi = __shfl_xor(bidx, o, 64);
            if (oi != INT_MAX && (bidx == INT_MAX || ok > bkey || (ok == bkey && oi < bidx))) { bkey = ok; bidx = oi; }
            ign_first = min(ign_first, __shfl_xor(ign_first, o, 64));
        }
        const int j = bidx != INT_MAX ? bidx : ign_first;        // pass 1 never sets ign_first
        if (j == INT_MAX) {
            if (ig == 0) ++fn;
            if (score_slot && lane == 0) *score_slot = -INFINITY;
            continue;
        }
        if (ig == 1 || idet[j] == 1) {
            if (score_slot && lane == 0) *score_slot = -INFINITY;
        } else {
            ++tp;
            if (score_slot && lane == 0) *score_slot = det[(size_t)j * KC + C_SCORE];
            if (fp_mode && metric == 0)
                sim += (1.0 + cos(s.gt[(size_t)(g0 + i) * KC + C_ALPHA] - det[(size_t)j * KC + C_ALPHA])) / 2.0;
        }
        if ((j & 63) == lane) assigned |= 1ull << (j >> 6);
    }
    if (!fp_mode) return;

    int fp_l = 0;
    for (int ch = 0; ch < chunks; ++ch) {
        const int j = (ch << 6) + lane;
        if (j < nd && !((assigned >> ch) & 1ull) && idet[j] == 0 && !(det[(size_t)j * KC + C_SCORE] < thresh)) ++fp_l;
    }
    if (metric == 0) {                                           // detections inside don't-care regions are not false
        const int nc = s.dc_off[f + 1] - s.dc_off[f];
        const double *dcov = s.ov_dc + s.dcpair_off[f];
        for (int k = 0; k < nc; ++k) {
            for (int ch = 0; ch < chunks; ++ch) {
                const int j = (ch << 6) + lane;
                if (j < nd && !((assigned >> ch) & 1ull) && idet[j] == 0 && !(det[(size_t)j * KC + C_SCORE] < thresh) &&
                    dcov[(long long)k * nd + j] > min_ov) {
                    assigned |= 1ull << ch;
                    --fp_l;
                }
            }
        }
    }
    const int fp = wave_sum(fp_l);
    if (lane == 0) {
        m.tp[out] = tp;
        m.fp[out] = fp;
        m.fn[out] = fn;
        m.similarity[out] = metric != 0 ? 0.0 : (tp + fp == 0 ? -1.0 : sim);
    }
}

int check_split(const srcnn_kitti_split *s)
{
    SRCNN_REQUIRE(s != nullptr, "null split");
    SRCNN_REQUIRE(s->n_frames >= 0, "n_frames < 0");
    SRCNN_REQUIRE(s->max_det_per_frame >= 0, "max_det_per_frame < 0");
    if (s->max_det_per_frame > SRCNN_KITTI_MAX_DET) {
        set_error("srcnn_kitti: a frame holds %d detections, more than the limit of %d (SRCNN_KITTI_MAX_DET)",
                  s->max_det_per_frame, SRCNN_KITTI_MAX_DET);
        return SRCNN_ERR_ARG;
    }
    if (s->n_frames > 0) {
        SRCNN_REQUIRE(s->det_off && s->gt_off && s->dc_off && s->pair_off && s->dcpair_off, "null offsets");
        SRCNN_REQUIRE(s->ov_img && s->ov_bev && s->ov_3d && s->ov_dc, "null overlap matrices");
    }
    return SRCNN_OK;
}

}  // namespace

}  // namespace srcnn

extern "C" {

int srcnn_kitti_overlaps(const srcnn_kitti_split *split, srcnn_stream_t stream)
{
    int rc = srcnn::check_split(split);
    if (rc) return rc;
    if (split->n_frames == 0) return SRCNN_OK;
    SRCNN_LAUNCH(srcnn::kitti_overlaps_kernel, dim3(split->n_frames), dim3(256), 0, srcnn::as_stream(stream), *split);
    return srcnn::check_launch("srcnn_kitti_overlaps");
}

int srcnn_kitti_match(const srcnn_kitti_split *split, const srcnn_kitti_match_desc *match, srcnn_stream_t stream)
{
    int rc = srcnn::check_split(split);
    if (rc) return rc;
    SRCNN_REQUIRE(match != nullptr, "null match descriptor");
    const srcnn_kitti_match_desc &m = *match;
    SRCNN_REQUIRE(m.compute_fp == 0 || m.compute_fp == 1, "compute_fp must be 0 or 1");
    SRCNN_REQUIRE(m.n_cfg >= 0, "n_cfg < 0");
    SRCNN_REQUIRE(m.compute_fp ? (m.n_slots >= 1 && m.n_slots <= SRCNN_KITTI_SLOTS) : m.n_slots == 1,
                  "n_slots must be 1 for pass 1 and 1..SRCNN_KITTI_SLOTS for pass 2");
    SRCNN_REQUIRE(m.n_gt_total >= 0 && m.n_det_total >= 0, "negative row totals");
    const long long n_items = (long long)m.n_cfg * m.n_slots * split->n_frames;
    if (n_items == 0) return SRCNN_OK;
    SRCNN_REQUIRE(m.cfg_flags && m.cfg_metric && m.cfg_min_overlap && m.ign_gt && m.ign_det, "null configuration arrays");
    SRCNN_REQUIRE(m.compute_fp ? (m.cfg_n_thresh && m.thresholds && m.tp && m.fp && m.fn && m.similarity) : m.gt_score != nullptr,
                  "null pass arrays");
    const long long blocks = (n_items + srcnn::WAVES - 1) / srcnn::WAVES;
    SRCNN_REQUIRE(blocks <= INT_MAX, "too many (configuration, slot, frame) items for one launch");
    SRCNN_LAUNCH(srcnn::kitti_match_kernel, dim3((unsigned)blocks), dim3(64 * srcnn::WAVES), 0, srcnn::as_stream(stream),
                 *split, m, n_items);
    return srcnn::check_launch("srcnn_kitti_match");
}

}  // extern "C"
