// Training target layers for gfx950: the anchor target layer and the proposal target layer of Stereo R-CNN.
//
// Reference: lib/model/rpn/anchor_target_layer.py:64-154, lib/model/rpn/proposal_target_layer.py:36-333,
// lib/model/rpn/bbox_transform.py:38-77 (bbox_transform_batch), :220-309 (bbox_overlaps_batch).  The contract -- what is
// bit-equal, how the caller's random draws are used, which quirks of the reference are kept -- is in include/srcnn_hip.h
// ("training target layers").
//
// Anchor layer, four launches behind one memset, nothing read back:
//   1. anchor_gtmax_kernel   per ground-truth box, the maximum overlap over the inside anchors (:86).  A maximum is the only
//                            floating reduction: integer atomicMax on the order-preserving bit pattern, LDS then global.
//   2. anchor_label_kernel   one anchor per thread, the ground truth of its image in LDS: overlaps again (same code, same
//                            bits), max / first argmax, labels (:88-100), both target sets (:133-134), zeroed weights, and the
//                            per-image foreground / background counts (integer atomics).
//   3. anchor_select_kernel  one workgroup per (image, class): radix select (4 x 8 bits, LDS histogram) of the quota-th
//                            smallest key, then one pass in index order that keeps keys below it and the first ties,
//                            disables the rest and writes the weights of what is kept.
// The passes of 3 run on one CU per (image, class); the anchor layer is latency-bound and this keeps every cross-workgroup
// dependency at a kernel boundary.
// Proposal layer: one launch, one workgroup per image (R + K is about 2000 + 30), everything in LDS.
#include "common.h"

namespace srcnn {

constexpr int TG_THREADS = 256;      // anchor kernels 1 and 2
constexpr int TG_WG = 1024;          // one-workgroup kernels
constexpr int TG_MAXK = SRCNN_TARGETS_MAX_GT;

// ---------------------------------------------------------------------------------------------- shared arithmetic
struct GtBoxes {            // the ground truth of one image in LDS, with what bbox_overlaps_batch derives from it (:239-247)
    float x1[TG_MAXK], y1[TG_MAXK], x2[TG_MAXK], y2[TG_MAXK], area[TG_MAXK];
    int zero[TG_MAXK];
};

__device__ __forceinline__ void load_gt(GtBoxes &g, const float *__restrict__ gt /* (K, 5) of this image */, int K, int tid)
{
    if (tid < K) {
        const float x1 = gt[tid * 5 + 0], y1 = gt[tid * 5 + 1], x2 = gt[tid * 5 + 2], y2 = gt[tid * 5 + 3];
        const float gx = (x2 - x1) + 1.0f, gy = (y2 - y1) + 1.0f;
        g.x1[tid] = x1, g.y1[tid] = y1, g.x2[tid] = x2, g.y2[tid] = y2;
        g.area[tid] = gx * gy;
        g.zero[tid] = (gx == 1.0f) & (gy == 1.0f);
    }
}

struct Box {
    float x1, y1, x2, y2, area;
    int zero;
};

__device__ __forceinline__ Box make_box(float x1, float y1, float x2, float y2)
{
    Box b;
    b.x1 = x1, b.y1 = y1, b.x2 = x2, b.y2 = y2;
    const float bx = (x2 - x1) + 1.0f, by = (y2 - y1) + 1.0f;
    b.area = bx * by;
    b.zero = (bx == 1.0f) & (by == 1.0f);
    return b;
}

// bbox_transform.py:253-265, one rounding per operation (the library is built with -ffp-contract=off; float division is
// correctly rounded)
__device__ __forceinline__ float overlap(const Box &a, const GtBoxes &g, int k)
{
    float iw = (fminf(a.x2, g.x2[k]) - fmaxf(a.x1, g.x1[k])) + 1.0f;
    if (iw < 0.0f) iw = 0.0f;
    float ih = (fminf(a.y2, g.y2[k]) - fmaxf(a.y1, g.y1[k])) + 1.0f;
    if (ih < 0.0f) ih = 0.0f;
    const float inter = iw * ih;
    const float ua = (a.area + g.area[k]) - inter;
    float ov = inter / ua;
    if (g.zero[k]) ov = 0.0f;
    if (a.zero) ov = -1.0f;
    return ov;
}

// torch.max(overlaps, 2): the maximum and its FIRST index
__device__ __forceinline__ void max_overlap(const Box &a, const GtBoxes &g, int K, float &best, int &arg)
{
    best = overlap(a, g, 0), arg = 0;
    for (int k = 1; k < K; ++k) {
        const float ov = overlap(a, g, k);
        if (ov > best) best = ov, arg = k;
    }
}

// bbox_transform_batch (bbox_transform.py:41-54 / :57-70): ex = anchor / roi, gt = its ground-truth box
__device__ __forceinline__ void box_targets(float ex1, float ey1, float ex2, float ey2, const float *__restrict__ gt, float *t)
{
    const float ex_w = (ex2 - ex1) + 1.0f, ex_h = (ey2 - ey1) + 1.0f;
    const float ex_cx = ex1 + 0.5f * ex_w, ex_cy = ey1 + 0.5f * ex_h;
    const float gt_w = (gt[2] - gt[0]) + 1.0f, gt_h = (gt[3] - gt[1]) + 1.0f;
    const float gt_cx = gt[0] + 0.5f * gt_w, gt_cy = gt[1] + 0.5f * gt_h;
    t[0] = (gt_cx - ex_cx) / ex_w;
    t[1] = (gt_cy - ex_cy) / ex_h;
    t[2] = logf(gt_w / ex_w);
    t[3] = logf(gt_h / ex_h);
}

// order-preserving float -> unsigned (0 is below every float): lets an integer atomicMax take a float maximum
__device__ __forceinline__ unsigned float_order(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_unorder(unsigned e)
{
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

// torch 0.3's round: half away from zero (x - trunc(x) is exact)
__device__ __forceinline__ float round_half_away(float x)
{
    const float t = truncf(x);
    return fabsf(x - t) >= 0.5f ? t + copysignf(1.0f, x) : t;
}

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------- anchor layer
// anchor_target_layer.py:68-71 with allowed_border 0; im_info row 0 serves every image
__device__ __forceinline__ bool anchor_inside(const float4 a, const float *__restrict__ im_info)
{
    const float w = (float)(long long)im_info[1], h = (float)(long long)im_info[0];
    return a.x >= 0.0f && a.y >= 0.0f && a.z < w && a.w < h;
}

__global__ __launch_bounds__(TG_THREADS) void anchor_gtmax_kernel(const float4 *__restrict__ anchors, int N,
                                                                  const float *__restrict__ gt_merge, int K,
                                                                  const float *__restrict__ im_info, unsigned *__restrict__ gt_max)
{
    __shared__ GtBoxes g;
    __shared__ unsigned smax[TG_MAXK];
    const int b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * TG_THREADS + tid;
    load_gt(g, gt_merge + (size_t)b * K * 5, K, tid);
    if (tid < TG_MAXK) smax[tid] = 0u;
    __syncthreads();
    if (i < N) {
        const float4 a = anchors[i];
        if (anchor_inside(a, im_info)) {
            const Box box = make_box(a.x, a.y, a.z, a.w);
            for (int k = 0; k < K; ++k) {
                const unsigned e = float_order(overlap(box, g, k));
                if (e > smax[k]) atomicMax(&smax[k], e);      // the plain read only filters: the word never decreases
            }
        }
    }
    __syncthreads();
    if (tid < K && smax[tid] != 0u) atomicMax(&gt_max[b * K + tid], smax[tid]);
}

__global__ __launch_bounds__(TG_THREADS) void anchor_label_kernel(const float4 *__restrict__ anchors, int N,
                                                                  const float *__restrict__ gt_left, const float *__restrict__ gt_right,
                                                                  const float *__restrict__ gt_merge, int K,
                                                                  const float *__restrict__ im_info, const unsigned *__restrict__ gt_max,
                                                                  srcnn_anchor_target_params p, int *__restrict__ labels,
                                                                  float4 *__restrict__ targets_left, float4 *__restrict__ targets_right,
                                                                  float *__restrict__ inside_w, float *__restrict__ outside_w,
                                                                  float *__restrict__ max_overlaps, int *__restrict__ counts)
{
    __shared__ GtBoxes g;
    __shared__ float gmax[TG_MAXK];
    const int b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * TG_THREADS + tid;
    load_gt(g, gt_merge + (size_t)b * K * 5, K, tid);
    if (tid < K) {
        const unsigned e = gt_max[b * K + tid];
        float m = e ? float_unorder(e) : -3.0f;            // no inside anchor at all: nothing can equal it
        if (m == 0.0f) m = 1e-5f;                          // :90
        gmax[tid] = m;
    }
    __syncthreads();
    int label = -1;
    if (i < N) {
        const float4 a = anchors[i];
        const size_t o = (size_t)b * N + i;
        float4 tl = make_float4(0.f, 0.f, 0.f, 0.f), tr = tl;
        float best = -2.0f;
        if (anchor_inside(a, im_info)) {
            const Box box = make_box(a.x, a.y, a.z, a.w);
            int arg = 0, keep = 0;
            best = overlap(box, g, 0);
            keep = best == gmax[0];
            for (int k = 1; k < K; ++k) {
                const float ov = overlap(box, g, k);
                keep |= ov == gmax[k];                      // :91
                if (ov > best) best = ov, arg = k;
            }
            if (!p.clobber_positives && best < p.negative_overlap) label = 0;      // :88
            if (keep) label = 1;                                                      // :94
            if (best >= p.positive_overlap) label = 1;                                // :97
            if (p.clobber_positives && best < p.negative_overlap) label = 0;         // :100
            float t[4];
            box_targets(a.x, a.y, a.z, a.w, gt_left + ((size_t)b * K + arg) * 5, t);  // :133, the MERGED argmax
            tl = make_float4(t[0], t[1], t[2], t[3]);
            box_targets(a.x, a.y, a.z, a.w, gt_right + ((size_t)b * K + arg) * 5, t); // :134
            tr = make_float4(t[0], t[1], t[2], t[3]);
        }
        labels[o] = label;
        targets_left[o] = tl;
        targets_right[o] = tr;
        inside_w[o] = 0.0f;
        outside_w[o] = 0.0f;
        if (max_overlaps) max_overlaps[o] = best;
    }
    const int nfg = __syncthreads_count(label == 1);       // :104-105
    const int nbg = __syncthreads_count(label == 0);
    if (tid == 0) {
        if (nfg) atomicAdd(&counts[2 * b], nfg);
        if (nbg) atomicAdd(&counts[2 * b + 1], nbg);
    }
}

// what the reference keeps of an image with these pre-subsample counts (:109-128)
__device__ __forceinline__ int kept_examples(int sum_fg, int sum_bg, const srcnn_anchor_target_params &p)
{
    const int fg = sum_fg > p.num_fg ? p.num_fg : sum_fg;
    const int num_bg = p.batch_size - sum_fg;
    const int bg = sum_bg > num_bg ? (num_bg > 0 ? num_bg : 0) : sum_bg;
    return fg + bg;
}

__global__ __launch_bounds__(TG_WG) void anchor_select_kernel(int N, int B, const unsigned *__restrict__ fg_keys,
                                                              const unsigned *__restrict__ bg_keys, const int *__restrict__ counts,
                                                              srcnn_anchor_target_params p, int *__restrict__ labels,
                                                              float *__restrict__ inside_w, float *__restrict__ outside_w)
{
    __shared__ int hist[256];
    __shared__ int wsum[TG_WG / 64];
    __shared__ int s_digit, s_remaining;
    const int cls = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int want = cls == 0 ? 1 : 0;
    const unsigned *keys = (cls == 0 ? fg_keys : bg_keys) + (size_t)b * N;
    int *lab = labels + (size_t)b * N;
    const int sum_fg = counts[2 * b], sum_bg = counts[2 * b + 1];
    const int count = cls == 0 ? sum_fg : sum_bg;
    int quota = cls == 0 ? p.num_fg : p.batch_size - sum_fg;       // :119: sum_fg as counted BEFORE the foreground subsample
    const bool subsample = count > quota;                          // :109 / :122
    if (quota < 0) quota = 0;                                      // a slice past the end disables every candidate
    // :140: `i` is the batch loop's leftover -- the LAST image's kept examples weigh every image
    const float outside = 1.0f / (float)kept_examples(counts[2 * (B - 1)], counts[2 * (B - 1) + 1], p);

    unsigned T = 0u;        // the quota-th smallest key
    int need = 0;           // how many candidates with key == T are kept (the lowest indices)
    if (subsample && quota > 0) {
        unsigned prefix = 0u;
        int remaining = quota;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < N; i += TG_WG) {
                if (lab[i] != want) continue;
                const unsigned k = keys[i];
                if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int cum = 0, d = 0;
                while (d < 255 && cum + hist[d] < remaining) cum += hist[d], ++d;
                s_digit = d, s_remaining = remaining - cum;
            }
            __syncthreads();
            prefix = (prefix << 8) | (unsigned)s_digit;
            remaining = s_remaining;
            __syncthreads();
        }
        T = prefix, need = remaining;
    }
    // one pass in index order: `run` = ties met so far
    int run = 0;
    for (int base = 0; base < N; base += TG_WG) {
        const int i = base + tid;
        const bool cand = i < N && lab[i] == want;
        const unsigned k = cand ? keys[i] : 0u;
        const bool tie = cand && subsample && k == T;
        const unsigned long long m = __ballot(tie);
        const int rank_in_wave = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < TG_WG / 64; ++w) {
            const int c = wsum[w];
            if (w < wv) before += c;
            total += c;
        }
        if (cand) {
            const bool keep = !subsample || k < T || (tie && run + before + rank_in_wave < need);
            if (keep) {
                outside_w[(size_t)b * N + i] = outside;                        // :147-148
                if (cls == 0) inside_w[(size_t)b * N + i] = p.inside_weight;   // :137
            } else {
                lab[i] = -1;                                                   // :117 / :128
            }
        }
        run += total;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- proposal layer
struct ProposalArgs {
    const float *rois_left, *rois_right, *gt_left, *gt_right, *gt_dim_orien, *gt_kpts;
    const unsigned *fg_keys;
    const double *u;
    float *out_rois_left, *out_rois_right, *bbox_targets_left, *bbox_targets_right, *dim_orien_targets, *kpts_weight, *inside_w,
        *outside_w;
    int *labels, *kpts_targets, *status, *keep_inds;
    int R, K, Mpad;
    srcnn_proposal_target_params p;
};

// roi i of image b: a proposal, or (i >= R) the appended ground-truth box i - R (:45-53)
__device__ __forceinline__ const float *roi_box(const float *__restrict__ rois, const float *__restrict__ gt, int b, int i, int R, int K)
{
    return i < R ? rois + ((size_t)b * R + i) * 5 + 1 : gt + ((size_t)b * K + (i - R)) * 5;
}

__device__ __forceinline__ int draw_with_replacement(double u, int count)
{
    int pos = (int)floor(u * (double)count);       // np.floor(np.random.rand(..) * count), in double
    return pos < 0 ? 0 : (pos >= count ? count - 1 : pos);
}

__global__ __launch_bounds__(TG_WG) void proposal_targets_kernel(ProposalArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ GtBoxes gl, gr;
    __shared__ int wsum_fg[TG_WG / 64], wsum_bg[TG_WG / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int R = a.R, K = a.K, M = R + K, S = a.p.rois_per_image;
    int *packed = reinterpret_cast<int *>(smem);                                   // (M) argl | argr << 8 | fg << 16 | bg << 17
    unsigned *fg_key = reinterpret_cast<unsigned *>(packed + a.Mpad);              // (fg_num) keys of the foreground candidates
    int *sel = reinterpret_cast<int *>(fg_key + a.Mpad);                           // (S) the selected roi of every output row
    unsigned short *fg_list = reinterpret_cast<unsigned short *>(sel + SRCNN_TARGETS_MAX_BATCH_ROIS);     // ascending index order
    unsigned short *bg_list = fg_list + a.Mpad;

    load_gt(gl, a.gt_left + (size_t)b * K * 5, K, tid);
    load_gt(gr, a.gt_right + (size_t)b * K * 5, K, tid);
    __syncthreads();
    for (int i = tid; i < M; i += TG_WG) {                                         // :201-205, :233-242
        const float *bl = roi_box(a.rois_left, a.gt_left, b, i, R, K), *br = roi_box(a.rois_right, a.gt_right, b, i, R, K);
        float ml, mr;
        int al, ar;
        max_overlap(make_box(bl[0], bl[1], bl[2], bl[3]), gl, K, ml, al);
        max_overlap(make_box(br[0], br[1], br[2], br[3]), gr, K, mr, ar);
        const int fg = ml >= a.p.fg_thresh && mr >= a.p.fg_thresh && al == ar;
        const int bg = (ml < a.p.bg_thresh_hi && ml >= a.p.bg_thresh_lo) || (mr < a.p.bg_thresh_hi && mr >= a.p.bg_thresh_lo);
        packed[i] = al | (ar << 8) | (fg << 16) | (bg << 17);
    }
    __syncthreads();
    // stable compaction of both candidate sets: thread t owns rois [t * per, (t + 1) * per)
    const int per = (M + TG_WG - 1) / TG_WG;
    const int lo = tid * per < M ? tid * per : M, hi = lo + per < M ? lo + per : M;
    int cf = 0, cb = 0;
    for (int i = lo; i < hi; ++i) cf += (packed[i] >> 16) & 1, cb += (packed[i] >> 17) & 1;
    const int sf = wave_inclusive_scan(cf, lane), sb = wave_inclusive_scan(cb, lane);
    if (lane == 63) wsum_fg[wv] = sf, wsum_bg[wv] = sb;
    __syncthreads();
    int of = sf - cf, ob = sb - cb, fg_num = 0, bg_num = 0;
    for (int w = 0; w < TG_WG / 64; ++w) {
        if (w < wv) of += wsum_fg[w], ob += wsum_bg[w];
        fg_num += wsum_fg[w], bg_num += wsum_bg[w];
    }
    for (int i = lo; i < hi; ++i) {
        if ((packed[i] >> 16) & 1) fg_key[of] = a.fg_keys[(size_t)b * M + i], fg_list[of++] = (unsigned short)i;
        if ((packed[i] >> 17) & 1) bg_list[ob++] = (unsigned short)i;
    }
    __syncthreads();
    // the four branches of :246-285
    const double *u = a.u + (size_t)b * S;
    int fg_rows = 0;
    const bool none = fg_num == 0 && bg_num == 0;
    if (fg_num > 0 && bg_num > 0) {
        fg_rows = a.p.fg_rois_per_image < fg_num ? a.p.fg_rois_per_image : fg_num;
        for (int c = tid; c < fg_num; c += TG_WG) {            // rank by (key, index): the list is in index order
            const unsigned k = fg_key[c];
            int rank = 0;
            for (int d = 0; d < fg_num; ++d) rank += fg_key[d] < k || (fg_key[d] == k && d < c);
            if (rank < fg_rows) sel[rank] = fg_list[c];
        }
        for (int r = fg_rows + tid; r < S; r += TG_WG) sel[r] = bg_list[draw_with_replacement(u[r], bg_num)];
    } else if (fg_num > 0) {
        fg_rows = S;
        for (int r = tid; r < S; r += TG_WG) sel[r] = fg_list[draw_with_replacement(u[r], fg_num)];
    } else if (bg_num > 0) {
        for (int r = tid; r < S; r += TG_WG) sel[r] = bg_list[draw_with_replacement(u[r], bg_num)];
    }
    if (tid == 0) a.status[b] = none ? 1 : 0;
    __syncthreads();
    for (int r = tid; r < S; r += TG_WG) {
        const size_t o = (size_t)b * S + r;
        float rl[5] = {0, 0, 0, 0, 0}, rr[5] = {0, 0, 0, 0, 0}, tl[4] = {0, 0, 0, 0}, tr[4] = {0, 0, 0, 0}, dim[5] = {0, 0, 0, 0, 0};
        float kw[3] = {0, 0, 0}, inw[4] = {0, 0, 0, 0};
        int kt[3] = {0, 0, 0}, label = 0, idx = 0;
        if (!none) {
            idx = sel[r];
            const int al = packed[idx] & 255, ar = (packed[idx] >> 8) & 255;
            const float *bl = roi_box(a.rois_left, a.gt_left, b, idx, R, K), *br = roi_box(a.rois_right, a.gt_right, b, idx, R, K);
            const float *gtl = a.gt_left + ((size_t)b * K + al) * 5, *gtr = a.gt_right + ((size_t)b * K + ar) * 5;
            const float cls = r < fg_rows ? gtl[4] : 0.0f;                         // :291-294
            label = (int)cls;
            rl[0] = rr[0] = (float)b;                                              // :297 / :300
            for (int j = 0; j < 4; ++j) rl[1 + j] = bl[j], rr[1 + j] = br[j];
            if (cls > 0.0f) {                                                      // :96 / :115
                box_targets(bl[0], bl[1], bl[2], bl[3], gtl, tl);
                box_targets(br[0], br[1], br[2], br[3], gtr, tr);
                for (int j = 0; j < 4; ++j) {                                      // :152-153
                    tl[j] = (tl[j] - a.p.bbox_means[j]) / a.p.bbox_stds[j];
                    tr[j] = (tr[j] - a.p.bbox_means[j]) / a.p.bbox_stds[j];
                    inw[j] = a.p.inside_weights[j];
                }
                const float *gd = a.gt_dim_orien + ((size_t)b * K + al) * 5;       // :309, the LEFT assignment
                for (int j = 0; j < 5; ++j) dim[j] = (gd[j] - a.p.dim_means[j]) / a.p.dim_stds[j];      // :163-164
            }
            if (cls == 1.0f) {                                                     // :133
                const float *gk = a.gt_kpts + ((size_t)b * K + al) * 6;            // :310
                const float grid = (float)a.p.kpts_grid, width = (bl[2] - bl[0]) + 1.0f;
                float t[6];
                for (int j = 0; j < 6; ++j) {                                      // :179-181
                    t[j] = round_half_away(((gk[j] - bl[0]) * grid) / width);
                    if (t[j] < 0.0f) t[j] = -225.0f;
                    if (t[j] > grid - 1.0f) t[j] = -225.0f;
                }
                float pos = t[0];
                int type = 0;
                for (int j = 1; j < 4; ++j)
                    if (t[j] > pos) pos = t[j], type = j;                          // :182, the first maximum
                const float v[3] = {(float)type * grid + pos, t[4], t[5]};         // :185
                for (int j = 0; j < 3; ++j) {
                    kw[j] = v[j] < 0.0f ? 0.0f : 1.0f;                             // :187-190
                    kt[j] = v[j] < 0.0f ? 0 : (int)v[j];
                }
            }
        }
        a.labels[o] = label;
        if (a.keep_inds) a.keep_inds[o] = idx;
        for (int j = 0; j < 5; ++j) a.out_rois_left[o * 5 + j] = rl[j], a.out_rois_right[o * 5 + j] = rr[j], a.dim_orien_targets[o * 5 + j] = dim[j];
        for (int j = 0; j < 4; ++j) {
            a.bbox_targets_left[o * 4 + j] = tl[j], a.bbox_targets_right[o * 4 + j] = tr[j];
            a.inside_w[o * 4 + j] = inw[j], a.outside_w[o * 4 + j] = inw[j] > 0.0f ? 1.0f : 0.0f;      // :64
        }
        for (int j = 0; j < 3; ++j) a.kpts_targets[o * 3 + j] = kt[j], a.kpts_weight[o * 3 + j] = kw[j];
    }
}

static size_t proposal_lds_bytes(int Mpad)
{
    return (size_t)Mpad * 4 * 2 + (size_t)SRCNN_TARGETS_MAX_BATCH_ROIS * 4 + (size_t)Mpad * 2 * 2;
}

}  // namespace srcnn

extern "C" {

size_t srcnn_anchor_targets_workspace_bytes(int B, int K)
{
    using namespace srcnn;
    if (B < 1 || K < 1 || K > SRCNN_TARGETS_MAX_GT) return 0;
    // ONE zeroed block: [gt_max (B, K) ordered bit patterns | counts (B, 2)]
    return align_up(((size_t)B * K + (size_t)B * 2) * sizeof(int), 256);
}

int srcnn_anchor_targets(const float *anchors, int N, const float *gt_left, const float *gt_right, const float *gt_merge, int B, int K,
                         const float *im_info, const unsigned *fg_keys, const unsigned *bg_keys,
                         const srcnn_anchor_target_params *params, int *labels, float *targets_left, float *targets_right,
                         float *inside_w, float *outside_w, float *max_overlaps, void *workspace, size_t workspace_bytes,
                         srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(params, "null params");
    SRCNN_REQUIRE(anchors && gt_left && gt_right && gt_merge && im_info && fg_keys && bg_keys, "null input pointer");
    SRCNN_REQUIRE(labels && targets_left && targets_right && inside_w && outside_w, "null output pointer");
    SRCNN_REQUIRE(B >= 1 && N >= 1, "negative or zero sizes: B and N must be >= 1");
    SRCNN_REQUIRE(K >= 1 && K <= SRCNN_TARGETS_MAX_GT, "K must be 1..64 (SRCNN_TARGETS_MAX_GT)");
    SRCNN_REQUIRE((long long)B * N < (1LL << 31), "B * N must stay below 2^31");
    SRCNN_REQUIRE(params->batch_size >= 0, "batch_size must be >= 0");
    SRCNN_REQUIRE(params->num_fg >= 0 && params->num_fg <= params->batch_size, "quota num_fg must be 0..batch_size");
    SRCNN_REQUIRE((reinterpret_cast<uintptr_t>(anchors) & 15) == 0 && (reinterpret_cast<uintptr_t>(targets_left) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(targets_right) & 15) == 0,
                  "anchors / targets must be 16-byte aligned");
    if (!workspace || workspace_bytes < srcnn_anchor_targets_workspace_bytes(B, K)) {
        set_error("srcnn_anchor_targets: workspace too small (srcnn_anchor_targets_workspace_bytes)");
        return SRCNN_ERR_WORKSPACE;
    }
    unsigned *gt_max = static_cast<unsigned *>(workspace);
    int *counts = reinterpret_cast<int *>(gt_max + (size_t)B * K);
    hipStream_t st = as_stream(stream);
    SRCNN_HIP_TRY(memset_async(workspace, 0, srcnn_anchor_targets_workspace_bytes(B, K), st));
    const dim3 grid(cdiv(N, TG_THREADS), B);
    const float4 *a4 = reinterpret_cast<const float4 *>(anchors);
    SRCNN_LAUNCH(anchor_gtmax_kernel, grid, TG_THREADS, 0, st, a4, N, gt_merge, K, im_info, gt_max);
    SRCNN_LAUNCH(anchor_label_kernel, grid, TG_THREADS, 0, st, a4, N, gt_left, gt_right, gt_merge, K, im_info, (const unsigned *)gt_max,
                 *params, labels, reinterpret_cast<float4 *>(targets_left), reinterpret_cast<float4 *>(targets_right), inside_w,
                 outside_w, max_overlaps, counts);
    SRCNN_LAUNCH(anchor_select_kernel, dim3(2, B), TG_WG, 0, st, N, B, fg_keys, bg_keys, (const int *)counts, *params, labels, inside_w,
                 outside_w);
    return check_launch("srcnn_anchor_targets");
}

size_t srcnn_proposal_targets_workspace_bytes(int B, int R, int K)
{
    if (B < 1 || R < 1 || K < 1 || K > SRCNN_TARGETS_MAX_GT || (long long)R + K > SRCNN_TARGETS_MAX_ROIS) return 0;
    return 256;     // everything lives in LDS; a token block keeps the caller-owned-workspace convention uniform
}

int srcnn_proposal_targets(const float *rois_left, const float *rois_right, int B, int R, const float *gt_left, const float *gt_right,
                           const float *gt_dim_orien, const float *gt_kpts, int K, const unsigned *fg_keys, const double *u,
                           const srcnn_proposal_target_params *params, float *out_rois_left, float *out_rois_right, int *labels,
                           float *bbox_targets_left, float *bbox_targets_right, float *dim_orien_targets, int *kpts_targets,
                           float *kpts_weight, float *inside_w, float *outside_w, int *status, int *keep_inds, void *workspace,
                           size_t workspace_bytes, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(params, "null params");
    SRCNN_REQUIRE(rois_left && rois_right && gt_left && gt_right && gt_dim_orien && gt_kpts && fg_keys && u, "null input pointer");
    SRCNN_REQUIRE(out_rois_left && out_rois_right && labels && bbox_targets_left && bbox_targets_right && dim_orien_targets &&
                      kpts_targets && kpts_weight && inside_w && outside_w && status,
                  "null output pointer");
    SRCNN_REQUIRE(B >= 1 && R >= 1, "negative or zero sizes: B and R must be >= 1");
    SRCNN_REQUIRE(K >= 1 && K <= SRCNN_TARGETS_MAX_GT, "K must be 1..64 (SRCNN_TARGETS_MAX_GT)");
    SRCNN_REQUIRE((long long)R + K <= SRCNN_TARGETS_MAX_ROIS, "R + K must be <= 4096 (SRCNN_TARGETS_MAX_ROIS)");
    SRCNN_REQUIRE(params->rois_per_image >= 1 && params->rois_per_image <= SRCNN_TARGETS_MAX_BATCH_ROIS,
                  "rois_per_image must be 1..1024 (SRCNN_TARGETS_MAX_BATCH_ROIS)");
    SRCNN_REQUIRE(params->fg_rois_per_image >= 0 && params->fg_rois_per_image <= params->rois_per_image,
                  "quota fg_rois_per_image must be 0..rois_per_image");
    SRCNN_REQUIRE(params->kpts_grid >= 1, "kpts_grid must be >= 1");
    for (int j = 0; j < 5; ++j)
        SRCNN_REQUIRE(params->dim_stds[j] != 0.0f && (j == 4 || params->bbox_stds[j] != 0.0f), "a zero std");
    if (!workspace || workspace_bytes < srcnn_proposal_targets_workspace_bytes(B, R, K)) {
        set_error("srcnn_proposal_targets: workspace too small (srcnn_proposal_targets_workspace_bytes)");
        return SRCNN_ERR_WORKSPACE;
    }
    ProposalArgs a;
    a.rois_left = rois_left, a.rois_right = rois_right, a.gt_left = gt_left, a.gt_right = gt_right, a.gt_dim_orien = gt_dim_orien;
    a.gt_kpts = gt_kpts, a.fg_keys = fg_keys, a.u = u;
    a.out_rois_left = out_rois_left, a.out_rois_right = out_rois_right, a.bbox_targets_left = bbox_targets_left;
    a.bbox_targets_right = bbox_targets_right, a.dim_orien_targets = dim_orien_targets, a.kpts_weight = kpts_weight;
    a.inside_w = inside_w, a.outside_w = outside_w, a.labels = labels, a.kpts_targets = kpts_targets, a.status = status;
    a.keep_inds = keep_inds;
    a.R = R, a.K = K, a.Mpad = (int)align_up((size_t)(R + K), 8);
    a.p = *params;
    SRCNN_LAUNCH(proposal_targets_kernel, B, TG_WG, proposal_lds_bytes(a.Mpad), as_stream(stream), a);
    return check_launch("srcnn_proposal_targets");
}

}  // extern "C"
