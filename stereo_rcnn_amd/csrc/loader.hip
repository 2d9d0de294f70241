// The per-iteration half of the training data loader (include/srcnn_hip.h, "training: batch assembly"):
//   srcnn_gt_batch          minibatch.py:47-82 + roibatchLoader.py:72-110 -- scale, clamp, mask, shuffle, truncate and pad the
//                           ground-truth rows of a whole batch from the device-resident table, one workgroup per batch slot;
//   srcnn_preprocess_train  minibatch.py:89-131 + blob.py:20-64 -- decoded uint8 pairs to the two zero-padded float32 blobs,
//                           flip, mean and OpenCV's INTER_LINEAR (resize_tap.h), one launch for the 2B images.
// Every output element is written exactly once (callers pass uninitialised buffers); no atomics, no host read.
#include "common.h"
#include "resize_tap.h"
#include <cmath>

namespace srcnn {

struct GtBatchArgs {
    srcnn_gt_slot slot[SRCNN_LOADER_MAX_BATCH];
};

#define GT_WG 256

// One workgroup per batch slot.  Row c of the slot (table row row_begin + c) goes to output row rank(c) = the number of rows d
// with (key[d], d) < (key[c], c), the convention of targets.hip; rows whose rank is >= K are dropped, output rows >= min(n, K)
// are zeros.  Thread t owns rows t, t + 256, .. and then the zero rows t, t + 256, .. of the tail.
__global__ __launch_bounds__(GT_WG) void gt_batch_kernel(const float *__restrict__ table, GtBatchArgs a,
                                                         const unsigned *__restrict__ keys, int key_stride, int K,
                                                         float *__restrict__ gt_left, float *__restrict__ gt_right,
                                                         float *__restrict__ gt_merge, float *__restrict__ gt_dim_orien,
                                                         float *__restrict__ gt_kpts, long long *__restrict__ num_boxes)
{
    __shared__ unsigned key_lds[SRCNN_GT_MAX_ROWS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const srcnn_gt_slot s = a.slot[b];
    const int n = s.n, kept = min(n, K);
    for (int c = tid; c < n; c += GT_WG) key_lds[c] = keys[(size_t)b * key_stride + c];
    __syncthreads();
    float *boxes[3] = {gt_left + (size_t)b * K * 5, gt_right + (size_t)b * K * 5, gt_merge + (size_t)b * K * 5};
    float *dim_o = gt_dim_orien + (size_t)b * K * 5, *kp_o = gt_kpts + (size_t)b * K * 6;
    for (int c = tid; c < n; c += GT_WG) {
        const unsigned k = key_lds[c];
        int rank = 0;
        for (int d = 0; d < n; ++d) {
            const unsigned kd = key_lds[d];
            rank += (kd < k || (kd == k && d < c)) ? 1 : 0;
        }
        if (rank >= kept) continue;
        const float *row = table + (size_t)(s.row_begin + c) * SRCNN_GT_COLS;
        const float cls = row[23];
#pragma unroll
        for (int g = 0; g < 3; ++g) {                      // left, right, merge boxes: columns 0-3, 4-7, 8-11
            float *o = boxes[g] + (size_t)rank * 5;
            o[0] = fminf(row[4 * g] * s.im_scale, s.im_width);     // minibatch.py:49-50: x1 = min(x1, im_width)
            o[1] = row[4 * g + 1] * s.im_scale;
            o[2] = row[4 * g + 2] * s.im_scale;
            o[3] = row[4 * g + 3] * s.im_scale;
            o[4] = cls;
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) dim_o[(size_t)rank * 5 + j] = row[12 + j];     // w, h, l, sin, cos: unscaled
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const float v = row[17 + j] * s.im_scale;
            kp_o[(size_t)rank * 6 + j] = (v < 0.f || v > s.im_width - 1.f) ? -1.f : v;     // :75-76
        }
    }
    for (int r = kept + tid; r < K; r += GT_WG) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            boxes[0][(size_t)r * 5 + j] = 0.f;
            boxes[1][(size_t)r * 5 + j] = 0.f;
            boxes[2][(size_t)r * 5 + j] = 0.f;
            dim_o[(size_t)r * 5 + j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) kp_o[(size_t)r * 6 + j] = 0.f;
    }
    if (tid == 0) num_boxes[b] = kept;
}

struct TrainImage {
    const unsigned char *left, *right;
    double step;          // 1 / scale: cv::resize's sampling step
    int H, W, OH, OWc;    // source size; output rows; output columns after the max_size crop
    int flipped, pad_;
};

struct TrainImageArgs {
    TrainImage slot[SRCNN_LOADER_MAX_BATCH];
};

// value of element (b, c, y, x) of one eye's (B, 3, Hmax, Wmax) blob
__device__ __forceinline__ float train_element(const TrainImageArgs &a, int eye, int b, int c, int y, int x)
{
    const TrainImage &s = a.slot[b];
    if (x >= s.OWc || y >= s.OH) return 0.f;              // blob.py:27-35: zero padding to the batch maximum
    // flipped (minibatch.py:116-119): the left output is the RIGHT source mirrored and the other way round
    const bool from_left = (eye == 0) != (s.flipped != 0);
    const unsigned char *img = from_left ? s.left : s.right;
    const ResizeTap tx = resize_tap(x, s.W, s.step, true), ty = resize_tap(y, s.H, s.step, false);
    return preprocess_channel(img, s.W, tx, ty, c, s.flipped != 0);
}

// grid (.., 2): blockIdx.y is the eye.  A thread owns four consecutive floats of the flat blob (one 16-byte store, consecutive
// lanes consecutive addresses, whatever Wmax is: rows of an odd width are not 16-byte aligned, the blob is); the last group of
// a blob whose size is no multiple of four is stored element by element.  The blob has fewer than 2^31 elements (checked by
// the entry point): the flat index is split by 32-bit divisions once per group and walked with carries.
__global__ __launch_bounds__(256) void preprocess_train_kernel(TrainImageArgs a, int B, int Hmax, int Wmax,
                                                               float *__restrict__ out_left, float *__restrict__ out_right)
{
    const int eye = blockIdx.y;
    float *out = eye == 0 ? out_left : out_right;
    const unsigned total = (unsigned)B * 3u * (unsigned)Hmax * (unsigned)Wmax, groups = (total + 3u) / 4u;
    for (unsigned g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        const unsigned e0 = g * 4u;
        int x = (int)(e0 % (unsigned)Wmax);
        unsigned t = e0 / (unsigned)Wmax;
        int y = (int)(t % (unsigned)Hmax);
        t /= (unsigned)Hmax;
        int c = (int)(t % 3u), b = (int)(t / 3u);
        float v[4];
        const int count = (int)min(4u, total - e0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = k < count ? train_element(a, eye, b, c, y, x) : 0.f;
            if (++x == Wmax) {
                x = 0;
                if (++y == Hmax) {
                    y = 0;
                    if (++c == 3) { c = 0; ++b; }
                }
            }
        }
        if (count == 4) {
            *reinterpret_cast<float4 *>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int k = 0; k < count; ++k) out[e0 + k] = v[k];
        }
    }
}

}  // namespace srcnn

extern "C" {

int srcnn_gt_batch(const float *table, int table_rows, const srcnn_gt_slot *slots_host, int B, const unsigned *keys,
                   int key_stride, int K, float *gt_left, float *gt_right, float *gt_merge, float *gt_dim_orien, float *gt_kpts,
                   long long *num_boxes, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(slots_host, "null slots");
    SRCNN_REQUIRE(B > 0 && B <= SRCNN_LOADER_MAX_BATCH, "B must be 1..SRCNN_LOADER_MAX_BATCH");
    SRCNN_REQUIRE(K > 0, "K must be positive");
    SRCNN_REQUIRE(table_rows >= 0 && key_stride >= 0, "negative table_rows / key_stride");
    SRCNN_REQUIRE(gt_left && gt_right && gt_merge && gt_dim_orien && gt_kpts && num_boxes, "null output pointer");
    GtBatchArgs a;
    bool any = false;
    for (int b = 0; b < B; ++b) {
        const srcnn_gt_slot &s = slots_host[b];
        SRCNN_REQUIRE(s.n >= 0 && s.row_begin >= 0, "negative row range");
        SRCNN_REQUIRE(s.n <= SRCNN_GT_MAX_ROWS, "more than SRCNN_GT_MAX_ROWS rows in one entry");
        SRCNN_REQUIRE((long long)s.row_begin + s.n <= (long long)table_rows, "row range beyond the table");
        SRCNN_REQUIRE(s.n <= key_stride, "fewer keys than rows (key_stride)");
        SRCNN_REQUIRE(std::isfinite(s.im_scale) && s.im_scale > 0.f && std::isfinite(s.im_width), "bad im_scale / im_width");
        any = any || s.n > 0;
        a.slot[b] = s;
    }
    for (int b = B; b < SRCNN_LOADER_MAX_BATCH; ++b) a.slot[b] = srcnn_gt_slot{0, 0, 1.f, 0.f};
    SRCNN_REQUIRE(!any || (table && keys), "null table / keys");
    SRCNN_LAUNCH(gt_batch_kernel, dim3(B), dim3(GT_WG), 0, as_stream(stream), table, a, keys, key_stride, K, gt_left, gt_right,
                 gt_merge, gt_dim_orien, gt_kpts, num_boxes);
    return check_launch("srcnn_gt_batch");
}

int srcnn_preprocess_train(const srcnn_train_image *slots_host, int B, int Hmax, int Wmax, int max_size, float *out_left,
                           float *out_right, srcnn_stream_t stream)
{
    using namespace srcnn;
    SRCNN_REQUIRE(slots_host, "null slots");
    SRCNN_REQUIRE(B > 0 && B <= SRCNN_LOADER_MAX_BATCH, "B must be 1..SRCNN_LOADER_MAX_BATCH");
    SRCNN_REQUIRE(Hmax > 0 && Wmax > 0 && max_size > 0, "Hmax, Wmax and max_size must be positive");
    SRCNN_REQUIRE(out_left && out_right, "null output pointer");
    SRCNN_REQUIRE(aligned16(out_left) && aligned16(out_right), "outputs must be 16-byte aligned");
    SRCNN_REQUIRE((unsigned long long)B * 3ull * (unsigned long long)Hmax * (unsigned long long)Wmax < (1ull << 31),
                  "a blob of 2^31 elements or more");
    TrainImageArgs a;
    for (int b = 0; b < SRCNN_LOADER_MAX_BATCH; ++b) a.slot[b] = TrainImage{nullptr, nullptr, 1.0, 1, 1, 0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
        const srcnn_train_image &s = slots_host[b];
        SRCNN_REQUIRE(s.left && s.right, "null image pointer");
        SRCNN_REQUIRE(s.H > 0 && s.W > 0 && s.H <= 32768 && s.W <= 32768, "image size out of range");
        SRCNN_REQUIRE(std::isfinite(s.scale) && s.scale > 0.0, "bad scale");
        // cv::resize derives the output size itself (cvRound = nearest, ties to even), blob.py:59-61 crops the columns
        const double oh = nearbyint((double)s.H * s.scale), ow = nearbyint((double)s.W * s.scale);
        SRCNN_REQUIRE(oh >= 1.0 && ow >= 1.0 && oh <= 1e6 && ow <= 1e6, "resized size out of range");
        const int OH = (int)oh, OWc = std::min((int)ow, max_size);
        SRCNN_REQUIRE(OH <= Hmax && OWc <= Wmax, "a resized image exceeds (Hmax, Wmax)");
        a.slot[b] = TrainImage{s.left, s.right, 1.0 / s.scale, s.H, s.W, OH, OWc, s.flipped ? 1 : 0, 0};
    }
    const size_t groups = ((size_t)B * 3 * Hmax * Wmax + 3) / 4;
    SRCNN_LAUNCH(preprocess_train_kernel, dim3(grid_for(groups, 256, 4096), 2), dim3(256), 0, as_stream(stream), a, B, Hmax, Wmax,
                 out_left, out_right);
    return check_launch("srcnn_preprocess_train");
}

}  // extern "C"
