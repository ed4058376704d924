// Depth errors on rendered rays: the arguments of the kernels of depth_err.hip and the arithmetic of
// compute_depth_error_on_rays (source/training/core/metrics.py:81-134) as plain functions of doubles and integers: which map and which
// pixel a rendered row reads, whether the row is kept, its error, and the two values at the end.  Double arithmetic on the fp32 operands,
// rounded once by the caller.  Nothing here touches a thread index, LDS or a HIP call; depth_err.hip owns the loop, the sums and the
// entry points.
// The file also compiles as plain C++ (tools/depth_err_host_check.cpp evaluates it on the host under the sanitizers).
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef DEPTH_ERR_DEV
#ifdef __HIPCC__
#define DEPTH_ERR_DEV __host__ __device__ __forceinline__
#else
#define DEPTH_ERR_DEV inline
#endif
#endif

namespace sparf {

enum {
    DEPTH_ERR_BLOCK = 256,       // four waves: the rows of a workgroup's stride
    DEPTH_ERR_CHUNK = 4096,      // rows up to which one workgroup does everything in one launch
    DEPTH_ERR_NACC = 5,          // K, S_abs, S_sq, S_abs_fine, S_sq_fine
    DEPTH_ERR_OUTS = 4,          // abs_e, rmse, abs_e_fine, rmse_fine
};

struct DepthErrArgs {
    const float* depth_gt;       // [B_maps][HW] as data_dict.depth_gt is stored
    const unsigned char* valid;  // [B_maps][HW] bytes (torch.bool storage), or null: every row is kept
    const int64_t* img_idx;      // [B] the map of rendered image b, or null: b itself
    const int64_t* ray_idx;      // [N] (per_image 0) or [B][N] (per_image 1), or null: the row itself (N == HW)
    int per_image, B_maps, B, HW, N, rows;       // rows = B N
    const float* depth;          // [B][N]
    const float* depth_fine;     // [B][N] or null
    float scale;
    const float* scale_dev;      // one float in device memory, or null; given, it wins
    float* out;                  // [4] (may be null without rows)
    int32_t* count;              // [1] (may be null without rows)
    double* ws;                  // [chunks][5] partial totals (rows > DEPTH_ERR_CHUNK), or null
};

// metrics.py:103-107: the map behind rendered image b -- img_idx[b], or b -- clamped to [0, B_maps)
static DEPTH_ERR_DEV int depth_err_image(const int64_t* img_idx, int b, int B_maps) {
    const int64_t m = img_idx ? img_idx[b] : (int64_t)b;
    return (int)(m < 0 ? 0 : m >= (int64_t)B_maps ? (int64_t)B_maps - 1 : m);
}

// metrics.py:108-125: the pixel behind row r of image b -- ray_idx[r], ray_idx[b][r], or r -- clamped to [0, HW)
static DEPTH_ERR_DEV int depth_err_pixel(const int64_t* ray_idx, int per_image, int b, int r, int N, int HW) {
    const int64_t p = ray_idx ? ray_idx[per_image ? (size_t)b * (size_t)N + (size_t)r : (size_t)r] : (int64_t)r;
    return (int)(p < 0 ? 0 : p >= (int64_t)HW ? (int64_t)HW - 1 : p);
}

// the element of a [B_maps][HW] map
static DEPTH_ERR_DEV size_t depth_err_at(int m, int p, int HW) { return (size_t)m * (size_t)HW + (size_t)p; }

// metrics.py:127: the boolean selection keeps a row whose mask byte is set
static DEPTH_ERR_DEV bool depth_err_kept(const unsigned char* valid, size_t at) { return !valid || valid[at] != 0; }

// metrics.py:128-130: e = depth_gt - pred s; s is a float32
static DEPTH_ERR_DEV double depth_err_row(float gt, float pred, float s) { return (double)gt - (double)pred * (double)s; }

// one head of a kept row into its two sums
static DEPTH_ERR_DEV void depth_err_add(double e, double& s_abs, double& s_sq) {
    s_abs += fabs(e);
    s_sq += e * e;
}

// everything of row r (of B N) into acc[DEPTH_ERR_NACC]: the map and the mask are read once for both heads
static DEPTH_ERR_DEV void depth_err_row_into(const DepthErrArgs& a, float s, int r, double* acc) {
    const int b = r / a.N, i = r - b * a.N;
    const size_t at = depth_err_at(depth_err_image(a.img_idx, b, a.B_maps), depth_err_pixel(a.ray_idx, a.per_image, b, i, a.N, a.HW), a.HW);
    if (!depth_err_kept(a.valid, at)) return;
    const float gt = a.depth_gt[at];
    acc[0] += 1.0;
    depth_err_add(depth_err_row(gt, a.depth[r], s), acc[1], acc[2]);
    if (a.depth_fine) depth_err_add(depth_err_row(gt, a.depth_fine[r], s), acc[3], acc[4]);
}

// metrics.py:130-131: sum |e| / (K + 1e-6); no kept row gives 0 / 1e-6 = 0
static DEPTH_ERR_DEV double depth_err_abs(double K, double s_abs) { return s_abs / (K + 1e-6); }

// metrics.py:78-79, :133: sqrt(mean e^2); the mean of no element is NaN
static DEPTH_ERR_DEV double depth_err_rmse(double K, double s_sq) { return K > 0.0 ? sqrt(s_sq / K) : (double)NAN; }

// the totals -> out[4] and count[1], each value rounded to float32 once; the fine pair is 0 without a fine head
static DEPTH_ERR_DEV void depth_err_outputs(const double* tot, bool fine, float* out, int32_t* count) {
    if (out) {
        out[0] = (float)depth_err_abs(tot[0], tot[1]);
        out[1] = (float)depth_err_rmse(tot[0], tot[2]);
        out[2] = fine ? (float)depth_err_abs(tot[0], tot[3]) : 0.0f;
        out[3] = fine ? (float)depth_err_rmse(tot[0], tot[4]) : 0.0f;
    }
    if (count) count[0] = (int32_t)tot[0];
}

}  // namespace sparf
