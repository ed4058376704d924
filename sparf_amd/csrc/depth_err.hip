// Depth errors on rendered rays: compute_depth_error_on_rays (source/training/core/metrics.py:81-134), which the
// trainers run once per head on every training iteration -- two indexed copies of every map, an index build and two gathers, two boolean
// selections with their readbacks and eight small reductions -- as one call for both heads.  The arithmetic of a row is depth_err.h's;
// this file owns the loop, the sums and the entry points.
//
// Gather: a row reads its ground-truth depth and its mask byte in place, depth_gt[m][p] and valid[m][p] with m = img_idx[b] or b and
// p = ray_idx[r], ray_idx[b][r] or r; no indexed copy of a map exists, and the fine head shares the coarse head's reads.  Indices may
// repeat; nothing is scattered, so there is no atomic.  An index outside its range is the caller's error (torch raises on it); it is
// clamped here so that the launch stays inside the maps.  No address depends on a value read from a map.
// Sums are fixed-order, by ordered.h's chunked sum over DepthErrSum: a thread adds its rows in index order, then the wave, the waves and
// the chunks in their order: the same bits from call to call.  Up to DEPTH_ERR_CHUNK rows (or without a workspace) one workgroup does
// all of it in one launch; above, a launch of one workgroup per chunk that leaves partial totals and a second one that adds them.  No
// workgroup waits for another, no host synchronisation, no readback.
#include <hip/hip_runtime.h>

#include "../../include/sparf_hip.h"
#include "depth_err.h"
#include "ordered.h"

namespace sparf {

// the rows first, first + DEPTH_ERR_BLOCK, ... < end into acc
static __device__ void depth_err_loop(const DepthErrArgs& a, int first, int end, double acc[DEPTH_ERR_NACC]) {
#pragma unroll
    for (int j = 0; j < DEPTH_ERR_NACC; ++j) acc[j] = 0.0;
    if (first >= end) return;                            // (no row: the scale is not read either)
    const float s = a.scale_dev ? a.scale_dev[0] : a.scale;
    for (int r = first; r < end; r += DEPTH_ERR_BLOCK) depth_err_row_into(a, s, r, acc);
}

// the policy of ordered.h's chunked sum
struct DepthErrSum {
    typedef DepthErrArgs Args;
    static constexpr int BLOCK = DEPTH_ERR_BLOCK, CHUNK = DEPTH_ERR_CHUNK, NACC = DEPTH_ERR_NACC;
    static __host__ __device__ int rows(const DepthErrArgs& a) { return a.rows; }
    static __host__ __device__ double* ws(const DepthErrArgs& a) { return a.ws; }
    static __device__ void loop(const DepthErrArgs& a, int first, int end, double* acc) { depth_err_loop(a, first, end, acc); }
    static __device__ void outputs(const DepthErrArgs& a, const double* tot) { depth_err_outputs(tot, a.depth_fine != nullptr, a.out, a.count); }
};

}  // namespace sparf

using namespace sparf;

// ---- the entry points (sparf_hip.h): every argument check comes before any HIP call
static const int64_t kDepthErrMax = (int64_t)1 << 30;

int64_t sparf_ray_depth_err_workspace_bytes(int64_t rows) {
    return rows <= kDepthErrMax ? ordered_sum_workspace_bytes<DepthErrSum>(rows) : 0;
}

int sparf_ray_depth_err(const float* depth_gt, const unsigned char* valid, const int64_t* img_idx, const int64_t* ray_idx, int per_image,
                        int B_maps, int B, int HW, int N, const float* depth, const float* depth_fine, float scale, const float* scale_dev,
                        float* out, int32_t* count, void* workspace, void* stream) {
    if (B_maps <= 0 || B < 0 || HW < 0 || N < 0 || (int64_t)B * HW > kDepthErrMax || (int64_t)B * N > kDepthErrMax) return 1;
    if (per_image != 0 && per_image != 1) return 1;
    const int rows = B * N;
    if (!ray_idx && N != HW && rows != 0) return 1;      // the identity is a full image (an empty index list has no address)
    if (rows > 0 && (!depth_gt || !depth || !out || !count || HW == 0)) return 1;
    if (rows == 0 && !out && !count) return 0;           // nothing to write
    DepthErrArgs a{};
    a.depth_gt = depth_gt; a.valid = valid; a.img_idx = img_idx; a.ray_idx = ray_idx; a.per_image = per_image;
    a.B_maps = B_maps; a.B = B; a.HW = HW; a.N = N; a.rows = rows; a.depth = depth; a.depth_fine = depth_fine;
    a.scale = scale; a.scale_dev = scale_dev; a.out = out; a.count = count; a.ws = (double*)workspace;
    // (rows == 0: one launch, no input is read, the totals are zero: abs_e 0, rmse NaN, count 0)
    return launch_ordered_sum<DepthErrSum>(a, (hipStream_t)stream);
}
