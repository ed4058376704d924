// The depth-consistency front end and the ray sampler: what runs in front of the renders of DepthConsistencyLoss
// (depth_cons_loss.py:45-63 sample_pose, :103-106 / :168-188 the pose preparation and sample_rays) and first in every iteration of every
// trainer (sampling_strategies.py:132-188 RaySamplingStrategy.__call__), as two kernels.  The arithmetic is pick.h's; this file owns
// the loops and the entry points.
//
// sparf_pick_pixels: one launch, one thread per output row.  A row reads one permutation entry (clamped into its pool: no address and
// no pixel depends on a wild value) and writes its pixel and / or its ray index with plain stores; rows never share an output.
// sparf_unseen_pose: one launch of one wave.  Lane l takes the cameras l, l + 64, ... and keeps the first index of its smallest
// angular distance; an xor butterfly leaves the first index of the minimum in every lane; lanes 0..15 then write one element of each
// of the four matrices, and lane 0 the index.  No LDS, no atomic, no workgroup waits for another, no readback: the same bits from call
// to call.
#include <hip/hip_runtime.h>

#include "../../include/sparf_hip.h"
#include "ordered.h"
#include "pick.h"

namespace sparf {

__global__ __launch_bounds__(PICK_BLOCK) void pick_pixels_kernel(const PickPixelsArgs a) {
    const int row = (int)blockIdx.x * PICK_BLOCK + (int)threadIdx.x;
    if (row < a.rows) pick_row(a, row);
}

__global__ __launch_bounds__(PICK_WAVE) void unseen_pose_kernel(const UnseenPoseArgs a) {
    const int lane = (int)threadIdx.x;
    double best;
    int at;
    pick_nearest(a, lane, PICK_WAVE, best, at);
#pragma unroll
    for (int d = PICK_WAVE / 2; d >= 1; d >>= 1) {
        const double e = __shfl_xor(best, d, PICK_WAVE);
        const int k = __shfl_xor(at, d, PICK_WAVE);
        if (pick_before(e, k, best, at)) { best = e; at = k; }
    }
    // (B >= 1: some lane holds a camera, and `at` is its index in every lane)
    if (lane < 16) pick_pose_outputs(a, at, lane);
    if (lane == 0) a.id_other[0] = (int32_t)at;
}

}  // namespace sparf

using namespace sparf;

// ---- the entry points (sparf_hip.h): every argument check comes before any HIP call
static const int64_t kPickMaxRows = (int64_t)1 << 30;
static const int kPickMaxPoses = 1 << 20;

// a pool with picks: not empty, its index an int, and pool + patch - 1 inside a row of the image
static bool pick_pool_ok(int n, const int64_t* perm, int x0, int y0, int w, int h, int W, int patch) {
    if (n == 0) return true;
    return perm && x0 >= 0 && y0 >= 0 && w > 0 && h > 0 && (int64_t)w * h <= kPickMaxRows && (int64_t)x0 + w + patch - 1 <= (int64_t)W;
}

int sparf_pick_pixels(const int64_t* perm_a, int n_a, const int64_t* perm_b, int n_b, int a_w, int a_h, int b_x0, int b_y0, int b_w, int b_h,
                      int W, int patch, float* pixels, int64_t* rays, void* stream) {
    if (n_a < 0 || n_b < 0 || W <= 0 || patch < 1 || patch > 1024) return 1;
    const int64_t rows = ((int64_t)n_a + n_b) * patch * patch;
    if (rows > kPickMaxRows) return 1;
    if (!pick_pool_ok(n_a, perm_a, 0, 0, a_w, a_h, W, patch) || !pick_pool_ok(n_b, perm_b, b_x0, b_y0, b_w, b_h, W, patch)) return 1;
    if (rows == 0 || (!pixels && !rays)) return 0;       // nothing to write
    PickPixelsArgs a{};
    a.perm_a = perm_a; a.perm_b = perm_b; a.n_a = n_a; a.n_b = n_b; a.a_w = a_w; a.a_h = a_h;
    a.b_x0 = b_x0; a.b_y0 = b_y0; a.b_w = b_w; a.b_h = b_h; a.W = W; a.patch = patch; a.rows = (int)rows;
    a.pixels = pixels; a.rays = rays;
    hipLaunchKernelGGL(pick_pixels_kernel, dim3((unsigned)((rows + PICK_BLOCK - 1) / PICK_BLOCK)), dim3(PICK_BLOCK), 0, (hipStream_t)stream, a);
    return launched();
}

int sparf_unseen_pose(const float* poses_w2c, int row_floats, int B, int id_self, float w, float one_minus_w, float* pose_w2c_ref,
                      float* pose_c2w_ref, float* pose_c2w_other, float* pose_w2c_at_unseen, int32_t* id_other, void* stream) {
    if ((row_floats != 12 && row_floats != 16) || B < 1 || B > kPickMaxPoses || id_self < 0 || id_self >= B) return 1;
    if (!poses_w2c || !pose_w2c_ref || !pose_c2w_ref || !pose_c2w_other || !pose_w2c_at_unseen || !id_other) return 1;
    UnseenPoseArgs a{};
    a.poses_w2c = poses_w2c; a.row_floats = row_floats; a.B = B; a.id_self = id_self; a.w = w; a.one_minus_w = one_minus_w;
    a.w2c_ref = pose_w2c_ref; a.c2w_ref = pose_c2w_ref; a.c2w_other = pose_c2w_other; a.w2c_unseen = pose_w2c_at_unseen; a.id_other = id_other;
    hipLaunchKernelGGL(unseen_pose_kernel, dim3(1), dim3(PICK_WAVE), 0, (hipStream_t)stream, a);
    return launched();
}
