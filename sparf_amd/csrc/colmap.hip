// DS-NeRF sparse depth loss: what SparseCOLMAPDepthLoss.compute_loss (base_losses.py:326-402) runs around its
// renders -- per image a torch.where with a host readback, six index and gather operations and two weighted means, and one more
// torch.where over all images -- as three calls: compact (the valid pixels of every image in torch.where's order, their number and the
// number of positive pixels), gather (the selected rows of every image, packed in image order) and loss (the value and both gradient
// seeds).  The logic of a pixel and of a row is colmap.h's; this file owns the item of the compaction, the gather, the loss loop and the entry points.
//
// Compaction: B images at once, the image is the grid's y dimension.  It keeps row-major order and uses no atomics (ordered.h's chunked
// compaction over ColmapItem, in tiles of COLMAP_BLOCK consecutive pixels, with the positive pixels as a second, counted flag).  Up to
// COLMAP_CHUNK pixels one workgroup per image does all of it in one launch; above, a counts launch over chunks of COLMAP_CHUNK pixels
// and a write launch in which each workgroup adds the counts of the chunks before it in chunk order.  `count` stays in device memory;
// the host reads its 2 B ints once.
// Gather: one thread per selected row; the maps are read in place.  Every address comes from the index list and the device counts --
// clamped against the count and the image size -- and none from a value read out of a map.
// Loss: double arithmetic on the fp32 operands, one rounding per stored value.  Sums are fixed-order (ordered.h's chunked sum over
// ColmapLossSum): a thread adds its rows in index order, then the wave, the waves and the chunks in their order: the same bits from call to call.
#include <hip/hip_runtime.h>

#include "../../include/sparf_hip.h"
#include "colmap.h"
#include "ordered.h"

namespace sparf {

// what is compacted (the item of ordered.h's chunked compaction, B images): the valid pixels of image b, their flat indices as the rows;
// the positive pixels are counted along.  run[] = {valid, positive}; `finish` leaves both as the image's counts.
struct ColmapItem {
    typedef ColmapCompactArgs Args;
    typedef OrderedNoShared Shared;
    static constexpr int BLOCK = COLMAP_BLOCK, CHUNK = COLMAP_CHUNK, NCOUNT = 2;
    static __host__ __device__ int n(const ColmapCompactArgs& a) { return a.n; }
    static __host__ __device__ int32_t* ws(const ColmapCompactArgs& a) { return a.ws; }
    const float* depth;
    int32_t* index;
    __device__ ColmapItem(const ColmapCompactArgs& a, const OrderedNoShared*, int b)
        : depth(a.depth + (size_t)b * (size_t)a.n), index(a.index + (size_t)b * (size_t)a.n) {}
    __device__ void flags(int p, bool in, bool (&f)[2]) const {
        const float d = in ? depth[p] : 0.0f;            // one guarded read for both flags
        f[0] = in & colmap_valid(d);
        f[1] = in & colmap_positive(d);
    }
    __device__ void place(int p, int j) const { index[j] = p; }
    __device__ void mark(int, int) const {}
    static __device__ void finish(const ColmapCompactArgs& a, int b, const int (&run)[2]) {
        a.count[b] = run[0];
        a.count[a.B + b] = run[1];
    }
};

// base_losses.py:378-386 for row j of image b: the pixel behind the j-th selected entry of the image's index list, and what the two
// maps hold there
__global__ void __launch_bounds__(COLMAP_BLOCK) colmap_gather_kernel(ColmapGatherArgs a) {
    const int b = (int)blockIdx.y, j = (int)blockIdx.x * COLMAP_BLOCK + (int)threadIdx.x;
    const int count = a.count[b];
    if (j >= colmap_rows(count, a.quota)) return;
    const int r = colmap_offset(a.count, b, a.quota) + j;
    if (r >= a.K) return;                                // (the caller's K is the sum of the rows: never taken then)
    const size_t image = (size_t)b * (size_t)a.n;
    const int p = colmap_pixel_of_row(a.index + image, a.sel ? a.sel + (size_t)b * (size_t)a.quota : nullptr, count, a.quota, a.n, j);
    a.ray_idx[r] = (int64_t)p;
    a.target[r] = a.depth[image + (size_t)p];
    a.weight[r] = a.conf[image + (size_t)p];
}

// the rows first, first + COLMAP_BLOCK, ... < end: -> the sum of their terms over k_b, their seeds stored
static __device__ double colmap_loss_loop(const ColmapLossArgs& a, int first, int end) {
    double acc = 0.0;
    for (int r = first; r < end; r += COLMAP_BLOCK) {
        int b, j, k;
        if (!colmap_locate(a.count, a.B, a.quota, r, b, j, k)) {      // (a row past the images' rows: the caller's K is too large)
            if (a.d_depth) a.d_depth[r] = 0.0f;
            if (a.d_depth_fine) a.d_depth_fine[r] = 0.0f;
            continue;
        }
        const double d = (double)a.target[r], w = (double)a.weight[r], p = (double)a.depth[r];
        const double pf = a.depth_fine ? (double)a.depth_fine[r] : 0.0;
        acc += colmap_row_term(d, w, p, a.depth_fine != nullptr, pf) / (double)k;
        if (a.d_depth) a.d_depth[r] = (float)colmap_row_seed(d, w, p, k, a.B);
        if (a.d_depth_fine) a.d_depth_fine[r] = (float)colmap_row_seed(d, w, pf, k, a.B);
    }
    return acc;
}

// the policy of ordered.h's chunked sum: one total
struct ColmapLossSum {
    typedef ColmapLossArgs Args;
    static constexpr int BLOCK = COLMAP_BLOCK, CHUNK = COLMAP_CHUNK, NACC = 1;
    static __host__ __device__ int rows(const ColmapLossArgs& a) { return a.K; }
    static __host__ __device__ double* ws(const ColmapLossArgs& a) { return a.ws; }
    static __device__ void loop(const ColmapLossArgs& a, int first, int end, double* acc) { acc[0] = colmap_loss_loop(a, first, end); }
    static __device__ void outputs(const ColmapLossArgs& a, const double* tot) { a.out[0] = (float)colmap_total(tot[0], a.B); }
};

}  // namespace sparf

using namespace sparf;

// ---- the entry points (sparf_hip.h): every argument check comes before any HIP call
static const int64_t kColmapMax = (int64_t)1 << 30;

int64_t sparf_colmap_workspace_bytes(int B, int64_t n, int64_t rows) {
    int64_t compact = 0, loss = 0;
    if (B > 0 && B <= COLMAP_MAX_IMAGES && n <= kColmapMax) compact = ordered_compact_workspace_bytes<ColmapItem>(n, B);
    if (rows <= kColmapMax) loss = ordered_sum_workspace_bytes<ColmapLossSum>(rows);
    return compact > loss ? compact : loss;
}

int sparf_colmap_compact(const float* depth, int B, int H, int W, int32_t* index, int32_t* count, void* workspace, void* stream) {
    if (B <= 0 || B > COLMAP_MAX_IMAGES || H < 0 || W < 0 || (int64_t)H * W > kColmapMax || !count) return 1;
    hipStream_t s = (hipStream_t)stream;
    const int n = H * W;
    if (n == 0) return hipMemsetAsync(count, 0, 2 * (size_t)B * sizeof(int32_t), s) == hipSuccess ? 0 : 2;      // (an empty tensor has no address)
    if (!depth || !index) return 1;
    ColmapCompactArgs a{};
    a.depth = depth; a.B = B; a.n = n; a.index = index; a.count = count; a.ws = (int32_t*)workspace;
    return launch_ordered_compact<ColmapItem>(a, B, s);
}

int sparf_colmap_gather(const int32_t* index, const int32_t* count, const int64_t* sel, int B, int H, int W, int quota, int K, const float* depth,
                        const float* conf, int64_t* ray_idx, float* target, float* weight, void* stream) {
    if (B <= 0 || B > COLMAP_MAX_IMAGES || H < 0 || W < 0 || (int64_t)H * W > kColmapMax || quota < 0 || K < 0 || (int64_t)K > kColmapMax) return 1;
    if ((int64_t)K > (int64_t)B * quota || (int64_t)K > (int64_t)B * H * W) return 1;      // more rows than the images can hold
    if (K == 0) return 0;
    if (!index || !count || !depth || !conf || !ray_idx || !target || !weight) return 1;
    ColmapGatherArgs a{};
    a.index = index; a.count = count; a.sel = sel; a.B = B; a.n = H * W; a.quota = quota; a.K = K;
    a.depth = depth; a.conf = conf; a.ray_idx = ray_idx; a.target = target; a.weight = weight;
    const int per_image = quota < a.n ? quota : a.n;
    hipLaunchKernelGGL(colmap_gather_kernel, dim3((per_image + COLMAP_BLOCK - 1) / COLMAP_BLOCK, B), dim3(COLMAP_BLOCK), 0, (hipStream_t)stream, a);
    return launched();
}

int sparf_colmap_loss(const float* target, const float* weight, const int32_t* count, int B, int quota, int K, const float* depth,
                      const float* depth_fine, float* out, float* d_depth, float* d_depth_fine, void* workspace, void* stream) {
    if (B <= 0 || B > COLMAP_MAX_IMAGES || quota < 0 || K < 0 || (int64_t)K > kColmapMax || (d_depth_fine && !depth_fine)) return 1;
    if (K == 0) return 0;                                // nothing to launch, no pointer looked at: the loss of no rows is the caller's zero
    if (!target || !weight || !count || !depth || !out) return 1;
    ColmapLossArgs a{};
    a.target = target; a.weight = weight; a.count = count; a.B = B; a.quota = quota; a.K = K; a.depth = depth; a.depth_fine = depth_fine;
    a.out = out; a.d_depth = d_depth; a.d_depth_fine = d_depth_fine; a.ws = (double*)workspace;
    return launch_ordered_sum<ColmapLossSum>(a, (hipStream_t)stream);
}
