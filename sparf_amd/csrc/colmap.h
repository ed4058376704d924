// DS-NeRF sparse depth loss: the arguments of the kernels of colmap.hip and the per-pixel and per-row arithmetic of
// SparseCOLMAPDepthLoss.compute_loss (base_losses.py:326-402) as plain functions: which pixels of a COLMAP depth map are valid and which
// positive, how many rows an image contributes, the image and the position of a packed row, the clamped entry of the index list behind
// a row, and the loss term and gradient seeds of a row.  Selection is compare and copy work: a result equals the reference's bit for bit
// or is wrong.  The loss is double arithmetic on the fp32 operands, rounded once by the caller.  Nothing here touches a thread index, LDS
// or a HIP call; colmap.hip owns the ordered compaction, the gather and the sums.
// The file also compiles as plain C++ (tools/colmap_host_check.cpp evaluates it on the host under the sanitizers).
#pragma once
#include <stdint.h>

#ifndef COLMAP_DEV
#ifdef __HIPCC__
#define COLMAP_DEV __host__ __device__ __forceinline__
#else
#define COLMAP_DEV inline
#endif
#endif

namespace sparf {

enum {
    COLMAP_BLOCK = 256,          // four waves: a tile of the compaction, and the rows of a gather or loss workgroup
    COLMAP_CHUNK = 4096,         // pixels (rows) up to which one workgroup per image (one workgroup) does everything in one launch
    COLMAP_MAX_IMAGES = 65535,   // the image index is the grid's y dimension
};

struct ColmapCompactArgs {
    const float* depth;          // [B][n] as colmap_depth [B,1,H,W] is stored
    int B, n, chunks;            // n = H W; chunks of COLMAP_CHUNK pixels per image
    int32_t* index;              // [B][n]: per image the flat indices of its valid pixels, ascending
    int32_t* count;              // [2 B]: valid pixels per image, then positive pixels per image
    int32_t* ws;                 // [B][chunks][2] valid and positive pixels per chunk (n > COLMAP_CHUNK), or null
};

struct ColmapGatherArgs {
    const int32_t* index;        // [B][n]
    const int32_t* count;        // [2 B], its first B entries read
    const int64_t* sel;          // [B][quota] positions in index[b], read where count[b] > quota; or null: the first rows everywhere
    int B, n, quota, K;          // K: the rows the outputs hold
    const float* depth;          // [B][n]
    const float* conf;           // [B][n]
    int64_t* ray_idx;            // [K]
    float* target;               // [K]
    float* weight;               // [K]
};

struct ColmapLossArgs {
    const float* target;         // [K]
    const float* weight;         // [K]
    const int32_t* count;        // [B]: image b holds min(count[b], quota) consecutive rows
    int B, quota, K;
    const float* depth;          // [K]
    const float* depth_fine;     // [K] or null
    float* out;                  // [1]
    float* d_depth;              // [K] or null
    float* d_depth_fine;         // [K] or null
    double* ws;                  // [chunks] partial sums (K > COLMAP_CHUNK), or null
};

// base_losses.py:372 colmap_depth_i > 1e-6: a float32 tensor against a Python number is a float32 compare
static COLMAP_DEV bool colmap_valid(float d) { return d > 1e-6f; }

// base_losses.py:367 colmap_depth > 0
static COLMAP_DEV bool colmap_positive(float d) { return d > 0.0f; }

// base_losses.py:374-380: the rows of an image with `count` valid pixels -- all of them up to the quota, the quota above it
static COLMAP_DEV int colmap_rows(int count, int quota) { return count < 0 ? 0 : count < quota ? count : quota; }

// base_losses.py:377: a permutation is drawn only ABOVE the quota
static COLMAP_DEV bool colmap_draws(int count, int quota) { return count > quota; }

// packed row r of K = sum_b k_b rows in image order -> its image b, its position j in it and k_b; false past the last row
static COLMAP_DEV bool colmap_locate(const int32_t* count, int B, int quota, int r, int& b, int& j, int& k) {
    int off = 0;
    for (b = 0; b < B; ++b) {
        k = colmap_rows(count[b], quota);
        if (r < off + k) {
            j = r - off;
            return true;
        }
        off += k;
    }
    return false;
}

// the first packed row of image b
static COLMAP_DEV int colmap_offset(const int32_t* count, int b, int quota) {
    int off = 0;
    for (int i = 0; i < b; ++i) off += colmap_rows(count[i], quota);
    return off;
}

// base_losses.py:378-380: the entry of image b's index list behind row j -- position sel[j] where a permutation was drawn, else j --
// clamped against the count, and the pixel it holds clamped against the image
static COLMAP_DEV int colmap_pixel_of_row(const int32_t* index_b, const int64_t* sel_b, int count, int quota, int n, int j) {
    const int64_t last = (int64_t)(count < 1 ? 1 : count > n ? n : count) - 1;
    int64_t s = sel_b && colmap_draws(count, quota) ? sel_b[j] : (int64_t)j;
    s = s < 0 ? 0 : s > last ? last : s;
    const int p = index_b[s];
    return p < 0 ? 0 : p >= n ? n - 1 : p;
}

// base_losses.py:392 / :397 for one row: w ((d - p)^2 [+ (d - pf)^2]); the caller divides by k_b and scales by 0.1 / B (:400)
static COLMAP_DEV double colmap_row_term(double d, double w, double p, bool fine, double pf) {
    const double e = d - p, ef = d - pf;
    return fine ? w * (e * e + ef * ef) : w * (e * e);
}

// dL/dp of one row: (0.1 / B) (2 / k_b) w (p - d)
static COLMAP_DEV double colmap_row_seed(double d, double w, double p, int k, int B) { return (0.1 / (double)B) * (2.0 / (double)k) * w * (p - d); }

// base_losses.py:400 on the sum over images of their per-image means
static COLMAP_DEV double colmap_total(double sum_of_means, int B) { return (0.1 / (double)B) * sum_of_means; }

}  // namespace sparf
