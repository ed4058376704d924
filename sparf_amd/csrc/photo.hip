// Photometric, mask and depth-patch loss: BasePhotoandReguLoss.compute_loss (base_losses.py:243-323 with the depth-patch
// regulariser of :180-194) and compute_mse_on_rays (metrics.py:33-75) as one call -- the five outputs and the six gradient seeds from one
// pass over the rows.  The arithmetic of an element is photo.h's; this file owns the gather, the loops, the reductions and the entry point.
//
// Gather: a row reads its ground-truth colours and its mask byte in place, image[b][c][idx] and fg_mask[b][idx] with idx = ray_idx[r],
// ray_idx[b][r] or r; no target tensor exists.  Indices may repeat; nothing is scattered, so there is no atomic.  An index outside
// [0, HW) is the caller's error (torch raises on it); it is clamped here so that the launch stays inside the image.
// Depth patches: a row sums over the P^2 partners of its own patch (read from global memory, wherever the patch lies relative to a
// chunk of rows), so every row's patch sum and seed are its own and no patch is split between workgroups.
// Sums are fixed-order, by ordered.h's chunked sum over PhotoSum: a thread adds its rows in index order, then the wave, the waves and
// the chunks in their order.  Up to PHOTO_CHUNK rows (or without a workspace) one workgroup does all of it in one launch; above, a
// launch of one workgroup per chunk that leaves partial totals and a second one that adds them.  No host synchronisation, no readback.
#include <hip/hip_runtime.h>

#include "../../include/sparf_hip.h"
#include "ordered.h"
#include "photo.h"

namespace sparf {

struct PhotoDepths {             // the depths of one patch, by position
    const float* p;
    __device__ double operator()(int j) const { return (double)p[j]; }
};

// one head of the colour term for row r: its three channels against the gathered pixel
static __device__ void photo_colour_row(const PhotoArgs& a, const PhotoScales& sc, const double target[3], const float* pred, float* seed, int r,
                                        double& sum_l, double& sum_e2) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double e = (double)pred[3 * (size_t)r + c] - target[c];
        double l, dl;
        photo_colour(a.kind, (double)a.delta, e, l, dl);
        sum_l += l;
        sum_e2 += e * e;
        if (seed) seed[3 * (size_t)r + c] = (float)(dl * sc.colour);
    }
}
static __device__ void photo_mask_row(const PhotoScales& sc, double fg, const float* opacity, float* seed, int r, double& sum) {
    double l;
    const double g = photo_mask(fg, (double)opacity[r], l);
    sum += l;
    if (seed) seed[r] = (float)(g * sc.mask);
}
static __device__ void photo_patch_of_row(const PhotoArgs& a, const PhotoScales& sc, const float* depth, float* seed, int r, double& sum) {
    const int M = a.patch * a.patch, i = r % M;           // (N % M == 0: a patch lies inside one image, and r - i is its first row)
    const PhotoDepths d{depth + (size_t)(r - i)};
    double s;
    const double g = photo_patch_row(d, M, i, (double)a.charbonnier, s);
    sum += s;
    if (seed) seed[r] = (float)(g * sc.patch);
}

// the rows first, first + PHOTO_BLOCK, ... < end into acc, their seeds stored
static __device__ void photo_loop(const PhotoArgs& a, int first, int end, double acc[PHOTO_NACC]) {
    const PhotoScales sc = photo_scales(a.kind, a.rows, a.patch);
#pragma unroll
    for (int j = 0; j < PHOTO_NACC; ++j) acc[j] = 0.0;
    for (int r = first; r < end; r += PHOTO_BLOCK) {
        const int b = r / a.N, i = r - b * a.N;
        int64_t idx = a.ray_idx ? a.ray_idx[a.per_image ? (size_t)r : (size_t)i] : (int64_t)i;
        idx = idx < 0 ? 0 : idx >= (int64_t)a.HW ? (int64_t)a.HW - 1 : idx;
        const float* px = a.image + (size_t)b * 3 * (size_t)a.HW + (size_t)idx;
        const double target[3] = {(double)px[0], (double)px[(size_t)a.HW], (double)px[2 * (size_t)a.HW]};
        photo_colour_row(a, sc, target, a.rgb, a.d_rgb, r, acc[0], acc[2]);
        if (a.rgb_fine) photo_colour_row(a, sc, target, a.rgb_fine, a.d_rgb_fine, r, acc[1], acc[3]);
        if (a.fg_mask) {
            const double fg = a.fg_mask[(size_t)b * (size_t)a.HW + (size_t)idx] ? 1.0 : 0.0;
            photo_mask_row(sc, fg, a.opacity, a.d_opacity, r, acc[4]);
            if (a.opacity_fine) photo_mask_row(sc, fg, a.opacity_fine, a.d_opacity_fine, r, acc[5]);
        } else {                                         // a seed of a term that is off: the derivative of a constant 0
            if (a.d_opacity) a.d_opacity[r] = 0.0f;
            if (a.d_opacity_fine) a.d_opacity_fine[r] = 0.0f;
        }
        if (a.patch) {
            photo_patch_of_row(a, sc, a.depth, a.d_depth, r, acc[6]);
            if (a.depth_fine) photo_patch_of_row(a, sc, a.depth_fine, a.d_depth_fine, r, acc[7]);
        } else {
            if (a.d_depth) a.d_depth[r] = 0.0f;
            if (a.d_depth_fine) a.d_depth_fine[r] = 0.0f;
        }
    }
}

// the policy of ordered.h's chunked sum
struct PhotoSum {
    typedef PhotoArgs Args;
    static constexpr int BLOCK = PHOTO_BLOCK, CHUNK = PHOTO_CHUNK, NACC = PHOTO_NACC;
    static __host__ __device__ int rows(const PhotoArgs& a) { return a.rows; }
    static __host__ __device__ double* ws(const PhotoArgs& a) { return a.ws; }
    static __device__ void loop(const PhotoArgs& a, int first, int end, double* acc) { photo_loop(a, first, end, acc); }
    static __device__ void outputs(const PhotoArgs& a, const double* tot) { photo_outputs(a, tot); }
};

}  // namespace sparf

using namespace sparf;

// ---- the entry point (sparf_hip.h): every argument check comes before any HIP call; rows == 0 launches no kernel
static const int64_t kPhotoMaxRows = (int64_t)1 << 30;

int64_t sparf_photo_regu_workspace_bytes(int64_t rows) {
    return rows <= kPhotoMaxRows ? ordered_sum_workspace_bytes<PhotoSum>(rows) : 0;
}

int sparf_photo_regu_loss(const float* image, const unsigned char* fg_mask, const int64_t* ray_idx, int per_image, int B, int HW, int N,
                          const float* rgb, const float* rgb_fine, const float* opacity, const float* opacity_fine, const float* depth,
                          const float* depth_fine, int kind, float delta, int patch, float charbonnier, float* out, float* d_rgb,
                          float* d_rgb_fine, float* d_opacity, float* d_opacity_fine, float* d_depth, float* d_depth_fine, void* workspace,
                          void* stream) {
    if (B < 0 || HW < 0 || N < 0 || (int64_t)B * N > kPhotoMaxRows || (int64_t)B * 3 * HW > ((int64_t)1 << 40)) return 1;
    if (kind < 0 || kind >= PHOTO_KINDS || patch < 0 || patch > PHOTO_MAX_PATCH || !out) return 1;
    if (patch > 0 && (N % (patch * patch) != 0 || !depth)) return 1;
    if ((d_rgb_fine && !rgb_fine) || (d_opacity_fine && !opacity_fine) || (d_depth_fine && !depth_fine)) return 1;
    if ((d_opacity && !opacity) || (d_depth && !depth) || (fg_mask && !opacity)) return 1;
    if (!ray_idx && N != HW && (int64_t)B * N != 0) return 1;          // the identity is a full image
    hipStream_t s = (hipStream_t)stream;
    const int rows = B * N;
    if (rows == 0) return hipMemsetAsync(out, 0, PHOTO_OUTS * sizeof(float), s) == hipSuccess ? 0 : 2;      // (an empty tensor has no address)
    if (!image || !rgb || HW == 0) return 1;
    PhotoArgs a{};
    a.B = B; a.HW = HW; a.N = N; a.rows = rows; a.per_image = per_image != 0; a.kind = kind; a.patch = patch;
    a.delta = delta; a.charbonnier = charbonnier;
    a.image = image; a.fg_mask = fg_mask; a.ray_idx = ray_idx; a.rgb = rgb; a.rgb_fine = rgb_fine;
    a.opacity = opacity; a.opacity_fine = opacity_fine; a.depth = depth; a.depth_fine = depth_fine; a.out = out;
    a.d_rgb = d_rgb; a.d_rgb_fine = d_rgb_fine; a.d_opacity = d_opacity; a.d_opacity_fine = d_opacity_fine;
    a.d_depth = d_depth; a.d_depth_fine = d_depth_fine; a.ws = (double*)workspace;
    return launch_ordered_sum<PhotoSum>(a, s);
}
