// Photometric, mask and depth-patch loss: the arguments of the kernels of photo.hip and the arithmetic of
// BasePhotoandReguLoss.compute_loss (base_losses.py:243-323, :180-194; regularization_losses.py:51-66) and compute_mse_on_rays
// (metrics.py:26-31, :71-74) as plain functions of doubles.  Every value is taken to double as it is loaded and each result is rounded to
// float once, on its store (the contract of reproj.h and dcons.h).  Nothing here touches a thread index, LDS or a HIP call: the functions
// state the mathematics of ONE element, of one patch row and of the five outputs; photo.hip owns the gather, the loops and the reductions.
// The file also compiles as plain C++ (tools/photo_host_check.cpp evaluates it on the host under the sanitizers).
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef PHOTO_DEV
#ifdef __HIPCC__
#define PHOTO_DEV __host__ __device__ __forceinline__
#else
#define PHOTO_DEV inline
#endif
#endif

namespace sparf {

enum { PHOTO_MSE = 0, PHOTO_HUBER = 1, PHOTO_KINDS = 2 };
enum {
    PHOTO_BLOCK = 512,           // eight waves, two per SIMD: the one workgroup of a SPARF step (4 x 1024 rays) holds eight rows a thread (at 1024 threads the one-workgroup kernel spills)
    PHOTO_CHUNK = 4096,          // rows up to which one workgroup does everything in one launch; above, the rows of one workgroup
    PHOTO_MAX_PATCH = 8,         // P: a patch is P^2 <= 64 consecutive rays
    PHOTO_OUTS = 5,              // out: render, fg_mask, depth_patch, mse, mse_fine
    // totals: [0] sum l (colour, coarse), [1] the same (fine), [2] sum e^2 (coarse), [3] (fine), [4] sum |fg - opacity| (coarse), [5] (fine),
    // [6] sum over patches and pairs (coarse), [7] (fine)
    PHOTO_NACC = 8,
};

struct PhotoArgs {
    int B, HW, N, rows, per_image, kind, patch;          // rows = B N; patch = P or 0
    float delta, charbonnier;
    const float* image;                                  // [B][3][HW]
    const unsigned char* fg_mask;                        // [B][HW] or null
    const int64_t* ray_idx;                              // [N], [B][N] (per_image) or null: identity
    const float *rgb, *rgb_fine;                         // [rows][3]; fine or null
    const float *opacity, *opacity_fine, *depth, *depth_fine;      // [rows] each, or null
    float* out;                                          // [PHOTO_OUTS]
    float *d_rgb, *d_rgb_fine, *d_opacity, *d_opacity_fine, *d_depth, *d_depth_fine;      // seeds, or null each
    double* ws;                                          // [chunks][PHOTO_NACC] partial totals (rows > PHOTO_CHUNK), or null
};

// base_losses.py:151-156 on one difference e = pred - target: kind 0  l = e^2; kind 1  torch.nn.functional.huber_loss with delta
// (the module's huber_loss: delta 0.5, mean, then x 2 -- the 2 is photo_scales').  dl = d l / d e
static PHOTO_DEV void photo_colour(int kind, double delta, double e, double& l, double& dl) {
    if (kind == PHOTO_MSE) {
        l = e * e;
        dl = 2.0 * e;
        return;
    }
    const double ab = fabs(e);
    if (ab <= delta) {
        l = 0.5 * e * e;
        dl = e;
    } else {
        l = delta * (ab - 0.5 * delta);
        dl = e > 0.0 ? delta : -delta;
    }
}

// base_losses.py:316: a = fg - opacity, l = |a|; -> d l / d opacity = -sgn(a) with sgn(0) = 0, as torch's abs gives
static PHOTO_DEV double photo_mask(double fg, double opacity, double& l) {
    const double a = fg - opacity;
    l = fabs(a);
    return a > 0.0 ? -1.0 : a < 0.0 ? 1.0 : 0.0;
}

// regularization_losses.py:65-66 for row i of a patch of M depths d[0..M): s = sum_j sqrt((d_i - d_j)^2 + c^2) over all M partners, the
// diagonal included, in j order; -> d (sum over ALL ordered pairs) / d d_i = 2 sum_j (d_i - d_j) / sqrt((d_i - d_j)^2 + c^2) (a pair
// appears twice, as (i, j) and as (j, i)).  A constant patch gives s = M c and exactly 0.
template <class Load>
static PHOTO_DEV double photo_patch_row(const Load& d, int M, int i, double c, double& s) {
    const double di = d(i), cc = c * c;
    double g = 0.0;
    s = 0.0;
    for (int j = 0; j < M; ++j) {
        const double r = di - d(j);
        const double q = sqrt(r * r + cc);
        s += q;
        g += r / q;
    }
    return 2.0 * g;
}

// what the totals are multiplied by: the reference's normalisers, known before the launch
struct PhotoScales {
    double colour, mask, patch, mse;
};
static PHOTO_DEV PhotoScales photo_scales(int kind, int rows, int patch) {
    PhotoScales s;
    const double n3 = 3.0 * (double)rows;
    s.colour = kind == PHOTO_MSE ? 1.0 / (n3 + 1e-6) : 2.0 / n3;               // :153 sum / (nelement + 1e-6); :156 mean x 2
    s.mask = 0.5 / (double)rows;                                                  // :315-316 mask_loss_strength x mean
    s.patch = patch > 0 ? 0.02 / ((double)rows * (double)(patch * patch)) : 0.0;  // :182 patch_loss_strength x the mean over rows x P^2 pairs
    s.mse = 1.0 / n3;                                                             // metrics.py:31 mean
    return s;
}
// the totals into out[5]: the two heads of a term add up (:307, :311, :318, :187)
static PHOTO_DEV void photo_outputs(const PhotoArgs& a, const double tot[PHOTO_NACC]) {
    const PhotoScales s = photo_scales(a.kind, a.rows, a.patch);
    a.out[0] = (float)(a.rgb_fine ? tot[0] * s.colour + tot[1] * s.colour : tot[0] * s.colour);
    a.out[1] = (float)(!a.fg_mask ? 0.0 : a.opacity_fine ? tot[4] * s.mask + tot[5] * s.mask : tot[4] * s.mask);
    a.out[2] = (float)(!a.patch ? 0.0 : a.depth_fine ? tot[6] * s.patch + tot[7] * s.patch : tot[6] * s.patch);
    a.out[3] = (float)(tot[2] * s.mse);
    a.out[4] = (float)(a.rgb_fine ? tot[3] * s.mse : 0.0);
}

}  // namespace sparf
