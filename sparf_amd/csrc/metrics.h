// Evaluation metrics: the arguments of the kernels of metrics.hip and the arithmetic of compute_metrics /
// compute_metrics_masked / compute_depth_error (metrics.py:136-268) and of the SSIM they call (third_party/pytorch_ssim/ssim.py:8-38) as
// plain functions of doubles.  Every value is taken to double as it is loaded and each result is rounded to float once, on its store (the
// contract of photo.h).  Nothing here touches a thread index, LDS or a HIP call: the functions state the mathematics of ONE pixel and of
// the outputs; metrics.hip owns the tiles, the window passes and the reductions.
// The file also compiles as plain C++ (tools/metrics_host_check.cpp evaluates it on the host under the sanitizers).
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef METRICS_DEV
#ifdef __HIPCC__
#define METRICS_DEV __host__ __device__ __forceinline__
#else
#define METRICS_DEV inline
#endif
#endif

namespace sparf {

enum {
    METRICS_K = 11,              // the window: 11 taps, sigma 1.5, zero padding of METRICS_R pixels (ssim.py:19, :41)
    METRICS_R = 5,
    METRICS_TH = 16,             // a workgroup's tile of output pixels: 16 rows of 32 (a half wave reads one LDS bank row of doubles)
    METRICS_TW = 32,
    METRICS_SH = METRICS_TH + 2 * METRICS_R,             // the tile with its halo: 26 x 42
    METRICS_SW = METRICS_TW + 2 * METRICS_R,
    METRICS_BLOCK = 256,         // four waves, one per SIMD
    METRICS_HEADS = 2,
    METRICS_OUTS = 10,           // out[head]: mse, psnr, ssim, mse_masked, psnr_masked, ssim_masked, abs_e, rmse, abs_e_scaled, rmse_scaled
    // totals of a head: [0] sum SSIM, [1] sum e^2, [2] sum masked SSIM, [3] sum e^2 over foreground elements, [4] sum |e_depth| at scale 1,
    // [5] sum e_depth^2 at scale 1, [6] and [7] the same at the given scale
    METRICS_HEAD_ACC = 8,
    // a tile's totals: the two heads, then [16] foreground pixels, [17] valid depth pixels (whole numbers below 2^31: exact)
    METRICS_NACC = 2 * METRICS_HEAD_ACC + 2,
};

// gaussian(11, 1.5) of ssim.py:8-10: exp() of a Python double rounded to float, divided in float by their float sum
static METRICS_DEV double metrics_weight(int k) {
    const float window[METRICS_K] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                     0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
    return (double)window[k];
}
// create_window of ssim.py:12-16 stores the 2-D window as the FLOAT products fl(w_i w_j), which is not the rank-one w w^T that two
// separable passes in double apply: the two differ by up to 2^-25 of a weight, the same way at every pixel, and that shows as several fp32
// spacings of a mean SSIM near 0 (uncorrelated images: sigma12 is a difference of two numbers near 0.25).  The kernel therefore adds what
// the separable passes leave out, sum_ij residual(i, j) x[i][j]; the residual is below 2^-25 of the moment, so float arithmetic on it
// costs less than 2^-48 of the moment.
static METRICS_DEV float metrics_window_2d(int i, int j) {
    const float wi = (float)metrics_weight(i), wj = (float)metrics_weight(j);
    const float w2 = wi * wj;
    return w2;
}
static METRICS_DEV float metrics_residual(int i, int j) {
    return (float)((double)metrics_window_2d(i, j) - metrics_weight(i) * metrics_weight(j));
}

struct MetricsImage {            // [B][3][H][W] read in place by element strides
    const float* p;
    int64_t sb, sc, sy, sx;
};
struct MetricsRows {             // [B][H W] floats or bytes, read in place
    const void* p;
    int64_t sb, sx;
};
struct MetricsArgs {
    int B, H, W, tiles_y, tiles_x;
    MetricsImage pred, fine, gt;                         // fine.p null: one head
    const unsigned char* mask;                           // [B][H][W] by mask_sb / sy / sx, or null
    int64_t mask_sb, mask_sy, mask_sx;
    MetricsRows depth, depth_fine, depth_gt, valid;      // null each; valid null with depth_gt: every pixel is valid
    float scale;
    float* out;                                          // [METRICS_HEADS][METRICS_OUTS]
    int32_t* counts;                                     // [2]: foreground pixels, valid depth pixels
    double* ws;                                          // [tiles][METRICS_NACC]
};

// ssim.py:22-33 on the five windowed moments of one pixel: mu1 = E x, mu2 = E y, e11 = E x^2, e22 = E y^2, e12 = E x y.  Written in the
// reference's order (each square and product a value of its own), so that x == y gives numerator == denominator and exactly 1.
static METRICS_DEV double metrics_ssim(double mu1, double mu2, double e11, double e22, double e12) {
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double mu1_sq = mu1 * mu1;
    const double mu2_sq = mu2 * mu2;
    const double mu1_mu2 = mu1 * mu2;
    const double sigma1_sq = e11 - mu1_sq;
    const double sigma2_sq = e22 - mu2_sq;
    const double sigma12 = e12 - mu1_mu2;
    const double num_l = 2.0 * mu1_mu2 + C1, num_c = 2.0 * sigma12 + C2;
    const double den_l = mu1_sq + mu2_sq + C1, den_c = sigma1_sq + sigma2_sq + C2;
    const double num = num_l * num_c;
    const double den = den_l * den_c;
    return num / den;
}

// metrics.py:208-209 for a binary mask m in {0, 1}: x m + (1 - m), which is x or 1 exactly
static METRICS_DEV double metrics_composite(double x, double m) {
    const double xm = x * m;
    return xm + (1.0 - m);
}

// metrics.py:160, :79 on one valid pixel: e = gt - s pred;  -> |e|, and e^2 in sq
static METRICS_DEV double metrics_depth(double gt, double pred, double s, double& sq) {
    const double sp = s * pred;
    const double e = gt - sp;
    sq = e * e;
    return fabs(e);
}

// the finishing arithmetic.  n = 0: mse 0/0 = NaN (torch's mean of an empty selection), psnr NaN; mse = 0: psnr +inf
static METRICS_DEV double metrics_mse(double sum, double n) { return sum / n; }
static METRICS_DEV double metrics_psnr(double mse) { return -10.0 * log10(mse); }
static METRICS_DEV double metrics_abs_e(double sum, double n) { return sum / (n + 1e-6); }              // metrics.py:161: 0 for n = 0
static METRICS_DEV double metrics_rmse(double sum, double n) { return sqrt(sum / n); }                  // metrics.py:79: NaN for n = 0

// the totals of all tiles into out[2][10] and counts[2]; what was not asked for is NaN (metrics.py:250 for the depth errors)
static METRICS_DEV void metrics_outputs(const MetricsArgs& a, const double tot[METRICS_NACC]) {
    const double nan = (double)NAN;
    const double n = 3.0 * (double)a.B * (double)a.H * (double)a.W;      // ssim_map.mean(), loss.mean(): every element of the batch
    const double nfg = tot[2 * METRICS_HEAD_ACC], nvalid = tot[2 * METRICS_HEAD_ACC + 1];
    for (int h = 0; h < METRICS_HEADS; ++h) {
        const double* t = tot + h * METRICS_HEAD_ACC;
        float* o = a.out + h * METRICS_OUTS;
        const bool head = h == 0 || a.fine.p, masked = head && a.mask, depth = head && (h == 0 ? a.depth.p : a.depth_fine.p);
        const double mse = head ? metrics_mse(t[1], n) : nan;
        const double mse_m = masked ? metrics_mse(t[3], 3.0 * nfg) : nan;
        o[0] = (float)mse;
        o[1] = (float)(head ? metrics_psnr(mse) : nan);
        o[2] = (float)(head ? t[0] / n : nan);
        o[3] = (float)mse_m;
        o[4] = (float)(masked ? metrics_psnr(mse_m) : nan);
        o[5] = (float)(masked ? t[2] / n : nan);
        o[6] = (float)(depth ? metrics_abs_e(t[4], nvalid) : nan);
        o[7] = (float)(depth ? metrics_rmse(t[5], nvalid) : nan);
        o[8] = (float)(depth ? metrics_abs_e(t[6], nvalid) : nan);
        o[9] = (float)(depth ? metrics_rmse(t[7], nvalid) : nan);
    }
    a.counts[0] = (int32_t)nfg;
    a.counts[1] = (int32_t)nvalid;
}

}  // namespace sparf
