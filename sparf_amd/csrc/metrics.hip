// Evaluation metrics: compute_metrics / compute_metrics_masked / compute_depth_error (metrics.py:136-268) with the SSIM
// of third_party/pytorch_ssim/ssim.py as one call for one or two predicted images against one ground truth.  The arithmetic of a pixel is
// metrics.h's; this file owns the tiles, the two window passes, the reductions and the entry point.
//
// A workgroup owns one tile of METRICS_TH x METRICS_TW output pixels of one image.  For each channel, and with a mask once more for the
// composited images, it stages the tile with its 5-pixel halo of ground truth, prediction and fine prediction as one float4 per pixel
// (zero outside the image: the reference's padding, which follows the composite), runs the 11 taps along the rows into LDS for the
// moment maps x, x^2 of the ground truth and y, y^2, x y of each head -- the ground truth's two are computed once for both heads -- and
// then along the columns.  The reference's stored window is the float product fl(w_i w_j), not w w^T: the column pass adds the difference
// over the 121 staged pixels of an output (metrics.h metrics_residual), without which a mean SSIM near 0 lies several fp32 spacings off.  LDS: 26 x 42 float4 = 17 472 B staged, 8 maps x 26 x 32 doubles = 53 248 B of row sums (5 maps = 33 280 B
// with one head), 576 B for the reduction: 71 296 B, two workgroups per CU.  The row pass reads one ds_read_b128 per tap, consecutive
// lanes consecutive 16-byte slots; the column pass reads ds_read_b64, a half wave one bank row of 32 consecutive doubles: no conflict.
// Sums follow photo.hip and dcons.hip: a thread adds its pixels in index order, a wave its lanes by an xor butterfly, the waves in wave
// order, the tiles in tile order in a second launch that reads the workspace.  No atomic, no host synchronisation, no readback.
#include <hip/hip_runtime.h>

#include "../../include/sparf_hip.h"
#include "metrics.h"

namespace sparf {

static constexpr int METRICS_WAVES = METRICS_BLOCK / 64;

static __device__ __forceinline__ float metrics_pixel(const float* image, const MetricsImage& im, int c, int y, int x) {      // image = im.p + b im.sb
    return image[(int64_t)c * im.sc + (int64_t)y * im.sy + (int64_t)x * im.sx];
}

template <int HEADS>
__global__ void __launch_bounds__(METRICS_BLOCK) image_metrics_tile_kernel(MetricsArgs a) {
    constexpr int MAPS = 2 + 3 * HEADS;                   // x, x^2; per head y, y^2, x y
    __shared__ float4 in[METRICS_SH * METRICS_SW];        // (ground truth, prediction, fine prediction, -) of a pixel
    __shared__ double rows[MAPS][METRICS_SH][METRICS_TW];
    __shared__ double red[METRICS_WAVES][METRICS_NACC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int tile = blockIdx.x;
    const int tx = tile % a.tiles_x;
    tile /= a.tiles_x;
    const int ty = tile % a.tiles_y, b = tile / a.tiles_y;
    const int y0 = ty * METRICS_TH, x0 = tx * METRICS_TW;
    // this image of every operand (the batch strides are dead after this)
    const float *gt = a.gt.p + (int64_t)b * a.gt.sb, *pred = a.pred.p + (int64_t)b * a.pred.sb, *fine = HEADS == 2 ? a.fine.p + (int64_t)b * a.fine.sb : nullptr;
    const unsigned char* mask = a.mask ? a.mask + (int64_t)b * a.mask_sb : nullptr;
    double w[METRICS_K];
#pragma unroll
    for (int k = 0; k < METRICS_K; ++k) w[k] = metrics_weight(k);
    double acc[METRICS_NACC];
#pragma unroll
    for (int j = 0; j < METRICS_NACC; ++j) acc[j] = 0.0;

    const int variants = a.mask ? 2 : 1;                 // 0: the images; 1: their composites with the mask
    for (int v = 0; v < variants; ++v) {
        for (int c = 0; c < 3; ++c) {
            for (int i = tid; i < METRICS_SH * METRICS_SW; i += METRICS_BLOCK) {
                const int sy = i / METRICS_SW, sx = i - sy * METRICS_SW;
                const int y = y0 - METRICS_R + sy, x = x0 - METRICS_R + sx;
                float4 px = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
                    px.x = metrics_pixel(gt, a.gt, c, y, x);
                    px.y = metrics_pixel(pred, a.pred, c, y, x);
                    if (HEADS == 2) px.z = metrics_pixel(fine, a.fine, c, y, x);
                    if (v) {
                        const double m = mask[(int64_t)y * a.mask_sy + (int64_t)x * a.mask_sx] ? 1.0 : 0.0;
                        px.x = (float)metrics_composite((double)px.x, m);
                        px.y = (float)metrics_composite((double)px.y, m);
                        if (HEADS == 2) px.z = (float)metrics_composite((double)px.z, m);
                    }
                }
                in[i] = px;
            }
            __syncthreads();
            for (int i = tid; i < METRICS_SH * METRICS_TW; i += METRICS_BLOCK) {
                const int r = i / METRICS_TW, x = i - r * METRICS_TW;
                double s[MAPS];
#pragma unroll
                for (int m = 0; m < MAPS; ++m) s[m] = 0.0;
#pragma unroll
                for (int k = 0; k < METRICS_K; ++k) {
                    const float4 px = in[r * METRICS_SW + x + k];
                    const double g = (double)px.x, p = (double)px.y;
                    s[0] += w[k] * g;
                    s[1] += w[k] * (g * g);
                    s[2] += w[k] * p;
                    s[3] += w[k] * (p * p);
                    s[4] += w[k] * (p * g);
                    if (HEADS == 2) {
                        const double f = (double)px.z;
                        s[5] += w[k] * f;
                        s[6] += w[k] * (f * f);
                        s[7] += w[k] * (f * g);
                    }
                }
#pragma unroll
                for (int m = 0; m < MAPS; ++m) rows[m][r][x] = s[m];
            }
            __syncthreads();
            double ssim[HEADS], sq_err[HEADS];           // this channel's sums of the thread (no array is indexed by v: registers)
#pragma unroll
            for (int h = 0; h < HEADS; ++h) ssim[h] = sq_err[h] = 0.0;
            for (int i = tid; i < METRICS_TH * METRICS_TW; i += METRICS_BLOCK) {
                const int y = i / METRICS_TW, x = i - y * METRICS_TW;
                if (y0 + y >= a.H || x0 + x >= a.W) continue;
                double s[MAPS];
#pragma unroll
                for (int m = 0; m < MAPS; ++m) s[m] = 0.0;
#pragma unroll
                for (int k = 0; k < METRICS_K; ++k)
#pragma unroll
                    for (int m = 0; m < MAPS; ++m) s[m] += w[k] * rows[m][y + k][x];
                // what the stored 2-D float window holds beyond w w^T (metrics.h metrics_residual): 121 taps on the staged pixels
                float q[MAPS];
#pragma unroll
                for (int m = 0; m < MAPS; ++m) q[m] = 0.0f;
#pragma unroll
                for (int ki = 0; ki < METRICS_K; ++ki) {
#pragma unroll
                    for (int kj = 0; kj < METRICS_K; ++kj) {
                        const float4 t = in[(y + ki) * METRICS_SW + x + kj];
                        const float d = metrics_residual(ki, kj);
                        q[0] += d * t.x;
                        q[1] += d * (t.x * t.x);
                        q[2] += d * t.y;
                        q[3] += d * (t.y * t.y);
                        q[4] += d * (t.y * t.x);
                        if (HEADS == 2) {
                            q[5] += d * t.z;
                            q[6] += d * (t.z * t.z);
                            q[7] += d * (t.z * t.x);
                        }
                    }
                }
#pragma unroll
                for (int m = 0; m < MAPS; ++m) s[m] += (double)q[m];
                const float4 px = in[(y + METRICS_R) * METRICS_SW + x + METRICS_R];
#pragma unroll
                for (int h = 0; h < HEADS; ++h) {
                    const double e = (double)(h ? px.z : px.y) - (double)px.x;      // composites: 1 - 1 = 0 outside the foreground
                    ssim[h] += metrics_ssim(s[2 + 3 * h], s[0], s[3 + 3 * h], s[1], s[4 + 3 * h]);
                    sq_err[h] += e * e;
                }
                if (c != 0) continue;
                if (v) {
                    if (mask[(int64_t)(y0 + y) * a.mask_sy + (int64_t)(x0 + x) * a.mask_sx]) acc[2 * METRICS_HEAD_ACC] += 1.0;
                } else if (a.depth_gt.p) {
                    const int64_t pix = (int64_t)(y0 + y) * a.W + (x0 + x);
                    if (a.valid.p && !((const unsigned char*)a.valid.p)[(int64_t)b * a.valid.sb + pix * a.valid.sx]) continue;
                    acc[2 * METRICS_HEAD_ACC + 1] += 1.0;
                    const double gt = (double)((const float*)a.depth_gt.p)[(int64_t)b * a.depth_gt.sb + pix * a.depth_gt.sx];
#pragma unroll
                    for (int h = 0; h < HEADS; ++h) {
                        const MetricsRows& d = h ? a.depth_fine : a.depth;
                        if (!d.p) continue;
                        const double pred = (double)((const float*)d.p)[(int64_t)b * d.sb + pix * d.sx];
                        double sq;
                        acc[h * METRICS_HEAD_ACC + 4] += metrics_depth(gt, pred, 1.0, sq);
                        acc[h * METRICS_HEAD_ACC + 5] += sq;
                        acc[h * METRICS_HEAD_ACC + 6] += metrics_depth(gt, pred, (double)a.scale, sq);
                        acc[h * METRICS_HEAD_ACC + 7] += sq;
                    }
                }
            }
#pragma unroll
            for (int h = 0; h < HEADS; ++h) {
                if (v) {
                    acc[h * METRICS_HEAD_ACC + 2] += ssim[h];
                    acc[h * METRICS_HEAD_ACC + 3] += sq_err[h];
                } else {
                    acc[h * METRICS_HEAD_ACC + 0] += ssim[h];
                    acc[h * METRICS_HEAD_ACC + 1] += sq_err[h];
                }
            }
            __syncthreads();                             // (the next channel's staging overwrites what the column pass read)
        }
    }

    // the tile's totals: wave butterfly, then the waves in order
#pragma unroll
    for (int j = 0; j < METRICS_NACC; ++j) {
        double t = acc[j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d);
        if (lane == 0) red[wave][j] = t;
    }
    __syncthreads();
    if (tid < METRICS_NACC) {
        double t = red[0][tid];
#pragma unroll
        for (int k = 1; k < METRICS_WAVES; ++k) t += red[k][tid];
        a.ws[(size_t)blockIdx.x * METRICS_NACC + tid] = t;
    }
}

// the partial totals added in tile order (lane j owns total j), then the outputs
__global__ void __launch_bounds__(64) image_metrics_finish_kernel(MetricsArgs a, int tiles) {
    __shared__ double tot[METRICS_NACC];
    const int j = threadIdx.x;
    if (j < METRICS_NACC) {
        double t = 0.0;
        for (int i = 0; i < tiles; ++i) t += a.ws[(size_t)i * METRICS_NACC + j];
        tot[j] = t;
    }
    __syncthreads();
    if (j == 0) metrics_outputs(a, tot);
}

static int launch_image_metrics(const MetricsArgs& a, hipStream_t s) {
    const int tiles = a.B * a.tiles_y * a.tiles_x;
    if (a.fine.p)
        hipLaunchKernelGGL(image_metrics_tile_kernel<2>, dim3(tiles), dim3(METRICS_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL(image_metrics_tile_kernel<1>, dim3(tiles), dim3(METRICS_BLOCK), 0, s, a);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(image_metrics_finish_kernel, dim3(1), dim3(64), 0, s, a, tiles);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace sparf

using namespace sparf;

// ---- the entry points (sparf_hip.h): every argument check comes before any HIP call
static const int64_t kMetricsMaxPixels = (int64_t)1 << 30;

static int64_t metrics_tiles(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || (int64_t)B * H * W > kMetricsMaxPixels) return 0;
    return (int64_t)B * ((H + METRICS_TH - 1) / METRICS_TH) * ((W + METRICS_TW - 1) / METRICS_TW);
}

int64_t sparf_image_metrics_workspace_bytes(int B, int H, int W) { return metrics_tiles(B, H, W) * METRICS_NACC * (int64_t)sizeof(double); }

static bool metrics_strides_ok(const int64_t* s, int n) {
    for (int i = 0; i < n; ++i)
        if (s[i] < 0) return false;
    return true;
}

int sparf_image_metrics(const sparf_image_metrics_t* m, void* stream) {
    if (!m) return 1;
    const int64_t need = sparf_image_metrics_workspace_bytes(m->B, m->H, m->W);
    if (need == 0 || !m->pred || !m->gt || !m->out || !m->counts || !m->workspace || m->workspace_bytes < need) return 1;
    if ((m->depth || m->depth_fine) && !m->depth_gt) return 1;
    if (m->depth_fine && !m->pred_fine) return 1;
    if (!metrics_strides_ok(m->pred_stride, 4) || !metrics_strides_ok(m->gt_stride, 4) || (m->pred_fine && !metrics_strides_ok(m->pred_fine_stride, 4)) ||
        (m->fg_mask && !metrics_strides_ok(m->fg_mask_stride, 3)) || (m->depth && !metrics_strides_ok(m->depth_stride, 2)) ||
        (m->depth_fine && !metrics_strides_ok(m->depth_fine_stride, 2)) || (m->depth_gt && !metrics_strides_ok(m->depth_gt_stride, 2)) ||
        (m->valid_depth_gt && !metrics_strides_ok(m->valid_depth_gt_stride, 2)))
        return 1;
    MetricsArgs a{};
    a.B = m->B; a.H = m->H; a.W = m->W;
    a.tiles_y = (m->H + METRICS_TH - 1) / METRICS_TH;
    a.tiles_x = (m->W + METRICS_TW - 1) / METRICS_TW;
    a.pred = MetricsImage{m->pred, m->pred_stride[0], m->pred_stride[1], m->pred_stride[2], m->pred_stride[3]};
    if (m->pred_fine) a.fine = MetricsImage{m->pred_fine, m->pred_fine_stride[0], m->pred_fine_stride[1], m->pred_fine_stride[2], m->pred_fine_stride[3]};
    a.gt = MetricsImage{m->gt, m->gt_stride[0], m->gt_stride[1], m->gt_stride[2], m->gt_stride[3]};
    if (m->fg_mask) {
        a.mask = m->fg_mask;
        a.mask_sb = m->fg_mask_stride[0]; a.mask_sy = m->fg_mask_stride[1]; a.mask_sx = m->fg_mask_stride[2];
    }
    if (m->depth) a.depth = MetricsRows{m->depth, m->depth_stride[0], m->depth_stride[1]};
    if (m->depth_fine) a.depth_fine = MetricsRows{m->depth_fine, m->depth_fine_stride[0], m->depth_fine_stride[1]};
    if (m->depth_gt) a.depth_gt = MetricsRows{m->depth_gt, m->depth_gt_stride[0], m->depth_gt_stride[1]};
    if (m->depth_gt && m->valid_depth_gt) a.valid = MetricsRows{m->valid_depth_gt, m->valid_depth_gt_stride[0], m->valid_depth_gt_stride[1]};
    a.scale = m->depth_scale;
    a.out = m->out; a.counts = m->counts; a.ws = (double*)m->workspace;
    return launch_image_metrics(a, (hipStream_t)stream);
}
