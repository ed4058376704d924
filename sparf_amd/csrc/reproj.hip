// Correspondence loss: the re-projection terms of one view pair -- one term i -> j, or the two / four terms of
// corres_loss.py:183-219 with both pose compositions -- with the loss, the stats, the valid mask and every gradient seed from one call.
// The arithmetic of a match, of a term's totals and of the compositions is reproj.h's; this file owns the loops, the reductions and the entry points.
//
// Reductions are fixed-order and use no atomics (ordered.h: block_totals, sum_parts); above REPROJ_SINGLE_MAX matches the workgroups'
// partial totals are added in workgroup order.  The normaliser 1 / (#valid + 1e-6) is known only after the count, so a
// term is evaluated twice: once for its totals, once -- with the scale in hand -- for the seeds, each of which is then a double
// product rounded once.  Up to REPROJ_SINGLE_MAX matches one workgroup does all of it in one launch; above, a totals launch and a
// seeds launch, REPROJ_PARTS workgroups per term.  No host synchronisation, no readback.
#include <hip/hip_runtime.h>

#include "../../include/sparf_hip.h"
#include "ordered.h"
#include "reproj.h"

namespace sparf {

static constexpr int REPROJ_WAVES = REPROJ_BLOCK / 64;

// the totals of a workgroup, in every thread
static REPROJ_DEV void reproj_block_totals(const double acc[REPROJ_NACC], double (*red)[REPROJ_NACC], double tot[REPROJ_NACC]) {
    block_totals<REPROJ_NACC, REPROJ_WAVES>(acc, red, tot);
    __syncthreads();                         // red is written again by the next term
}

// the matches first, first + stride, ... < n of term t into acc; term 0 also leaves the valid mask
static REPROJ_DEV void reproj_totals_loop(const ReprojArgs& a, int t, const ReprojSetup& s, int first, int stride, double acc[REPROJ_NACC]) {
    const ReprojTerm& term = a.term[t];
    const double *Kinv = s.Kinv[term.cam_i], *Kj = s.K[term.cam_j], *T = s.T[term.tf];
#pragma unroll
    for (int j = 0; j < REPROJ_NACC; ++j) acc[j] = 0.0;
    for (int k = first; k < a.n; k += stride) {
        ReprojMatch m;
        reproj_match(a, term, Kinv, Kj, T, k, m);
        reproj_accumulate(m, (double)term.depth_i[k], acc);
        if (t == 0 && a.valid) a.valid[k] = (m.vpix && m.vdepth) ? 1 : 0;
    }
}

static REPROJ_DEV void reproj_seeds_loop(const ReprojArgs& a, int t, const ReprojSetup& s, double scale, int first, int stride) {
    const ReprojTerm& term = a.term[t];
    if (!term.d_depth_i) return;
    const double *Kinv = s.Kinv[term.cam_i], *Kj = s.K[term.cam_j], *T = s.T[term.tf];
    for (int k = first; k < a.n; k += stride) {
        ReprojMatch m;
        reproj_match(a, term, Kinv, Kj, T, k, m);
        term.d_depth_i[k] = (float)(m.gd * scale);
    }
}

// n <= REPROJ_SINGLE_MAX (or no workspace): one workgroup, every term in turn
__global__ void __launch_bounds__(REPROJ_BLOCK) reproj_single_kernel(ReprojArgs a) {
    __shared__ ReprojSetup s;
    __shared__ ReprojFinal f;
    __shared__ double red[REPROJ_WAVES][REPROJ_NACC];
    if (threadIdx.x == 0) {
        reproj_setup(a, s);
        reproj_final_init(f);
    }
    __syncthreads();
    for (int t = 0; t < a.nterms; ++t) {
        double acc[REPROJ_NACC], tot[REPROJ_NACC];
        reproj_totals_loop(a, t, s, threadIdx.x, REPROJ_BLOCK, acc);
        reproj_block_totals(acc, red, tot);
        if (threadIdx.x == 0) reproj_term_finish(a, t, tot, f);
        reproj_seeds_loop(a, t, s, reproj_scale(a, tot), threadIdx.x, REPROJ_BLOCK);
    }
    if (threadIdx.x == 0) reproj_outputs(a, s, f);
}

// n > REPROJ_SINGLE_MAX, grid (parts, nterms): workgroup b of term t leaves its totals at ws[t][b]
__global__ void __launch_bounds__(REPROJ_BLOCK) reproj_partial_kernel(ReprojArgs a) {
    __shared__ ReprojSetup s;
    __shared__ double red[REPROJ_WAVES][REPROJ_NACC];
    if (threadIdx.x == 0) reproj_setup(a, s);
    __syncthreads();
    const int t = blockIdx.y;
    double acc[REPROJ_NACC], tot[REPROJ_NACC];
    reproj_totals_loop(a, t, s, blockIdx.x * REPROJ_BLOCK + threadIdx.x, gridDim.x * REPROJ_BLOCK, acc);
    reproj_block_totals(acc, red, tot);
    if (threadIdx.x == 0) {
        double* o = a.ws + ((size_t)t * REPROJ_PARTS + blockIdx.x) * REPROJ_NACC;
#pragma unroll
        for (int j = 0; j < REPROJ_NACC; ++j) o[j] = tot[j];
    }
}

// the partial totals of term t, ws[t][REPROJ_PARTS], added in workgroup order
static REPROJ_DEV void reproj_sum_parts(const double* ws, int t, int parts, double tot[REPROJ_NACC]) {
    sum_parts<REPROJ_NACC>(ws + (size_t)t * REPROJ_PARTS * REPROJ_NACC, parts, tot);
}

// same grid: every workgroup adds the partials of its term (the same sum in the same order everywhere) and writes its share of the
// seeds; workgroup (0, 0) also goes through every term for the outputs
__global__ void __launch_bounds__(REPROJ_BLOCK) reproj_seeds_kernel(ReprojArgs a) {
    __shared__ ReprojSetup s;
    __shared__ ReprojFinal f;
    if (threadIdx.x == 0) reproj_setup(a, s);
    __syncthreads();
    const int t = blockIdx.y;
    double tot[REPROJ_NACC];
    reproj_sum_parts(a.ws, t, gridDim.x, tot);
    reproj_seeds_loop(a, t, s, reproj_scale(a, tot), blockIdx.x * REPROJ_BLOCK + threadIdx.x, gridDim.x * REPROJ_BLOCK);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        reproj_final_init(f);
        for (int u = 0; u < a.nterms; ++u) {
            reproj_sum_parts(a.ws, u, gridDim.x, tot);
            reproj_term_finish(a, u, tot, f);
        }
        reproj_outputs(a, s, f);
    }
}

// n > 0
static int launch_reproj(const ReprojArgs& a, hipStream_t s) {
    if (a.n <= REPROJ_SINGLE_MAX || !a.ws) {
        hipLaunchKernelGGL(reproj_single_kernel, dim3(1), dim3(REPROJ_BLOCK), 0, s, a);
        return launched();
    }
    int parts = (a.n + 4 * REPROJ_BLOCK - 1) / (4 * REPROJ_BLOCK);
    if (parts > REPROJ_PARTS) parts = REPROJ_PARTS;
    hipLaunchKernelGGL(reproj_partial_kernel, dim3(parts, a.nterms), dim3(REPROJ_BLOCK), 0, s, a);
    if (launched()) return 2;
    hipLaunchKernelGGL(reproj_seeds_kernel, dim3(parts, a.nterms), dim3(REPROJ_BLOCK), 0, s, a);
    return launched();
}

}  // namespace sparf

using namespace sparf;

// ---- the entry points (sparf_hip.h): every argument check comes before any HIP call; n == 0 launches no kernel
static inline bool reproj_opts_ok(int n, int loss_type, const float* out) {
    return n >= 0 && n <= (1 << 30) && loss_type >= 0 && loss_type < REPROJ_LOSS_TYPES && out;
}
static int reproj_zero(float* p, int floats, hipStream_t s) {
    return !p || hipMemsetAsync(p, 0, (size_t)floats * sizeof(float), s) == hipSuccess ? 0 : 2;
}
int64_t sparf_reproj_workspace_bytes(int n) {
    return n > REPROJ_SINGLE_MAX ? (int64_t)REPROJ_MAX_TERMS * REPROJ_PARTS * REPROJ_NACC * (int64_t)sizeof(double) : 0;
}
// corres_loss.py:50-95 compute_render_and_repro_loss_w_repro_thres: batched_geometry_utils.py:199-228 batch_project_to_other_img,
// the two detached checks, base_losses.py:197-224 compute_diff_loss -- and what autograd derives from them for depth_i and T
int sparf_reproj_loss(const float* pixels_i, const float* depth_i, const float* K_i, const float* pixels_j, const float* depth_j,
                      const float* K_j, const float* T_itoj, const float* weights, int n, int loss_type, int pix_check, float pix_thresh,
                      int depth_check, float depth_thresh, float* out, float* d_depth_i, float* d_T, unsigned char* valid, void* workspace,
                      void* stream) {
    if (!reproj_opts_ok(n, loss_type, out) || (depth_check && !depth_j)) return 1;
    if (n > 0 && (!pixels_i || !depth_i || !K_i || !pixels_j || !K_j || !T_itoj)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return reproj_zero(out, 4, s) | reproj_zero(d_T, 16, s);
    ReprojArgs a{};
    a.n = n; a.nterms = 1; a.loss_type = loss_type; a.pix_check = pix_check != 0; a.depth_check = depth_check != 0; a.pair = 0;
    a.pix_thresh = pix_thresh; a.depth_thresh = depth_thresh;
    a.K[0] = K_i; a.K[1] = K_j; a.T = T_itoj; a.weights = weights;
    a.term[0] = ReprojTerm{pixels_i, depth_i, pixels_j, depth_j, d_depth_i, 0, 1, 0};
    a.out = out; a.valid = valid; a.d_T = d_T; a.ws = (double*)workspace;
    return launch_reproj(a, s);
}
// corres_loss.py:183-219 of compute_loss_on_image_pair: T_self2other = P_other pose_inverse_4x4(P_self) (camera.py:37-61), its inverse,
// the two (four with depth_fine) terms, their mean, stats_dict as that call order leaves it -- and the gradients to every depth and
// to both poses
int sparf_reproj_pair_loss(const float* pixels_self, const float* pixels_other, const float* depth_self, const float* depth_other,
                           const float* depth_fine_self, const float* depth_fine_other, const float* K_self, const float* K_other,
                           const float* pose_self, const float* pose_other, const float* weights, int n, int loss_type, int pix_check,
                           float pix_thresh, int depth_check, float depth_thresh, float* out, float* d_depth_self, float* d_depth_other,
                           float* d_depth_fine_self, float* d_depth_fine_other, float* d_pose_self, float* d_pose_other, void* workspace,
                           void* stream) {
    if (!reproj_opts_ok(n, loss_type, out)) return 1;
    if ((depth_fine_self != nullptr) != (depth_fine_other != nullptr)) return 1;
    if (!depth_fine_self && (d_depth_fine_self || d_depth_fine_other)) return 1;
    if (n > 0 && (!pixels_self || !pixels_other || !depth_self || !depth_other || !K_self || !K_other || !pose_self || !pose_other)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return reproj_zero(out, 4, s) | reproj_zero(d_pose_self, 12, s) | reproj_zero(d_pose_other, 12, s);
    ReprojArgs a{};
    a.n = n; a.nterms = depth_fine_self ? 4 : 2; a.loss_type = loss_type; a.pix_check = pix_check != 0; a.depth_check = depth_check != 0; a.pair = 1;
    a.pix_thresh = pix_thresh; a.depth_thresh = depth_thresh;
    a.K[0] = K_self; a.K[1] = K_other; a.pose[0] = pose_self; a.pose[1] = pose_other; a.weights = weights;
    a.term[0] = ReprojTerm{pixels_self, depth_self, pixels_other, depth_other, d_depth_self, 0, 1, 0};
    a.term[1] = ReprojTerm{pixels_other, depth_other, pixels_self, depth_self, d_depth_other, 1, 0, 1};
    a.term[2] = ReprojTerm{pixels_self, depth_fine_self, pixels_other, depth_fine_other, d_depth_fine_self, 0, 1, 0};
    a.term[3] = ReprojTerm{pixels_other, depth_fine_other, pixels_self, depth_fine_self, d_depth_fine_other, 1, 0, 1};
    a.out = out; a.d_pose[0] = d_pose_self; a.d_pose[1] = d_pose_other; a.ws = (double*)workspace;
    return launch_reproj(a, s);
}
