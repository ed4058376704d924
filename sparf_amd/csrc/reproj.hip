// Correspondence loss: the re-projection terms of one view pair -- one term i -> j, or the two / four terms of
// corres_loss.py:183-219 with both pose compositions -- with the loss, the stats, the valid mask and every gradient seed from one call.
// The arithmetic of a match, of a term's totals and of the compositions is reproj.h's; this file owns the loops and the reductions.
//
// Reductions are fixed-order and use no atomics (ordered.h: block_totals, sum_parts); above REPROJ_SINGLE_MAX matches the workgroups'
// partial totals are added in workgroup order.  The normaliser 1 / (#valid + 1e-6) is known only after the count, so a
// term is evaluated twice: once for its totals, once -- with the scale in hand -- for the seeds, each of which is then a double
// product rounded once.  Up to REPROJ_SINGLE_MAX matches one workgroup does all of it in one launch; above, a totals launch and a
// seeds launch, REPROJ_PARTS workgroups per term.  No host synchronisation, no readback.
#include <hip/hip_runtime.h>

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

int64_t reproj_workspace_bytes(int n) {
    return n > REPROJ_SINGLE_MAX ? (int64_t)REPROJ_MAX_TERMS * REPROJ_PARTS * REPROJ_NACC * (int64_t)sizeof(double) : 0;
}

// n > 0
int launch_reproj(const ReprojArgs& a, hipStream_t s) {
    if (a.n <= REPROJ_SINGLE_MAX || !a.ws) {
        hipLaunchKernelGGL(reproj_single_kernel, dim3(1), dim3(REPROJ_BLOCK), 0, s, a);
        return hipGetLastError() == hipSuccess ? 0 : 2;
    }
    int parts = (a.n + 4 * REPROJ_BLOCK - 1) / (4 * REPROJ_BLOCK);
    if (parts > REPROJ_PARTS) parts = REPROJ_PARTS;
    hipLaunchKernelGGL(reproj_partial_kernel, dim3(parts, a.nterms), dim3(REPROJ_BLOCK), 0, s, a);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(reproj_seeds_kernel, dim3(parts, a.nterms), dim3(REPROJ_BLOCK), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace sparf
