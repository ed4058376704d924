// Pose evaluation: CommonPoseEvaluation.evaluate_any_poses with prealign_w2c_small_camera_systems and
// evaluate_camera_alignment (joint_pose_nerf_trainer.py:160-311) as ONE launch, and backtrack_from_aligning_the_trajectory
// (align_trajectories.py:94-101) as another.  pose_eval.h holds the arithmetic; this file owns the staging, the candidate-per-thread
// split and the choice.  One workgroup per pose set: both pose arrays are inverted to camera-to-world once and staged as doubles in
// LDS, thread p evaluates alignment candidate p over all B poses and leaves its three scores in LDS, one thread takes the argmin in
// index order, and the chosen candidate is evaluated once more, a pose per thread, for the stores.  Doubles on the fp32 operands, one
// rounding per stored value, no atomics: the same bits from call to call.
#include <hip/hip_runtime.h>

#include "pose_eval.h"

namespace sparf {

static constexpr int PE_BLOCK = 128;           // >= PE_MAX_PAIRS + 1 (the thread of the unaligned means) and >= PE_MAX_POSES
static constexpr int PE_BACK_BLOCK = 64;
static_assert(PE_BLOCK > PE_MAX_PAIRS && PE_BLOCK >= PE_MAX_POSES, "a thread per candidate, one more, and a thread per pose");

struct PoseEvalArgs {
    const float* pose;        // [S][B][12]
    const float* pose_gt;     // [gt_sets][B][12]
    int B, n, align, gt_stride;                // n = min(B, 10) views make the candidates; gt_stride = 0 or B * 12 floats
    float *stats, *errors, *aligned, *sim3, *scores;
    int* best;
};

__global__ void __launch_bounds__(PE_BLOCK) pose_eval_kernel(PoseEvalArgs g) {
    __shared__ double c2w[PE_MAX_POSES * 12], gt_c2w[PE_MAX_POSES * 12];
    __shared__ double score[PE_MAX_PAIRS * 3], before[2];
    __shared__ int chosen;
    const int s = blockIdx.x, tid = threadIdx.x, B = g.B;
    const int P = g.align ? g.n * (g.n - 1) : 0;
    const float* pose = g.pose + (size_t)s * B * 12;
    const float* gt = g.pose_gt + (size_t)s * g.gt_stride;
    for (int i = tid; i < 2 * B; i += PE_BLOCK) {
        const int k = i < B ? i : i - B;
        double w2c[12], inv[12];
        load12((i < B ? pose : gt) + (size_t)k * 12, w2c);
        pe_invert(w2c, inv);
        double* dst = (i < B ? c2w : gt_c2w) + k * 12;
#pragma unroll
        for (int e = 0; e < 12; ++e) dst[e] = inv[e];
    }
    __syncthreads();
    if (tid < P) {
        int a, b;
        double sc[3];
        pe_pair(tid, g.n, a, b);
        pe_candidate(c2w, gt_c2w, B, a, b, sc);
        score[tid * 3] = sc[0];
        score[tid * 3 + 1] = sc[1];
        score[tid * 3 + 2] = sc[2];
    } else if (tid == PE_BLOCK - 1) {          // the means before alignment (:300-302), in index order
        double sum_R = 0.0, sum_t = 0.0;
        for (int i = 0; i < B; ++i) {
            double eR, et;
            pe_alignment_errors(c2w + i * 12, gt_c2w + i * 12, eR, et);
            sum_R += eR;
            sum_t += et;
        }
        before[0] = sum_R / (double)B * 180. / PE_PI;
        before[1] = sum_t / (double)B;
    }
    __syncthreads();
    if (tid == 0) chosen = P ? pe_choose(score + 2, P) : -1;
    __syncthreads();
    const int best = chosen;
    double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, scale = 1.0;
    if (best >= 0) {
        int a, b;
        pe_pair(best, g.n, a, b);
        pe_similarity(c2w, gt_c2w, a, b, T, scale);
    }
    if (tid < B) {
        double eR0, et0, eR1, et1;
        pe_alignment_errors(c2w + tid * 12, gt_c2w + tid * 12, eR0, et0);
        float* al_out = g.aligned + ((size_t)s * B + tid) * 12;
        if (best >= 0) {
            double al[12];
            pe_align(T, scale, c2w + tid * 12, al);
            pe_aligned_errors(al, gt_c2w + tid * 12, eR1, et1);
            store12(al_out, al);
        } else {                               // :219-223 / a bare evaluate_camera_alignment: the poses as they came
            const float* in = pose + (size_t)tid * 12;
#pragma unroll
            for (int e = 0; e < 12; ++e) al_out[e] = in[e];
            eR1 = eR0;
            et1 = et0;
        }
        float* e0 = g.errors + ((size_t)s * 2 * B + tid) * 2;
        float* e1 = e0 + (size_t)B * 2;
        e0[0] = (float)eR0;
        e0[1] = (float)et0;
        e1[0] = (float)eR1;
        e1[1] = (float)et1;
    }
    if (tid == 0) {
        float* sim = g.sim3 + (size_t)s * PE_SIM3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) sim[i * 3 + j] = (float)T[i * 4 + j];
            sim[9 + i] = (float)T[i * 4 + 3];
        }
        sim[12] = (float)scale;
        float* st = g.stats + (size_t)s * 4;
        st[0] = (float)before[0];
        st[1] = (float)before[1];
        st[2] = (float)(best >= 0 ? score[best * 3] : before[0]);
        st[3] = (float)(best >= 0 ? score[best * 3 + 1] : before[1]);
        g.best[s] = best;
    }
    if (g.scores && tid < P) {
        float* o = g.scores + ((size_t)s * PE_MAX_PAIRS + tid) * 3;
        o[0] = (float)score[tid * 3];
        o[1] = (float)score[tid * 3 + 1];
        o[2] = (float)score[tid * 3 + 2];
    }
}

// one thread per pose; sim3_stride 0: one similarity for all
__global__ void __launch_bounds__(PE_BACK_BLOCK) pose_backtrack_kernel(const float* pose_gt_w2c, int n, const float* sim3, int sim3_stride, float* out) {
    const int i = blockIdx.x * PE_BACK_BLOCK + threadIdx.x;
    if (i >= n) return;
    double p[12], sim[PE_SIM3], o[12];
    load12(pose_gt_w2c + (size_t)i * 12, p);
    const float* sp = sim3 + (size_t)i * sim3_stride;
#pragma unroll
    for (int k = 0; k < PE_SIM3; ++k) sim[k] = (double)sp[k];
    pe_backtrack(p, sim, o);
    store12(out + (size_t)i * 12, o);
}

// B in [1, PE_MAX_POSES], S > 0; align needs B >= 2 (checked by the entry point)
int launch_pose_eval(const float* pose, const float* pose_gt, int gt_sets, int S, int B, int align, float* stats, float* errors, float* aligned,
                     float* sim3, int* best, float* scores, hipStream_t s) {
    PoseEvalArgs g{pose, pose_gt, B, B < PE_MAX_VIEWS ? B : PE_MAX_VIEWS, align, gt_sets == 1 ? 0 : B * 12, stats, errors, aligned, sim3, scores, best};
    hipLaunchKernelGGL(pose_eval_kernel, dim3(S), dim3(PE_BLOCK), 0, s, g);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
int launch_pose_backtrack(const float* pose_gt_w2c, int n, const float* sim3, int sim3_stride, float* out, hipStream_t s) {
    hipLaunchKernelGGL(pose_backtrack_kernel, dim3((n + PE_BACK_BLOCK - 1) / PE_BACK_BLOCK), dim3(PE_BACK_BLOCK), 0, s, pose_gt_w2c, n, sim3, sim3_stride, out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace sparf
