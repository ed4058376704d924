// Pose evaluation: the arithmetic of CommonPoseEvaluation's small-system alignment and of the trajectory backtrack
// (joint_pose_nerf_trainer.py:160-311, camera.py:466-471, align_trajectories.py:94-101) as plain functions of doubles: a pose is 12
// doubles [R | t], rows of 4; every value is fp32 taken to double, all arithmetic is double and the caller rounds once on its store (the
// contract of pose.hip).  Nothing here touches a thread index, LDS or a HIP call, so the file compiles as host C++ too
// (tools/pose_eval_host_check.cpp defines POSE_DEV empty).  The products keep the reference's zero terms -- its 4 x 4 matmuls multiply
// the translation column by the padded bottom row -- so that an infinite or NaN scale spreads to the same entries as there.
#pragma once

#include <math.h>

#include "rigid.h"

namespace sparf {

static constexpr int PE_MAX_POSES = 64;        // B of one set: both pose arrays of a set are staged in LDS
static constexpr int PE_MAX_VIEWS = 10;        // joint_pose_nerf_trainer.py:233 min(B, 10)
static constexpr int PE_MAX_PAIRS = PE_MAX_VIEWS * (PE_MAX_VIEWS - 1);
static constexpr int PE_SIM3 = 13;             // R (9, rows), t (3), s
static constexpr double PE_PI = 3.141592653589793;      // np.pi

// camera.py:466-471 clamps at 1 - 1e-7 on an fp32 tensor: the bound as that tensor sees it, 0.99999988...
static POSE_DEV double pe_clamp_bound() { return (double)(float)(1.0 - 1e-7); }

// camera.py:92-98 Pose.invert / :37-59 pose_inverse_4x4: [R | t] -> [R^T | -R^T t]
static POSE_DEV void pe_invert(const double p[12], double o[12]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) o[i * 4 + j] = p[j * 4 + i];
        o[i * 4 + 3] = (-p[i]) * p[3] + (-p[4 + i]) * p[7] + (-p[8 + i]) * p[11];
    }
}

// a @ b of two padded poses (bottom row 0 0 0 1), the zero terms kept: 0 * inf is NaN here as in the reference's 4 x 4 product
static POSE_DEV void pe_matmul(const double a[12], const double b[12], double o[12]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[i * 4 + j] = a[i * 4] * b[j] + a[i * 4 + 1] * b[4 + j] + a[i * 4 + 2] * b[8 + j] + a[i * 4 + 3] * (j == 3 ? 1.0 : 0.0);
}

// camera.py:466-471 rotation_distance: acos(clamp((tr(R1 R2^T) - 1) / 2, -c, c)); a NaN passes the clamp as it does torch's
static POSE_DEV double pe_rotation_distance(const double p1[12], const double p2[12]) {
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) tr += p1[i * 4] * p2[i * 4] + p1[i * 4 + 1] * p2[i * 4 + 1] + p1[i * 4 + 2] * p2[i * 4 + 2];
    const double c = pe_clamp_bound();
    double x = (tr - 1.0) / 2.0;
    x = x < -c ? -c : (x > c ? c : x);
    return acos(x);
}

// joint_pose_nerf_trainer.py:257-287 evaluate_camera_alignment of one pose, on the camera-to-world inverses: the rotation error in
// radians and the distance of the camera centres
static POSE_DEV void pe_alignment_errors(const double c2w[12], const double gt_c2w[12], double& err_R, double& err_t) {
    err_R = pe_rotation_distance(c2w, gt_c2w);
    const double dx = c2w[3] - gt_c2w[3], dy = c2w[7] - gt_c2w[7], dz = c2w[11] - gt_c2w[11];
    err_t = sqrt(dx * dx + dy * dy + dz * dz);
}

// candidate p of n views in the reference's order (:233-236): a the outer index, b skips a
static POSE_DEV void pe_pair(int p, int n, int& a, int& b) {
    a = p / (n - 1);
    const int r = p - a * (n - 1);
    b = r + (r >= a ? 1 : 0);
}

// alignment_function (:173-213) of the pair (a, b): scale = |c_gt[a] - c_gt[b]| / |c[a] - c[b]|, T = GT_c2w[a] o inverse(scaled[a])
static POSE_DEV void pe_similarity(const double* c2w, const double* gt_c2w, int a, int b, double T[12], double& scale) {
    const double *ea = c2w + a * 12, *eb = c2w + b * 12, *ga = gt_c2w + a * 12, *gb = gt_c2w + b * 12;
    const double fx = ea[3] - eb[3], fy = ea[7] - eb[7], fz = ea[11] - eb[11];
    const double tx = ga[3] - gb[3], ty = ga[7] - gb[7], tz = ga[11] - gb[11];
    scale = sqrt(tx * tx + ty * ty + tz * tz) / sqrt(fx * fx + fy * fy + fz * fz);
    double sa[12], inv[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) sa[k] = (k & 3) == 3 ? ea[k] * scale : ea[k];
    pe_invert(sa, inv);
    pe_matmul(ga, inv, T);
}

// one estimated camera-to-world pose under (T, scale) -> the aligned world-to-camera pose (:201-209)
static POSE_DEV void pe_align(const double T[12], double scale, const double c2w[12], double aligned_w2c[12]) {
    double sc[12], al[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) sc[k] = (k & 3) == 3 ? c2w[k] * scale : c2w[k];
    pe_matmul(T, sc, al);
    pe_invert(al, aligned_w2c);
}

// the aligned world-to-camera pose against the ground truth, as evaluate_camera_alignment is handed it (:244): inverted again
static POSE_DEV void pe_aligned_errors(const double aligned_w2c[12], const double gt_c2w[12], double& err_R, double& err_t) {
    double back[12];
    pe_invert(aligned_w2c, back);
    pe_alignment_errors(back, gt_c2w, err_R, err_t);
}

// (R_deg_mean, t_mean, R_deg_mean t_mean) of a candidate over all B poses, means in index order (:244-247)
static POSE_DEV void pe_candidate(const double* c2w, const double* gt_c2w, int B, int a, int b, double score[3]) {
    double T[12], scale, sum_R = 0.0, sum_t = 0.0;
    pe_similarity(c2w, gt_c2w, a, b, T, scale);
    for (int i = 0; i < B; ++i) {
        double al[12], eR, et;
        pe_align(T, scale, c2w + i * 12, al);
        pe_aligned_errors(al, gt_c2w + i * 12, eR, et);
        sum_R += eR;
        sum_t += et;
    }
    score[0] = sum_R / (double)B * 180. / PE_PI;
    score[1] = sum_t / (double)B;
    score[2] = score[1] * score[0];
}

// np.argmin on the list of scores (:249), stride 3 doubles: the lowest index that is NaN if any is, otherwise the lowest index of
// the minimum
static POSE_DEV int pe_choose(const double* full_error, int P) {
    int best = 0;
    for (int p = 0; p < P; ++p) {
        const double v = full_error[p * 3];
        if (v != v) return p;
        if (v < full_error[best * 3]) best = p;
    }
    return best;
}

// align_trajectories.py:94-101 backtrack_from_aligning_the_trajectory of one pose under sim = (R, t, s):
// invert([R^T R_c | (R^T / s) (t_c - t)]) with [R_c | t_c] = invert(pose_gt_w2c)
static POSE_DEV void pe_backtrack(const double gt_w2c[12], const double sim[PE_SIM3], double out[12]) {
    double c[12], al[12];
    pe_invert(gt_w2c, c);
    const double d[3] = {c[3] - sim[9], c[7] - sim[10], c[11] - sim[11]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) al[i * 4 + j] = sim[i] * c[j] + sim[3 + i] * c[4 + j] + sim[6 + i] * c[8 + j];
        al[i * 4 + 3] = (sim[i] / sim[12]) * d[0] + (sim[3 + i] / sim[12]) * d[1] + (sim[6 + i] / sim[12]) * d[2];
    }
    pe_invert(al, out);
}

}  // namespace sparf
