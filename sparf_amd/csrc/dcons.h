// Depth-consistency loss: the arguments of the project / select / loss kernels and their arithmetic as plain functions
// of doubles, shared by the kernels of dcons.hip.  Every value is taken to double as it is loaded and each result is rounded to float
// once, on its store (the contract of pose.hip and reproj.h).  Nothing here touches a thread index, LDS or a HIP call: the functions
// state the mathematics of ONE point; dcons.hip owns the loops, the compaction and the reductions.
#pragma once
#include <math.h>
#include <stdint.h>

#include "reproj.h"

#define DCONS_DEV POSE_DEV

namespace sparf {

enum {
    DCONS_BLOCK = 256,           // four waves, one per SIMD; a tile of the compaction = 256 consecutive points
    DCONS_CHUNK = 4096,          // points up to which one workgroup does everything in one launch; above, the points of one workgroup
    DCONS_LOSS_TYPES = 3,        // REPROJ_HUBER, REPROJ_L1, REPROJ_MSE (epe on a 1-D difference is the norm of the whole vector: torch's)
    // totals of the loss: [0] sum l w (coarse), [1] sum w (coarse), [2] sum l w (fine), [3] sum w (fine)
    DCONS_NACC = 4,
};

struct DconsProjectArgs {
    int n, ref_rows, unseen_rows;                        // rows of the two poses: 3 or 4 (a missing bottom row is [0,0,0,1])
    float u_max, v_max, depth_min;                       // W - 1, H - 1, depth_range[0][0]
    const float* depth_min_dev;                          // the same on the device (then depth_min is not read), or null
    const float* points_w;                               // [n][3], or null: back-project
    const float *pixels_ref, *depth_ref, *K_ref, *pose_c2w_ref;     // [n][2], [n], [3][3], [rows][4]
    const float *pose_w2c_unseen, *K_unseen;             // [rows][4], [3][3]
    float *uv, *z;                                       // forward: [count][2], [count] (room for n)
    int32_t *dst, *src, *count;                          // forward: [n], [count], [1]
    int32_t* ws;                                         // [chunks] counts (n > DCONS_CHUNK), or null
    const int32_t* dst_in;                               // backward: [n]
    const float *d_uv, *d_z;                             // backward: [count][2], [count]; null = 0
    float *d_points_w, *d_depth_ref;                     // backward: [n][3] or [n]
};

struct DconsSelectArgs {
    int n;
    float thresh;
    const float *vis, *uv, *z;                           // [n], [n][2], [n]
    float *uv_out, *z_out, *vis_out;                     // [count][2], [count], [count] (room for n)
    int32_t *dst, *src, *count, *ws;
};

struct DconsLossArgs {
    int n, loss_type;
    const float *z_pseudo, *vis, *depth, *opacity, *depth_fine, *opacity_fine;      // [n] each; the fine two or null
    float* out;                                          // [2]: loss, avg_vis_weight
    float *d_z_pseudo, *d_depth, *d_depth_fine;          // [n] each, or null
    double* ws;                                          // [chunks][DCONS_NACC] partial totals (n > DCONS_CHUNK), or null
};

// what every workgroup derives from the matrices before its loop
struct DconsSetup {
    double Kinv[9], T[16], P[16], K[9];                  // K_ref^-1, T_c2w of the reference view, P of the unseen view, K_unseen
    float depth_min;
};

static DCONS_DEV void dcons_load_pose(const float* p, int rows, double o[16]) {
    for (int i = 0; i < 4 * rows; ++i) o[i] = (double)p[i];
    if (rows == 3) {
        o[12] = o[13] = o[14] = 0.0;
        o[15] = 1.0;
    }
}
static DCONS_DEV void dcons_setup(const DconsProjectArgs& a, DconsSetup& s) {
    if (!a.points_w) {
        double K[9];
        reproj_load(a.K_ref, 9, K);
        reproj_inverse3(K, s.Kinv);
        dcons_load_pose(a.pose_c2w_ref, a.ref_rows, s.T);
    }
    dcons_load_pose(a.pose_w2c_unseen, a.unseen_rows, s.P);
    reproj_load(a.K_unseen, 9, s.K);
    s.depth_min = a.depth_min_dev ? a.depth_min_dev[0] : a.depth_min;
}

// batched_geometry_utils.py:244-247 batch_backproject_to_3d in its operation order: ray = K^-1 [p, 1]; x = ray d; h = T [x, 1];
// X_w = h[0:3] / (h[3] + 1e-6)
struct DconsWorld {
    double ray[3], Xw[3], sh;
};
static DCONS_DEV void dcons_backproject(const DconsSetup& s, double px, double py, double d, DconsWorld& w) {
    double x[3], h[4];
    for (int r = 0; r < 3; ++r) {
        w.ray[r] = s.Kinv[3 * r] * px + s.Kinv[3 * r + 1] * py + s.Kinv[3 * r + 2];
        x[r] = w.ray[r] * d;
    }
    for (int r = 0; r < 4; ++r) h[r] = s.T[4 * r] * x[0] + s.T[4 * r + 1] * x[1] + s.T[4 * r + 2] * x[2] + s.T[4 * r + 3];
    w.sh = h[3] + 1e-6;
    for (int r = 0; r < 3; ++r) w.Xw[r] = h[r] / w.sh;
}

// batched_geometry_utils.py:262-265 batch_project with return_depth: g = P [X_w, 1]; X = g[0:3] / (g[3] + 1e-6); y = K X;
// uv = y[0:2] / (y[2] + 1e-6); z = X[2]
struct DconsPoint {
    double X[3], uv[2], s, sy;
};
static DCONS_DEV void dcons_project(const DconsSetup& s, const double Xw[3], DconsPoint& p) {
    double g[4], y[3];
    for (int r = 0; r < 4; ++r) g[r] = s.P[4 * r] * Xw[0] + s.P[4 * r + 1] * Xw[1] + s.P[4 * r + 2] * Xw[2] + s.P[4 * r + 3];
    p.s = g[3] + 1e-6;
    for (int r = 0; r < 3; ++r) p.X[r] = g[r] / p.s;
    for (int r = 0; r < 3; ++r) y[r] = s.K[3 * r] * p.X[0] + s.K[3 * r + 1] * p.X[1] + s.K[3 * r + 2] * p.X[2];
    p.sy = y[2] + 1e-6;
    p.uv[0] = y[0] / p.sy;
    p.uv[1] = y[1] / p.sy;
}
// depth_cons_loss.py:252-254 on the values as they are stored: what goes to the renderer is consistent with the mask
static DCONS_DEV bool dcons_inside(float u, float v, float z, float u_max, float v_max, float depth_min) {
    return u >= 0.0f && v >= 0.0f && u <= u_max && v <= v_max && z >= depth_min;
}
// the VJP of dcons_project: (d uv, d z) -> d X_w
static DCONS_DEV void dcons_project_vjp(const DconsSetup& s, const DconsPoint& p, const double guv[2], double gz, double gXw[3]) {
    const double gy[3] = {guv[0] / p.sy, guv[1] / p.sy, -(guv[0] * p.uv[0] + guv[1] * p.uv[1]) / p.sy};
    double gX[3], gg[4];
    for (int c = 0; c < 3; ++c) gX[c] = s.K[c] * gy[0] + s.K[3 + c] * gy[1] + s.K[6 + c] * gy[2];
    gX[2] += gz;
    for (int c = 0; c < 3; ++c) gg[c] = gX[c] / p.s;
    gg[3] = -(gX[0] * p.X[0] + gX[1] * p.X[1] + gX[2] * p.X[2]) / p.s;
    for (int c = 0; c < 3; ++c) gXw[c] = s.P[c] * gg[0] + s.P[4 + c] * gg[1] + s.P[8 + c] * gg[2] + s.P[12 + c] * gg[3];
}
// the VJP of dcons_backproject: d X_w -> d depth_ref (nothing to K, the pose or the pixels: the reference detaches them, :172)
static DCONS_DEV double dcons_backproject_vjp(const DconsSetup& s, const DconsWorld& w, const double gXw[3]) {
    double gh[4], gd = 0.0;
    for (int c = 0; c < 3; ++c) gh[c] = gXw[c] / w.sh;
    gh[3] = -(gXw[0] * w.Xw[0] + gXw[1] * w.Xw[1] + gXw[2] * w.Xw[2]) / w.sh;
    for (int c = 0; c < 3; ++c) gd += (s.T[c] * gh[0] + s.T[4 + c] * gh[1] + s.T[8 + c] * gh[2] + s.T[12 + c] * gh[3]) * w.ray[c];
    return gd;
}

// base_losses.py:197-224 compute_diff_loss on one difference: l and d l / d e (huber with delta 1)
static DCONS_DEV void dcons_diff_loss(int loss_type, double e, double& l, double& ge) {
    const double ab = fabs(e), sg = e > 0.0 ? 1.0 : e < 0.0 ? -1.0 : 0.0;
    if (loss_type == REPROJ_HUBER) {
        l = ab <= 1.0 ? 0.5 * e * e : ab - 0.5;
        ge = ab <= 1.0 ? e : sg;
    } else if (loss_type == REPROJ_L1) {
        l = ab;
        ge = sg;
    } else {
        l = e * e;
        ge = 2.0 * e;
    }
}
// depth_cons_loss.py:293-300 (or :303-310) for one kept point: w = vis opacity (detached), e = z_pseudo - depth; adds l w and w to
// acc[0..1]; -> d (l w) / d e
static DCONS_DEV double dcons_loss_term(int loss_type, double zp, double vis, double depth, double opacity, double acc[2]) {
    const double w = vis * opacity;
    double l, ge;
    dcons_diff_loss(loss_type, zp - depth, l, ge);
    acc[0] += l * w;
    acc[1] += w;
    return ge * w;
}
// base_losses.py:223 and depth_cons_loss.py:312: one over (number of kept points + 1e-6), known before the launch
static DCONS_DEV double dcons_scale(int n) { return 1.0 / ((double)n + 1e-6); }
// the totals into out[2]: the loss terms add up, avg_vis_weight is that of the last term evaluated (:312 reads the overwritten variable)
static DCONS_DEV void dcons_loss_outputs(const DconsLossArgs& a, const double tot[DCONS_NACC]) {
    const double scale = dcons_scale(a.n);
    a.out[0] = (float)(a.depth_fine ? tot[0] * scale + tot[2] * scale : tot[0] * scale);
    a.out[1] = (float)((a.depth_fine ? tot[3] : tot[1]) * scale);
}

}  // namespace sparf
