// Correspondence loss: the arguments of the re-projection kernels and their arithmetic as plain functions of doubles,
// shared by the kernels of reproj.hip.  Every value is taken to double as it is loaded and each result is rounded to float once, on its
// store (the contract of pose.hip).  Nothing here touches a thread index, LDS or a HIP call: the functions state the mathematics of ONE
// match, of one term's totals and of the two pose compositions; reproj.hip owns the loops and the reductions.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rigid.h"

#define REPROJ_DEV POSE_DEV

namespace sparf {

enum { REPROJ_HUBER = 0, REPROJ_L1 = 1, REPROJ_MSE = 2, REPROJ_EPE = 3, REPROJ_LOSS_TYPES = 4 };
enum {
    REPROJ_BLOCK = 256,          // four waves, one per SIMD: the ~150 live doubles of a thread stay in registers
    REPROJ_SINGLE_MAX = 4096,    // matches per term up to which one workgroup does everything in one launch
    REPROJ_PARTS = 64,           // workgroups per term above it
    REPROJ_MAX_TERMS = 4,
    // totals of one term: [0] sum l w valid, [1] #valid, [2] #pixel check passed, [3] #depth check passed, [4..19] d T (unnormalised), [20] sum depth_i
    REPROJ_NACC = 21,
};

struct ReprojTerm {              // one direction i -> j
    const float *pix_i, *depth_i, *pix_j, *depth_j;     // [n][2], [n], [n][2], [n] (depth_j may be null without the depth check)
    float* d_depth_i;            // [n] gradient seed, or null
    int cam_i, cam_j, tf;        // which of K[2] is K_i / K_j, which of the two transforms is T
};

struct ReprojArgs {
    int n, nterms, loss_type, pix_check, depth_check, pair;
    float pix_thresh, depth_thresh;
    const float* K[2];           // [3][3] each
    const float* T;              // [4][4] (single term: pair == 0)
    const float* pose[2];        // [3][4] w2c of self, other (pair != 0)
    const float* weights;        // [n] or null
    ReprojTerm term[REPROJ_MAX_TERMS];
    float* out;                  // [4]: loss, perc_val_pix_rep, perc_val_depth_rep, mean(depth_i of term 0)
    unsigned char* valid;        // [n] mask of term 0, or null
    float* d_T;                  // [16] (single term), or null
    float* d_pose[2];            // [3][4] each (pair), or null
    double* ws;                  // [nterms][REPROJ_PARTS][REPROJ_NACC] partial totals (n > REPROJ_SINGLE_MAX), or null
};

// what every workgroup derives from the 3x3 and 3x4 / 4x4 operands before its loop: K, K^-1 of both cameras, both transforms
struct ReprojSetup {
    double K[2][9], Kinv[2][9], T[2][16];
};
// what one workgroup accumulates over the terms: the outputs in double, d T of both transforms
struct ReprojFinal {
    double out[4], G[2][16];
};

// K^-1 = adj(K) / det(K): general K, not only the pinhole pattern (batched_geometry_utils.py:220 torch.inverse)
static REPROJ_DEV void reproj_inverse3(const double K[9], double o[9]) {
    const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[5] * K[6] - K[3] * K[8], c02 = K[3] * K[7] - K[4] * K[6];
    const double det = K[0] * c00 + K[1] * c01 + K[2] * c02;
    o[0] = c00 / det; o[1] = (K[2] * K[7] - K[1] * K[8]) / det; o[2] = (K[1] * K[5] - K[2] * K[4]) / det;
    o[3] = c01 / det; o[4] = (K[0] * K[8] - K[2] * K[6]) / det; o[5] = (K[2] * K[3] - K[0] * K[5]) / det;
    o[6] = c02 / det; o[7] = (K[1] * K[6] - K[0] * K[7]) / det; o[8] = (K[0] * K[4] - K[1] * K[3]) / det;
}

// [R | t] rows of 4 -> [R^T | -R^T t] (camera.py:37-61 pose_inverse_4x4, the transpose form)
static REPROJ_DEV void reproj_rigid_inverse(const double p[12], double o[12]) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[i * 4 + j] = p[j * 4 + i];
        o[i * 4 + 3] = -(p[i] * p[3] + p[4 + i] * p[7] + p[8 + i] * p[11]);
    }
}
// its VJP: g = d out -> d p.  d R[k][i] = g_R[i][k] - t[k] g_t[i];  d t[k] = -sum_i R[k][i] g_t[i]
static REPROJ_DEV void reproj_rigid_inverse_vjp(const double p[12], const double g[12], double gp[12]) {
    for (int k = 0; k < 3; ++k) {
        for (int i = 0; i < 3; ++i) gp[k * 4 + i] = g[i * 4 + k] - p[k * 4 + 3] * g[i * 4 + 3];
        gp[k * 4 + 3] = -(p[k * 4] * g[3] + p[k * 4 + 1] * g[7] + p[k * 4 + 2] * g[11]);
    }
}
static REPROJ_DEV void reproj_load(const float* p, int n, double* o) {
    for (int i = 0; i < n; ++i) o[i] = (double)p[i];
}

// corres_loss.py:188, :199: T_s2o = P_other pose_inverse_4x4(P_self), T_o2s = pose_inverse_4x4(T_s2o); bottom rows exactly [0,0,0,1]
static REPROJ_DEV void reproj_setup(const ReprojArgs& a, ReprojSetup& s) {
    for (int c = 0; c < 2; ++c) {
        reproj_load(a.K[c], 9, s.K[c]);
        reproj_inverse3(s.K[c], s.Kinv[c]);
    }
    if (a.pair) {
        double ps[12], po[12], inv[12];
        load12(a.pose[0], ps);
        load12(a.pose[1], po);
        reproj_rigid_inverse(ps, inv);
        compose12(inv, po, s.T[0]);
        reproj_rigid_inverse(s.T[0], s.T[1]);
        for (int c = 0; c < 2; ++c) {
            s.T[c][12] = s.T[c][13] = s.T[c][14] = 0.0;
            s.T[c][15] = 1.0;
        }
    } else {
        reproj_load(a.T, 16, s.T[0]);
        for (int i = 0; i < 16; ++i) s.T[1][i] = 0.0;
    }
}

// One match of one term, batched_geometry_utils.py:199-228 in its operation order, then corres_loss.py:77-91 and
// base_losses.py:197-224.  Out: l = loss w valid; the checks; gd = d l / d depth_i; gh = d l / d h with h = T [x, 1]; x.
struct ReprojMatch {
    double l, gd, gh[4], x[3];
    bool vpix, vdepth;
};
static REPROJ_DEV void reproj_match(const ReprojArgs& a, const ReprojTerm& t, const double* Kinv, const double* Kj, const double* T, int k,
                                    ReprojMatch& m) {
    const double px = (double)t.pix_i[2 * (size_t)k], py = (double)t.pix_i[2 * (size_t)k + 1], d = (double)t.depth_i[k];
    const double qx = (double)t.pix_j[2 * (size_t)k], qy = (double)t.pix_j[2 * (size_t)k + 1];
    double ray[3], h[4], X[3], y[3];
    for (int r = 0; r < 3; ++r) {
        ray[r] = Kinv[3 * r] * px + Kinv[3 * r + 1] * py + Kinv[3 * r + 2];
        m.x[r] = ray[r] * d;
    }
    for (int r = 0; r < 4; ++r) h[r] = T[4 * r] * m.x[0] + T[4 * r + 1] * m.x[1] + T[4 * r + 2] * m.x[2] + T[4 * r + 3];
    const double s = h[3] + 1e-6;
    for (int r = 0; r < 3; ++r) X[r] = h[r] / s;
    for (int r = 0; r < 3; ++r) y[r] = Kj[3 * r] * X[0] + Kj[3 * r + 1] * X[1] + Kj[3 * r + 2] * X[2];
    const double sy = y[2] + 1e-6;
    const double uv[2] = {y[0] / sy, y[1] / sy};
    const double e[2] = {uv[0] - qx, uv[1] - qy};
    const double r = sqrt(e[0] * e[0] + e[1] * e[1]);
    m.vpix = !a.pix_check || r <= (double)a.pix_thresh;
    m.vdepth = true;
    if (a.depth_check) {
        const double dj = (double)t.depth_j[k];
        m.vdepth = fabs(dj - X[2]) / (dj + 1e-6) <= (double)a.depth_thresh;
    }
    double l = 0.0, ge[2];
    if (a.loss_type == REPROJ_EPE) {
        l = r;
        for (int c = 0; c < 2; ++c) ge[c] = r > 0.0 ? e[c] / r : 0.0;
    } else {
        for (int c = 0; c < 2; ++c) {
            const double ab = fabs(e[c]), sg = e[c] > 0.0 ? 1.0 : e[c] < 0.0 ? -1.0 : 0.0;
            if (a.loss_type == REPROJ_HUBER) {           // delta 1
                l += ab <= 1.0 ? 0.5 * e[c] * e[c] : ab - 0.5;
                ge[c] = ab <= 1.0 ? e[c] : sg;
            } else if (a.loss_type == REPROJ_L1) {
                l += ab;
                ge[c] = sg;
            } else {
                l += e[c] * e[c];
                ge[c] = 2.0 * e[c];
            }
        }
    }
    const double w = (m.vpix && m.vdepth) ? (a.weights ? (double)a.weights[k] : 1.0) : 0.0;
    m.l = l * w;
    // uv = y[0:2] / sy;  y = K_j X;  X = h[0:3] / s;  h = T [x, 1];  x = ray d
    const double gy[3] = {ge[0] * w / sy, ge[1] * w / sy, -(ge[0] * uv[0] + ge[1] * uv[1]) * w / sy};
    double gX[3];
    for (int c = 0; c < 3; ++c) gX[c] = Kj[c] * gy[0] + Kj[3 + c] * gy[1] + Kj[6 + c] * gy[2];
    for (int c = 0; c < 3; ++c) m.gh[c] = gX[c] / s;
    m.gh[3] = -(gX[0] * X[0] + gX[1] * X[1] + gX[2] * X[2]) / s;
    m.gd = 0.0;
    for (int c = 0; c < 3; ++c) m.gd += (T[c] * m.gh[0] + T[4 + c] * m.gh[1] + T[8 + c] * m.gh[2] + T[12 + c] * m.gh[3]) * ray[c];
}

static REPROJ_DEV void reproj_accumulate(const ReprojMatch& m, double depth_i, double acc[REPROJ_NACC]) {
    acc[0] += m.l;
    acc[1] += (m.vpix && m.vdepth) ? 1.0 : 0.0;
    acc[2] += m.vpix ? 1.0 : 0.0;
    acc[3] += m.vdepth ? 1.0 : 0.0;
    for (int r = 0; r < 4; ++r) {
        for (int c = 0; c < 3; ++c) acc[4 + 4 * r + c] += m.gh[r] * m.x[c];
        acc[4 + 4 * r + 3] += m.gh[r];
    }
    acc[20] += depth_i;
}

// base_losses.py:223 and corres_loss.py:218: what every seed and sum of a term is multiplied by
static REPROJ_DEV double reproj_scale(const ReprojArgs& a, const double tot[REPROJ_NACC]) { return 1.0 / ((tot[1] + 1e-6) * (double)a.nterms); }

static REPROJ_DEV void reproj_final_init(ReprojFinal& f) {
    for (int i = 0; i < 4; ++i) f.out[i] = 0.0;
    for (int i = 0; i < 32; ++i) f.G[i / 16][i % 16] = 0.0;
}
// the totals of term t into the outputs: the loss adds up, the stats are those of the last term evaluated (corres_loss.py:82, :88
// overwrite stats_dict), depth_in_corr_loss is the coarse depth_self's mean (:186)
static REPROJ_DEV void reproj_term_finish(const ReprojArgs& a, int t, const double tot[REPROJ_NACC], ReprojFinal& f) {
    const double scale = reproj_scale(a, tot);
    f.out[0] += tot[0] * scale;
    if (a.pix_check) f.out[1] = tot[2] / ((double)a.n + 1e-6);
    if (a.depth_check) f.out[2] = tot[3] / ((double)a.n + 1e-6);
    if (t == 0) f.out[3] = tot[20] / (double)a.n;
    double* G = f.G[a.term[t].tf];
    for (int i = 0; i < 16; ++i) G[i] += tot[4 + i] * scale;
}
// the stores of one call: out[4], d T or the two d pose through the VJP of T_o2s = inverse(T_s2o), T_s2o = P_other o inverse(P_self)
static REPROJ_DEV void reproj_outputs(const ReprojArgs& a, const ReprojSetup& s, const ReprojFinal& f) {
    for (int i = 0; i < 4; ++i) a.out[i] = (float)f.out[i];
    if (!a.pair) {
        if (a.d_T)
            for (int i = 0; i < 16; ++i) a.d_T[i] = (float)f.G[0][i];
        return;
    }
    if (!a.d_pose[0] && !a.d_pose[1]) return;
    double ps[12], po[12], inv[12], g1[12], g2[12], ginv[12], gs[12], go[12];
    load12(a.pose[0], ps);
    load12(a.pose[1], po);
    reproj_rigid_inverse(ps, inv);
    reproj_rigid_inverse_vjp(s.T[0], f.G[1], g2);          // (the top three rows of a 4x4 ARE its [R | t])
    for (int i = 0; i < 12; ++i) g1[i] = f.G[0][i] + g2[i];
    compose12_vjp(inv, po, g1, ginv, go);
    reproj_rigid_inverse_vjp(ps, ginv, gs);
    for (int i = 0; i < 12; ++i) {
        if (a.d_pose[0]) a.d_pose[0][i] = (float)gs[i];
        if (a.d_pose[1]) a.d_pose[1][i] = (float)go[i];
    }
}

}  // namespace sparf
