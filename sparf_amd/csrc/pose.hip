// Pose parameterisations: se(3) -> SE(3) with an optional composition onto a base pose, composition of two
// poses, and the 9-vector (translation + two rows of the rotation) -> pose of the 6D rotation model; each with its exact
// vector-Jacobian product.  One thread per pose, 64-thread workgroups; every value is taken to double as it is loaded, all
// arithmetic runs in double and each result is rounded to float once, on its store (ray_geom of ray_ops.hip inverts the
// intrinsics the same way).  No atomics, no LDS, no state.
#include <hip/hip_runtime.h>

#include "rigid.h"

namespace sparf {

static constexpr int POSE_BLOCK = 64;
static constexpr int POSE_TERMS = 11;          // camera.py:180-205 taylor_A / _B / _C with nth = 10: i = 0 .. 10

// The three truncated series as polynomials in x = theta^2:  P_k(x) = sum_i (-1)^i x^i / (2i + k)!,  k = 1: sin(theta)/theta,
// k = 2: (1 - cos(theta))/theta^2,  k = 3: (theta - sin(theta))/theta^3.  coef(k, i) = (-1)^i / (2i + k)!
static constexpr double pose_coef(int k, int i) {
    double f = 1.0;
    for (int j = 2; j <= 2 * i + k; ++j) f *= (double)j;
    return ((i & 1) ? -1.0 : 1.0) / f;
}
struct PoseSeries {
    double c[3][POSE_TERMS];
};
static constexpr PoseSeries pose_series() {
    PoseSeries s{};
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < POSE_TERMS; ++i) s.c[k][i] = pose_coef(k + 1, i);
    return s;
}
static constexpr PoseSeries kSeries = pose_series();

// P_k(x) and dP_k/dx by Horner
template <int K>
static POSE_DEV void series_eval(double x, double& p, double& dp) {
    p = kSeries.c[K][POSE_TERMS - 1];
    dp = 0.0;
#pragma unroll
    for (int i = POSE_TERMS - 2; i >= 0; --i) {
        dp = dp * x + p;
        p = p * x + kSeries.c[K][i];
    }
}

// wx^2 = w w^T - x I,  x = |w|^2
struct Se3 {
    double w[3], u[3], x, A, dA, B, dB, C, dC;
};
static POSE_DEV Se3 se3_load(const float* xi) {
    Se3 s;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        s.w[i] = (double)xi[i];
        s.u[i] = (double)xi[3 + i];
    }
    s.x = s.w[0] * s.w[0] + s.w[1] * s.w[1] + s.w[2] * s.w[2];
    series_eval<0>(s.x, s.A, s.dA);
    series_eval<1>(s.x, s.B, s.dB);
    series_eval<2>(s.x, s.C, s.dC);
    return s;
}
// M = I + p wx + q wx^2 (row-major 3x3)
static POSE_DEV void se3_matrix(const Se3& s, double p, double q, double M[9]) {
    const double* w = s.w;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i * 3 + j] = q * (w[i] * w[j] - (i == j ? s.x : 0.0)) + (i == j ? 1.0 : 0.0);
    M[1] -= p * w[2]; M[2] += p * w[1];
    M[3] += p * w[2]; M[5] -= p * w[0];
    M[6] -= p * w[1]; M[7] += p * w[0];
}
// refine = [R | V u]   (camera.py:142-157)
static POSE_DEV void se3_refine(const Se3& s, double out[12]) {
    double R[9], V[9];
    se3_matrix(s, s.A, s.B, R);
    se3_matrix(s, s.B, s.C, V);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out[i * 4 + j] = R[i * 3 + j];
        out[i * 4 + 3] = V[i * 3] * s.u[0] + V[i * 3 + 1] * s.u[1] + V[i * 3 + 2] * s.u[2];
    }
}

// <G, wx> = sum_ij G_ij wx_ij  and  <G, wx^2>
static POSE_DEV double dot_wx(const double G[9], const double w[3]) {
    return w[0] * (G[7] - G[5]) + w[1] * (G[2] - G[6]) + w[2] * (G[3] - G[1]);
}
static POSE_DEV double dot_wx2(const double G[9], const double w[3], double x) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) s += G[i * 3 + j] * w[i] * w[j];
    return s - x * (G[0] + G[4] + G[8]);
}

__global__ void __launch_bounds__(POSE_BLOCK) pose_se3_fwd_kernel(const float* xi, const float* base, int n, float* refine_out, float* pose_out) {
    const int i = blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const Se3 s = se3_load(xi + (size_t)i * 6);
    double rf[12];
    se3_refine(s, rf);
    if (refine_out) store12(refine_out + (size_t)i * 12, rf);
    if (base) {
        double b[12], o[12];
        load12(base + (size_t)i * 12, b);
        compose12(rf, b, o);
        store12(pose_out + (size_t)i * 12, o);
    } else {
        store12(pose_out + (size_t)i * 12, rf);
    }
}

__global__ void __launch_bounds__(POSE_BLOCK) pose_se3_bwd_kernel(const float* xi, const float* base, int n, const float* d_pose, const float* d_refine,
                                                                  float* d_xi, float* d_base) {
    const int i = blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const Se3 s = se3_load(xi + (size_t)i * 6);
    double g[12], gr[12];                   // d pose, d refine
    load12(d_pose + (size_t)i * 12, g);
    if (base) {
        double b[12], rf[12], gb[12];
        load12(base + (size_t)i * 12, b);
        se3_refine(s, rf);
        compose12_vjp(rf, b, g, gr, d_base ? gb : nullptr);
        if (d_base) store12(d_base + (size_t)i * 12, gb);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) gr[k] = g[k];
    }
    if (d_refine) {
#pragma unroll
        for (int k = 0; k < 12; ++k) gr[k] += (double)d_refine[(size_t)i * 12 + k];
    }
    // refine = [R | V u]:  gR = d R,  gV = g_t u^T,  g_u = V^T g_t
    double gR[9], gV[9], V[9], gu[3];
    se3_matrix(s, s.B, s.C, V);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gR[r * 3 + c] = gr[r * 4 + c];
            gV[r * 3 + c] = gr[r * 4 + 3] * s.u[c];
        }
        gu[r] = V[r] * gr[3] + V[3 + r] * gr[7] + V[6 + r] * gr[11];
    }
    // R = I + A wx + B wx^2,  V = I + B wx + C wx^2
    const double gA = dot_wx(gR, s.w);
    const double gB = dot_wx2(gR, s.w, s.x) + dot_wx(gV, s.w);
    const double gC = dot_wx2(gV, s.w, s.x);
    double M[9], Q[9];                      // d wx (as a free matrix) and d wx^2
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        M[k] = s.A * gR[k] + s.B * gV[k];
        Q[k] = s.B * gR[k] + s.C * gV[k];
    }
    // wx^2 = w w^T - x I:  d w = (Q + Q^T) w - 2 tr(Q) w;  each series P(x): d w += 2 P'(x) w * its gradient
    const double radial = 2.0 * (s.dA * gA + s.dB * gB + s.dC * gC - (Q[0] + Q[4] + Q[8]));
    double gw[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        gw[r] = radial * s.w[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) gw[r] += (Q[r * 3 + c] + Q[c * 3 + r]) * s.w[c];
    }
    gw[0] += M[7] - M[5];
    gw[1] += M[2] - M[6];
    gw[2] += M[3] - M[1];
    float* o = d_xi + (size_t)i * 6;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o[r] = (float)gw[r];
        o[3 + r] = (float)gu[r];
    }
}

__global__ void __launch_bounds__(POSE_BLOCK) pose_compose_fwd_kernel(const float* a, const float* b, int n, float* out) {
    const int i = blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (i >= n) return;
    double pa[12], pb[12], o[12];
    load12(a + (size_t)i * 12, pa);
    load12(b + (size_t)i * 12, pb);
    compose12(pa, pb, o);
    store12(out + (size_t)i * 12, o);
}

__global__ void __launch_bounds__(POSE_BLOCK) pose_compose_bwd_kernel(const float* a, const float* b, int n, const float* d_out, float* d_a, float* d_b) {
    const int i = blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (i >= n) return;
    double pa[12], pb[12], g[12], ga[12], gb[12];
    load12(a + (size_t)i * 12, pa);
    load12(b + (size_t)i * 12, pb);
    load12(d_out + (size_t)i * 12, g);
    compose12_vjp(pa, pb, g, ga, gb);
    store12(d_a + (size_t)i * 12, ga);
    store12(d_b + (size_t)i * 12, gb);
}

// d9 = (t, a1, a2);  rows of R: b1 = a1 / max(|a1|, eps),  b2 = c / max(|c|, eps) with c = a2 - (b1 . a2) b1,  b3 = b1 x b2
// (two_columns.py:42-62; torch.nn.functional.normalize's eps = 1e-12)
static constexpr double POSE_NORM_EPS = 1e-12;
struct D9 {
    double t[3], a2[3], b1[3], b2[3], b3[3], n1, n2, d;
    bool live1, live2;                      // the norm is above eps: the clamp passes its gradient
};
static POSE_DEV double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static POSE_DEV void cross3(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
static POSE_DEV D9 d9_load(const float* p) {
    D9 s;
    double a1[3], c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        s.t[i] = (double)p[i];
        a1[i] = (double)p[3 + i];
        s.a2[i] = (double)p[6 + i];
    }
    const double l1 = sqrt(dot3(a1, a1));
    s.live1 = l1 >= POSE_NORM_EPS;
    s.n1 = s.live1 ? l1 : POSE_NORM_EPS;
#pragma unroll
    for (int i = 0; i < 3; ++i) s.b1[i] = a1[i] / s.n1;
    s.d = dot3(s.b1, s.a2);
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = s.a2[i] - s.d * s.b1[i];
    const double l2 = sqrt(dot3(c, c));
    s.live2 = l2 >= POSE_NORM_EPS;
    s.n2 = s.live2 ? l2 : POSE_NORM_EPS;
#pragma unroll
    for (int i = 0; i < 3; ++i) s.b2[i] = c[i] / s.n2;
    cross3(s.b1, s.b2, s.b3);
    return s;
}

__global__ void __launch_bounds__(POSE_BLOCK) pose_d9_fwd_kernel(const float* d9, int invert, int n, float* pose_out) {
    const int i = blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const D9 s = d9_load(d9 + (size_t)i * 9);
    const double* rows[3] = {s.b1, s.b2, s.b3};
    double o[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (invert) {                       // Pose.invert, camera.py:92-98: [R^T | -R^T t]
#pragma unroll
            for (int c = 0; c < 3; ++c) o[r * 4 + c] = rows[c][r];
            o[r * 4 + 3] = -(s.b1[r] * s.t[0] + s.b2[r] * s.t[1] + s.b3[r] * s.t[2]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[r * 4 + c] = rows[r][c];
            o[r * 4 + 3] = s.t[r];
        }
    }
    store12(pose_out + (size_t)i * 12, o);
}

// v = a / max(|a|, eps) -> d a from d v:  (g - v (v . g)) / |a| above eps, g / eps below it
static POSE_DEV void normalize_vjp(const double v[3], double nrm, bool live, const double g[3], double ga[3]) {
    const double k = live ? dot3(v, g) : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) ga[i] = (g[i] - v[i] * k) / nrm;
}

__global__ void __launch_bounds__(POSE_BLOCK) pose_d9_bwd_kernel(const float* d9, int invert, int n, const float* d_pose, float* d_d9) {
    const int i = blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const D9 s = d9_load(d9 + (size_t)i * 9);
    double g[12];
    load12(d_pose + (size_t)i * 12, g);
    double gb[3][3], gt[3];                 // d (b1, b2, b3) = d rows of R;  d t
    if (invert) {                           // out_R[r][c] = R[c][r];  out_t[r] = -sum_c R[c][r] t[c]
        const double* rows[3] = {s.b1, s.b2, s.b3};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int r = 0; r < 3; ++r) gb[c][r] = g[r * 4 + c] - s.t[c] * g[r * 4 + 3];
            gt[c] = -(rows[c][0] * g[3] + rows[c][1] * g[7] + rows[c][2] * g[11]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) gb[r][c] = g[r * 4 + c];
            gt[r] = g[r * 4 + 3];
        }
    }
    double x[3], gc[3], ga1[3], ga2[3];
    cross3(s.b2, gb[2], x);                 // b3 = b1 x b2:  d b1 += b2 x g3,  d b2 += g3 x b1
#pragma unroll
    for (int k = 0; k < 3; ++k) gb[0][k] += x[k];
    cross3(gb[2], s.b1, x);
#pragma unroll
    for (int k = 0; k < 3; ++k) gb[1][k] += x[k];
    normalize_vjp(s.b2, s.n2, s.live2, gb[1], gc);
    const double gd = -dot3(gc, s.b1);      // c = a2 - d b1,  d = b1 . a2
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gb[0][k] += gd * s.a2[k] - s.d * gc[k];
        ga2[k] = gc[k] + gd * s.b1[k];
    }
    normalize_vjp(s.b1, s.n1, s.live1, gb[0], ga1);
    float* o = d_d9 + (size_t)i * 9;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = (float)gt[k];
        o[3 + k] = (float)ga1[k];
        o[6 + k] = (float)ga2[k];
    }
}

static inline int pose_grid(int n) { return (n + POSE_BLOCK - 1) / POSE_BLOCK; }
static inline int pose_launched() { return hipGetLastError() == hipSuccess ? 0 : 2; }

int launch_pose_se3_fwd(const float* xi, const float* base, int n, float* refine_out, float* pose_out, hipStream_t s) {
    hipLaunchKernelGGL(pose_se3_fwd_kernel, dim3(pose_grid(n)), dim3(POSE_BLOCK), 0, s, xi, base, n, refine_out, pose_out);
    return pose_launched();
}
int launch_pose_se3_bwd(const float* xi, const float* base, int n, const float* d_pose, const float* d_refine, float* d_xi, float* d_base,
                        hipStream_t s) {
    hipLaunchKernelGGL(pose_se3_bwd_kernel, dim3(pose_grid(n)), dim3(POSE_BLOCK), 0, s, xi, base, n, d_pose, d_refine, d_xi, d_base);
    return pose_launched();
}
int launch_pose_compose_fwd(const float* a, const float* b, int n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(pose_compose_fwd_kernel, dim3(pose_grid(n)), dim3(POSE_BLOCK), 0, s, a, b, n, out);
    return pose_launched();
}
int launch_pose_compose_bwd(const float* a, const float* b, int n, const float* d_out, float* d_a, float* d_b, hipStream_t s) {
    hipLaunchKernelGGL(pose_compose_bwd_kernel, dim3(pose_grid(n)), dim3(POSE_BLOCK), 0, s, a, b, n, d_out, d_a, d_b);
    return pose_launched();
}
int launch_pose_d9_fwd(const float* d9, int invert, int n, float* pose_out, hipStream_t s) {
    hipLaunchKernelGGL(pose_d9_fwd_kernel, dim3(pose_grid(n)), dim3(POSE_BLOCK), 0, s, d9, invert, n, pose_out);
    return pose_launched();
}
int launch_pose_d9_bwd(const float* d9, int invert, int n, const float* d_pose, float* d_d9, hipStream_t s) {
    hipLaunchKernelGGL(pose_d9_bwd_kernel, dim3(pose_grid(n)), dim3(POSE_BLOCK), 0, s, d9, invert, n, d_pose, d_d9);
    return pose_launched();
}

}  // namespace sparf
