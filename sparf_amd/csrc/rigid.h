// Rigid transforms [R | t] as 12 doubles, rows of 4: loads, stores, composition and its vector-Jacobian product -- shared by the pose
// kernels (pose.hip) and the correspondence loss (reproj.h).
#pragma once

#ifndef POSE_DEV
#define POSE_DEV __device__ __forceinline__
#endif

namespace sparf {

static POSE_DEV void load12(const float* p, double m[12]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = (double)p[i];
}
static POSE_DEV void store12(float* p, const double m[12]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) p[i] = (float)m[i];
}

// out = b o a on [R|t] rows of 4:  R = R_b R_a,  t = R_b t_a + t_b   (camera.py:108-115)
static POSE_DEV void compose12(const double a[12], const double b[12], double o[12]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[i * 4 + j] = b[i * 4] * a[j] + b[i * 4 + 1] * a[4 + j] + b[i * 4 + 2] * a[8 + j];
        o[i * 4 + 3] += b[i * 4 + 3];
    }
}
// VJP of compose12: g = d out.  ga = R_b^T g (all four columns);  gb = [g_R R_a^T + g_t t_a^T | g_t].  Either may be skipped (null).
static POSE_DEV void compose12_vjp(const double a[12], const double b[12], const double g[12], double* ga, double* gb) {
    if (ga) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) ga[i * 4 + j] = b[i] * g[j] + b[4 + i] * g[4 + j] + b[8 + i] * g[8 + j];
    }
    if (gb) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                gb[i * 4 + j] = g[i * 4] * a[j * 4] + g[i * 4 + 1] * a[j * 4 + 1] + g[i * 4 + 2] * a[j * 4 + 2] + g[i * 4 + 3] * a[j * 4 + 3];
            gb[i * 4 + 3] = g[i * 4 + 3];
        }
    }
}

}  // namespace sparf
