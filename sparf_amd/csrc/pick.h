// The depth-consistency front end and the ray sampler: the arguments of the kernels of pick.hip and their arithmetic
// as plain functions -- which pixel an output row of sample_rays / sample_rays_for_patch / RaySamplingStrategy.__call__
// (source/training/core/sampling_strategies.py:132-296) is, and every element of the four matrices and the index that
// DepthConsistencyLoss.sample_pose (depth_cons_loss.py:45-63) with get_nearest_pose_ids (data_utils.py:248-311, 'vector', one neighbour,
// scene centre 0) and pose_inverse_4x4 (camera.py:37-64) leave.  Nothing here touches a thread index, LDS or a HIP call; pick.hip owns
// the loops and the entry points.
// Pixels.  A pool is a rectangle given by value: index i of pool A is (i % a_w, i / a_w), of pool B (b_x0 + i % b_w, b_y0 + i / b_w)
// -- the reference's meshgrid order and its linspace centre box, whose values are exact integers.  A permutation entry outside
// [0, pool size) is the caller's error (torch raises on it); it is CLAMPED into the pool here, so every pixel is a pixel of its pool
// plus a patch offset and no address depends on a wild value.  The entry points check that pool + patch - 1 stays inside a ROW
// (x < W); the image height is not an argument, so y is bounded by the pools the caller hands over -- the reference's own pools keep
// it below H except a centre box with precrop_frac near 1 under a patch, where the reference leaves the image too.
// Poses.  float32 as the reference's torch ops, the angular distances in double on the float32 centres as numpy computes them (the int64
// scene centre promotes them).  The blend w a + (1 - w) b is element-wise: two rounded products and one rounded sum, never contracted.
// The file also compiles as plain C++ (tools/pick_host_check.cpp evaluates it on the host under the sanitizers).
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef PICK_DEV
#ifdef __HIPCC__
#define PICK_DEV __host__ __device__ __forceinline__
#else
#define PICK_DEV inline
#endif
#endif

namespace sparf {

enum {
    PICK_BLOCK = 256,            // four waves: the output rows of a workgroup
    PICK_WAVE = 64,              // the one wave of the pose kernel
};

struct PickPixelsArgs {
    const int64_t* perm_a;       // [n_a] indices into pool A, or null (n_a == 0)
    const int64_t* perm_b;       // [n_b] indices into pool B, or null (n_b == 0)
    int n_a, n_b;
    int a_w, a_h;                // pool A: the grid [0, a_w) x [0, a_h)
    int b_x0, b_y0, b_w, b_h;    // pool B: the box of b_w x b_h pixels at (b_x0, b_y0)
    int W, patch, rows;          // rows = (n_a + n_b) patch^2
    float* pixels;               // [rows][2] (x, y), or null
    int64_t* rays;               // [rows] y W + x, or null
};

struct UnseenPoseArgs {
    const float* poses_w2c;      // [B][row_floats]: [B,3,4] (12) or [B,4,4] (16)
    int row_floats, B, id_self;
    float w, one_minus_w;
    float* w2c_ref;              // [16] poses_w2c[id_self] on top of its bottom row ([0,0,0,1] for a [3,4] pose)
    float* c2w_ref;              // [16] its transpose inverse
    float* c2w_other;            // [16] the transpose inverse of the nearest other pose
    float* w2c_unseen;           // [16] the transpose inverse of the blend
    int32_t* id_other;           // [1]
};

// ---- pixels
// a permutation entry -> an index of a pool of `size` > 0 elements
static PICK_DEV int pick_clamp(int64_t i, int size) { return (int)(i < 0 ? 0 : i >= (int64_t)size ? (int64_t)size - 1 : i); }

// output row -> (x, y): the picks of A, then the picks of B (the reference's cat), each expanded by the patch offsets, dy outer, dx inner
static PICK_DEV void pick_pixel(const PickPixelsArgs& a, int row, int& x, int& y) {
    const int pp = a.patch * a.patch, k = row / pp, o = row - k * pp, dy = o / a.patch, dx = o - dy * a.patch;
    if (k < a.n_a) {
        const int i = pick_clamp(a.perm_a[k], a.a_w * a.a_h);
        x = i % a.a_w;
        y = i / a.a_w;
    } else {
        const int i = pick_clamp(a.perm_b[k - a.n_a], a.b_w * a.b_h);
        x = a.b_x0 + i % a.b_w;
        y = a.b_y0 + i / a.b_w;
    }
    x += dx;
    y += dy;
}

static PICK_DEV int64_t pick_ray(int x, int y, int W) { return (int64_t)y * (int64_t)W + (int64_t)x; }

// everything of output row `row`: plain stores
static PICK_DEV void pick_row(const PickPixelsArgs& a, int row) {
    int x, y;
    pick_pixel(a, row, x, y);
    if (a.pixels) {
        a.pixels[2 * (size_t)row] = (float)x;
        a.pixels[2 * (size_t)row + 1] = (float)y;
    }
    if (a.rays) a.rays[row] = pick_ray(x, y, a.W);
}

// ---- poses
// w a + (1 - w) b as torch evaluates `w * A + (1 - w) * B` on float32 tensors: each product rounded, then the sum
static PICK_DEV float pick_blend(float w, float a, float omw, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(__fmul_rn(w, a), __fmul_rn(omw, b));
#else
    volatile float p = w * a, q = omw * b;               // (volatile: no contraction whatever the host compiler's default)
    return p + q;
#endif
}

// element (r, c), r < 3, of pose m ([3,4] rows of a [B][row_floats] array)
static PICK_DEV float pick_at(const float* m, int r, int c) { return m[4 * r + c]; }

// element (r, c) of pose_inverse_4x4 of m: [R^T | -R^T t] on top of [0,0,0,1]
static PICK_DEV float pick_inverse_at(const float* m, int r, int c) {
    if (r == 3) return c == 3 ? 1.0f : 0.0f;
    if (c < 3) return pick_at(m, c, r);
    return -(pick_at(m, 0, r) * pick_at(m, 0, 3) + pick_at(m, 1, r) * pick_at(m, 1, 3) + pick_at(m, 2, r) * pick_at(m, 2, 3));
}

// element (r, c) of m as a [4,4]: its own bottom row where it has one
static PICK_DEV float pick_full_at(const float* m, int row_floats, int r, int c) {
    if (r < 3 || row_floats == 16) return m[4 * r + c];
    return c == 3 ? 1.0f : 0.0f;
}

// element (r, c), r < 3, of the blend of the inverses of ms (self) and mo (other)
static PICK_DEV float pick_blend_at(const UnseenPoseArgs& a, const float* ms, const float* mo, int r, int c) {
    return pick_blend(a.w, pick_inverse_at(ms, r, c), a.one_minus_w, pick_inverse_at(mo, r, c));
}

// element (r, c) of the transpose inverse of that blend (which is not rigid; the reference transposes it all the same)
static PICK_DEV float pick_unseen_at(const UnseenPoseArgs& a, const float* ms, const float* mo, int r, int c) {
    if (r == 3) return c == 3 ? 1.0f : 0.0f;
    if (c < 3) return pick_blend_at(a, ms, mo, c, r);
    return -(pick_blend_at(a, ms, mo, 0, r) * pick_blend_at(a, ms, mo, 0, 3) + pick_blend_at(a, ms, mo, 1, r) * pick_blend_at(a, ms, mo, 1, 3) +
             pick_blend_at(a, ms, mo, 2, r) * pick_blend_at(a, ms, mo, 2, 3));
}

static PICK_DEV const float* pick_pose(const UnseenPoseArgs& a, int j) { return a.poses_w2c + (size_t)j * (size_t)a.row_floats; }

// data_utils.py:248-252 on the float32 camera centres of poses s and j, in double: acos(clip(u_s . u_j, -1, 1)), u = v / (|v| + 1e-6)
static PICK_DEV double pick_angle(const float* ms, const float* mj) {
    double s[3], v[3];
    for (int k = 0; k < 3; ++k) {
        s[k] = (double)pick_inverse_at(ms, k, 3);
        v[k] = (double)pick_inverse_at(mj, k, 3);
    }
    const double ns = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]) + 1e-6, nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + 1e-6;
    double d = (s[0] / ns) * (v[0] / nv) + (s[1] / ns) * (v[1] / nv) + (s[2] / ns) * (v[2] / nv);
    d = d < -1.0 ? -1.0 : d > 1.0 ? 1.0 : d;
    return acos(d);
}

// the distance get_nearest_pose_ids sorts by: the self entry is 1e3
static PICK_DEV double pick_dist(const UnseenPoseArgs& a, int j) {
    return j == a.id_self ? 1e3 : pick_angle(pick_pose(a, a.id_self), pick_pose(a, j));
}

// (d, j) comes before (e, k) in the order of the search: the smaller distance, the lower index among equals
static PICK_DEV bool pick_before(double d, int j, double e, int k) { return d < e || (d == e && j < k); }

// the first index of the minimum over j = first, first + step, ... < B; (1e300, B) without one
static PICK_DEV void pick_nearest(const UnseenPoseArgs& a, int first, int step, double& best, int& at) {
    best = 1e300;
    at = a.B;
    for (int j = first; j < a.B; j += step) {
        const double d = pick_dist(a, j);
        if (pick_before(d, j, best, at)) { best = d; at = j; }
    }
}

// element e = 4 r + c of the four matrices, the other pose known
static PICK_DEV void pick_pose_outputs(const UnseenPoseArgs& a, int id_other, int e) {
    const int r = e >> 2, c = e & 3;
    const float *ms = pick_pose(a, a.id_self), *mo = pick_pose(a, id_other);
    a.w2c_ref[e] = pick_full_at(ms, a.row_floats, r, c);
    a.c2w_ref[e] = pick_inverse_at(ms, r, c);
    a.c2w_other[e] = pick_inverse_at(mo, r, c);
    a.w2c_unseen[e] = pick_unseen_at(a, ms, mo, r, c);
}

}  // namespace sparf
