// Depth-consistency loss: the body of DepthConsistencyLoss.compute_loss_at_sampled_pose (depth_cons_loss.py:219-321)
// around its two renders as three calls -- project (with the mask and selections of :252-259), select (the visibility threshold of
// :277-283) and loss (:293-312) -- and the gathers that are the backward of the first two.  The arithmetic of a point is dcons.h's; this
// file owns the items of the compactions, the loops, the backward gathers and the entry points.
//
// Compaction keeps source order and uses no atomics (ordered.h's chunked compaction over the two items, in tiles of DCONS_BLOCK
// consecutive points).  Up to DCONS_CHUNK points one workgroup does all of it in one launch; above, a counts launch over chunks of
// DCONS_CHUNK points and a write launch in which each workgroup adds the counts of the chunks before it in chunk order.  The sums of the
// loss are fixed-order (ordered.h's chunked sum over DconsLossSum): a thread adds its points in index order, then the wave, the waves and
// the chunks in their order.  No host synchronisation, no readback: `count` stays in device memory.
#include <hip/hip_runtime.h>

#include "../../include/sparf_hip.h"
#include "dcons.h"
#include "ordered.h"

namespace sparf {

// ---- what is compacted (the items of ordered.h's chunked compaction, one image): `keep(k)` evaluates point k and holds its row,
// `place(k, j)` writes it as output row j with src, `mark(k, j)` leaves dst, `finish` leaves the number kept
template <class A>
struct DconsItem {
    typedef A Args;
    static constexpr int BLOCK = DCONS_BLOCK, CHUNK = DCONS_CHUNK, NCOUNT = 1;
    static __host__ __device__ int n(const A& a) { return a.n; }
    static __host__ __device__ int32_t* ws(const A& a) { return a.ws; }
    static __device__ void finish(const A& a, int, const int (&run)[1]) { a.count[0] = run[0]; }
};

struct DconsProjectItem : DconsItem<DconsProjectArgs> {
    typedef DconsSetup Shared;
    const DconsProjectArgs& a;
    const DconsSetup& s;
    float u, v, z;
    __device__ DconsProjectItem(const DconsProjectArgs& a_, const DconsSetup* s_, int) : a(a_), s(*s_), u(0.f), v(0.f), z(0.f) {}
    static __device__ void setup(const DconsProjectArgs& a, DconsSetup& s) { dcons_setup(a, s); }
    __device__ bool keep(int k) {
        DconsWorld w;
        DconsPoint p;
        if (a.points_w) {
            for (int c = 0; c < 3; ++c) w.Xw[c] = (double)a.points_w[3 * (size_t)k + c];
        } else {
            dcons_backproject(s, (double)a.pixels_ref[2 * (size_t)k], (double)a.pixels_ref[2 * (size_t)k + 1], (double)a.depth_ref[k], w);
        }
        dcons_project(s, w.Xw, p);
        u = (float)p.uv[0];
        v = (float)p.uv[1];
        z = (float)p.X[2];
        return dcons_inside(u, v, z, a.u_max, a.v_max, s.depth_min);
    }
    __device__ void flags(int k, bool in, bool (&f)[1]) { f[0] = in && keep(k); }
    __device__ void place(int k, int j) const {
        a.uv[2 * (size_t)j] = u;
        a.uv[2 * (size_t)j + 1] = v;
        a.z[j] = z;
        a.src[j] = k;
    }
    __device__ void mark(int k, int j) const { a.dst[k] = j; }
};

struct DconsSelectItem : DconsItem<DconsSelectArgs> {
    typedef OrderedNoShared Shared;
    const DconsSelectArgs& a;
    float vis;
    __device__ DconsSelectItem(const DconsSelectArgs& a_, const OrderedNoShared*, int) : a(a_), vis(0.f) {}
    __device__ bool keep(int k) {
        vis = a.vis[k];
        return vis >= a.thresh;                          // tensor.ge(0.2): an fp32 compare
    }
    __device__ void flags(int k, bool in, bool (&f)[1]) { f[0] = in && keep(k); }
    __device__ void place(int k, int j) const {
        a.uv_out[2 * (size_t)j] = a.uv[2 * (size_t)k];
        a.uv_out[2 * (size_t)j + 1] = a.uv[2 * (size_t)k + 1];
        a.z_out[j] = a.z[k];
        a.vis_out[j] = vis;
        a.src[j] = k;
    }
    __device__ void mark(int k, int j) const { a.dst[k] = j; }
};

// ---- the backward of the two compactions: a gather over SOURCE points through dst (no atomics, no zero-fill pass)
__global__ void __launch_bounds__(DCONS_BLOCK) dcons_project_bwd_kernel(DconsProjectArgs a) {
    __shared__ DconsSetup s;
    if (threadIdx.x == 0) dcons_setup(a, s);
    __syncthreads();
    const int k = (int)blockIdx.x * DCONS_BLOCK + (int)threadIdx.x;
    if (k >= a.n) return;
    const int j = a.dst_in[k];
    double gXw[3] = {0.0, 0.0, 0.0}, gd = 0.0;
    if (j >= 0) {
        DconsWorld w;
        DconsPoint p;
        if (a.points_w) {
            for (int c = 0; c < 3; ++c) w.Xw[c] = (double)a.points_w[3 * (size_t)k + c];
        } else {
            dcons_backproject(s, (double)a.pixels_ref[2 * (size_t)k], (double)a.pixels_ref[2 * (size_t)k + 1], (double)a.depth_ref[k], w);
        }
        dcons_project(s, w.Xw, p);
        const double guv[2] = {a.d_uv ? (double)a.d_uv[2 * (size_t)j] : 0.0, a.d_uv ? (double)a.d_uv[2 * (size_t)j + 1] : 0.0};
        dcons_project_vjp(s, p, guv, a.d_z ? (double)a.d_z[j] : 0.0, gXw);
        if (!a.points_w) gd = dcons_backproject_vjp(s, w, gXw);
    }
    if (a.points_w) {
        for (int c = 0; c < 3; ++c) a.d_points_w[3 * (size_t)k + c] = (float)gXw[c];
    } else {
        a.d_depth_ref[k] = (float)gd;
    }
}

__global__ void __launch_bounds__(DCONS_BLOCK) dcons_select_bwd_kernel(const int32_t* dst, const float* d_uv, const float* d_z, int n, float* d_uv_in,
                                                                       float* d_z_in) {
    const int k = (int)blockIdx.x * DCONS_BLOCK + (int)threadIdx.x;
    if (k >= n) return;
    const int j = dst[k];
    if (d_uv_in) {
        d_uv_in[2 * (size_t)k] = (j >= 0 && d_uv) ? d_uv[2 * (size_t)j] : 0.0f;
        d_uv_in[2 * (size_t)k + 1] = (j >= 0 && d_uv) ? d_uv[2 * (size_t)j + 1] : 0.0f;
    }
    if (d_z_in) d_z_in[k] = (j >= 0 && d_z) ? d_z[j] : 0.0f;
}

// ---- the loss: totals and seeds from one pass (the normaliser 1 / (n + 1e-6) is known before the launch)
// the points first, first + DCONS_BLOCK, ... < end into acc, their seeds stored
static __device__ void dcons_loss_loop(const DconsLossArgs& a, int first, int end, double acc[DCONS_NACC]) {
    const double scale = dcons_scale(a.n);
#pragma unroll
    for (int j = 0; j < DCONS_NACC; ++j) acc[j] = 0.0;
    for (int k = first; k < end; k += DCONS_BLOCK) {
        const double zp = (double)a.z_pseudo[k], vis = (double)a.vis[k];
        const double gc = dcons_loss_term(a.loss_type, zp, vis, (double)a.depth[k], (double)a.opacity[k], acc);
        double gf = 0.0;
        if (a.depth_fine) {
            gf = dcons_loss_term(a.loss_type, zp, vis, (double)a.depth_fine[k], (double)a.opacity_fine[k], acc + 2);
            if (a.d_depth_fine) a.d_depth_fine[k] = (float)(-gf * scale);
        }
        if (a.d_depth) a.d_depth[k] = (float)(-gc * scale);
        if (a.d_z_pseudo) a.d_z_pseudo[k] = (float)((gc + gf) * scale);
    }
}

// the policy of ordered.h's chunked sum
struct DconsLossSum {
    typedef DconsLossArgs Args;
    static constexpr int BLOCK = DCONS_BLOCK, CHUNK = DCONS_CHUNK, NACC = DCONS_NACC;
    static __host__ __device__ int rows(const DconsLossArgs& a) { return a.n; }
    static __host__ __device__ double* ws(const DconsLossArgs& a) { return a.ws; }
    static __device__ void loop(const DconsLossArgs& a, int first, int end, double* acc) { dcons_loss_loop(a, first, end, acc); }
    static __device__ void outputs(const DconsLossArgs& a, const double* tot) { dcons_loss_outputs(a, tot); }
};

}  // namespace sparf

using namespace sparf;

// ---- the entry points (sparf_hip.h): every argument check comes before any HIP call; n == 0 launches no kernel
static inline bool dcons_n_ok(int n) { return n >= 0 && n <= (1 << 30); }
static inline bool dcons_rows_ok(int rows) { return rows == 3 || rows == 4; }
// 0: the points form, 1: the back-projecting form, -1: neither or both (or half of the second)
static int dcons_form(const float* points_w, const float* pixels_ref, const float* depth_ref, const float* K_ref, const float* pose_c2w_ref, int ref_rows) {
    const int given = (pixels_ref != nullptr) + (depth_ref != nullptr) + (K_ref != nullptr) + (pose_c2w_ref != nullptr);
    if (points_w) return given == 0 ? 0 : -1;
    return given == 4 && dcons_rows_ok(ref_rows) ? 1 : -1;
}
static int dcons_zero_count(int32_t* count, hipStream_t s) { return hipMemsetAsync(count, 0, sizeof(int32_t), s) == hipSuccess ? 0 : 2; }
static int dcons_zero_out(float* out, hipStream_t s) { return hipMemsetAsync(out, 0, 2 * sizeof(float), s) == hipSuccess ? 0 : 2; }
int64_t sparf_dcons_workspace_bytes(int n) { return n > 0 ? ordered_sum_workspace_bytes<DconsLossSum>(n) : 0; }
// depth_cons_loss.py:247-259 (optionally with :209 folded in): batched_geometry_utils.py:244-247 batch_backproject_to_3d, :262-265
// batch_project, the five-way mask and its boolean-index selections as one ordered compaction
int sparf_dcons_project(const float* points_w, const float* pixels_ref, const float* depth_ref, const float* K_ref, const float* pose_c2w_ref,
                        int ref_rows, const float* pose_w2c_unseen, int unseen_rows, const float* K_unseen, int n, int H, int W, float depth_min,
                        const float* depth_min_dev, float* uv, float* z, int32_t* dst, int32_t* src, int32_t* count, void* workspace, void* stream) {
    if (!dcons_n_ok(n) || !count || !dcons_rows_ok(unseen_rows)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return dcons_zero_count(count, s);       // (an empty tensor has no address: the pointers are not looked at)
    if (dcons_form(points_w, pixels_ref, depth_ref, K_ref, pose_c2w_ref, ref_rows) < 0) return 1;
    if (!pose_w2c_unseen || !K_unseen || !uv || !z || !dst || !src) return 1;
    DconsProjectArgs a{};
    a.n = n; a.ref_rows = ref_rows; a.unseen_rows = unseen_rows;
    a.u_max = (float)(W - 1); a.v_max = (float)(H - 1); a.depth_min = depth_min; a.depth_min_dev = depth_min_dev;
    a.points_w = points_w; a.pixels_ref = pixels_ref; a.depth_ref = depth_ref; a.K_ref = K_ref; a.pose_c2w_ref = pose_c2w_ref;
    a.pose_w2c_unseen = pose_w2c_unseen; a.K_unseen = K_unseen;
    a.uv = uv; a.z = z; a.dst = dst; a.src = src; a.count = count; a.ws = (int32_t*)workspace;
    return launch_ordered_compact<DconsProjectItem>(a, 1, s);
}
// what autograd derives from the lines above for the world points, or for depth_ref in the back-projecting form: a gather through dst
int sparf_dcons_project_backward(const float* points_w, const float* pixels_ref, const float* depth_ref, const float* K_ref,
                                 const float* pose_c2w_ref, int ref_rows, const float* pose_w2c_unseen, int unseen_rows, const float* K_unseen,
                                 int n, const int32_t* dst, const float* d_uv, const float* d_z, float* d_points_w, float* d_depth_ref,
                                 void* stream) {
    if (!dcons_n_ok(n) || !dcons_rows_ok(unseen_rows)) return 1;
    if (n == 0) return 0;
    const int form = dcons_form(points_w, pixels_ref, depth_ref, K_ref, pose_c2w_ref, ref_rows);
    if (form < 0 || !pose_w2c_unseen || !K_unseen || !dst) return 1;
    if (form == 0 ? (!d_points_w || d_depth_ref) : (!d_depth_ref || d_points_w)) return 1;
    DconsProjectArgs a{};
    a.n = n; a.ref_rows = ref_rows; a.unseen_rows = unseen_rows;
    a.points_w = points_w; a.pixels_ref = pixels_ref; a.depth_ref = depth_ref; a.K_ref = K_ref; a.pose_c2w_ref = pose_c2w_ref;
    a.pose_w2c_unseen = pose_w2c_unseen; a.K_unseen = K_unseen;
    a.dst_in = dst; a.d_uv = d_uv; a.d_z = d_z; a.d_points_w = d_points_w; a.d_depth_ref = d_depth_ref;
    hipLaunchKernelGGL(dcons_project_bwd_kernel, dim3((n + DCONS_BLOCK - 1) / DCONS_BLOCK), dim3(DCONS_BLOCK), 0, (hipStream_t)stream, a);
    return launched();
}
// depth_cons_loss.py:277-283: valid_mask = visibility_weight_.ge(0.2) and its five selections
int sparf_dcons_select(const float* vis, const float* uv, const float* z, int m, float thresh, float* uv_out, float* z_out, float* vis_out,
                       int32_t* dst, int32_t* src, int32_t* count, void* workspace, void* stream) {
    if (!dcons_n_ok(m) || !count) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) return dcons_zero_count(count, s);
    if (!vis || !uv || !z || !uv_out || !z_out || !vis_out || !dst || !src) return 1;
    DconsSelectArgs a{};
    a.n = m; a.thresh = thresh; a.vis = vis; a.uv = uv; a.z = z; a.uv_out = uv_out; a.z_out = z_out; a.vis_out = vis_out;
    a.dst = dst; a.src = src; a.count = count; a.ws = (int32_t*)workspace;
    return launch_ordered_compact<DconsSelectItem>(a, 1, s);
}
int sparf_dcons_select_backward(const int32_t* dst, const float* d_uv, const float* d_z, int m, float* d_uv_in, float* d_z_in, void* stream) {
    if (!dcons_n_ok(m)) return 1;
    if (m == 0) return 0;
    if (!dst) return 1;
    if (!d_uv_in && !d_z_in) return 0;
    hipLaunchKernelGGL(dcons_select_bwd_kernel, dim3((m + DCONS_BLOCK - 1) / DCONS_BLOCK), dim3(DCONS_BLOCK), 0, (hipStream_t)stream, dst, d_uv, d_z, m,
                       d_uv_in, d_z_in);
    return launched();
}
// depth_cons_loss.py:293-312: the weighted compute_diff_loss (base_losses.py:197-224) of the coarse and, if given, the fine depth,
// avg_vis_weight, and the gradient seeds of the pseudo depth and of both rendered depths
int sparf_dcons_loss(const float* z_pseudo, const float* vis, const float* depth, const float* opacity, const float* depth_fine,
                     const float* opacity_fine, int m, int loss_type, float* out, float* d_z_pseudo, float* d_depth, float* d_depth_fine,
                     void* workspace, void* stream) {
    if (!dcons_n_ok(m) || loss_type < 0 || loss_type >= DCONS_LOSS_TYPES || !out) return 1;
    if ((depth_fine != nullptr) != (opacity_fine != nullptr) || (d_depth_fine && !depth_fine)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) return dcons_zero_out(out, s);
    if (!z_pseudo || !vis || !depth || !opacity) return 1;
    DconsLossArgs a{};
    a.n = m; a.loss_type = loss_type; a.z_pseudo = z_pseudo; a.vis = vis; a.depth = depth; a.opacity = opacity;
    a.depth_fine = depth_fine; a.opacity_fine = opacity_fine; a.out = out;
    a.d_z_pseudo = d_z_pseudo; a.d_depth = d_depth; a.d_depth_fine = d_depth_fine; a.ws = (double*)workspace;
    return launch_ordered_sum<DconsLossSum>(a, s);
}
