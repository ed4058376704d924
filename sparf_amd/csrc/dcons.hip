// Depth-consistency loss: the body of DepthConsistencyLoss.compute_loss_at_sampled_pose (depth_cons_loss.py:219-321)
// around its two renders as three calls -- project (with the mask and selections of :252-259), select (the visibility threshold of
// :277-283) and loss (:293-312) -- and the gathers that are the backward of the first two.  The arithmetic of a point is dcons.h's; this
// file owns the loops, the ordered compaction and the reductions.
//
// Compaction keeps source order and uses no atomics (ordered.h: ordered_compact_range, in tiles of DCONS_BLOCK consecutive points).  Up
// to DCONS_CHUNK points one workgroup does all of it in one launch; above, a counts launch over chunks of DCONS_CHUNK points and a write
// launch in which each workgroup adds the counts of the chunks before it in chunk order.  The sums of the loss are fixed-order
// (ordered.h: block_totals, sum_parts): a thread adds its points in index order, then the wave, the waves and the chunks in their order.
// No host synchronisation, no readback: `count` stays in device memory.
#include <hip/hip_runtime.h>

#include "dcons.h"
#include "ordered.h"

namespace sparf {

static constexpr int DCONS_WAVES = DCONS_BLOCK / 64;

// ---- what is compacted (the items of ordered_compact_range): `keep(k)` evaluates point k and holds its row, `place(k, j)` writes it
// as output row j with src, `mark(k, j)` leaves dst
struct DconsProjectItem {
    typedef DconsProjectArgs Args;
    typedef DconsSetup Shared;
    const DconsProjectArgs& a;
    const DconsSetup& s;
    float u, v, z;
    __device__ DconsProjectItem(const DconsProjectArgs& a_, const DconsSetup& s_) : a(a_), s(s_), u(0.f), v(0.f), z(0.f) {}
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

struct DconsSelectItem {
    typedef DconsSelectArgs Args;
    typedef int Shared;
    const DconsSelectArgs& a;
    float vis;
    __device__ DconsSelectItem(const DconsSelectArgs& a_, const int&) : a(a_), vis(0.f) {}
    static __device__ void setup(const DconsSelectArgs&, int&) {}
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

// the points [first, end) by one workgroup: -> base + the number kept (in every thread).  `write`: leave the rows, dst and src;
// otherwise count only.
template <class Item>
static __device__ int dcons_compact_range(const typename Item::Args& a, const typename Item::Shared& sh, int first, int end, int base, bool write,
                                          int (*wave_tot)[1]) {
    Item item(a, sh);
    int run[1] = {base};
    ordered_compact_range<DCONS_BLOCK>(item, first, end, write, run, wave_tot);
    return run[0];
}

// n <= DCONS_CHUNK (or no workspace): one workgroup, every tile in turn
template <class Item>
__global__ void __launch_bounds__(DCONS_BLOCK) dcons_compact_single_kernel(typename Item::Args a) {
    __shared__ typename Item::Shared sh;
    __shared__ int wave_tot[DCONS_WAVES][1];
    if (threadIdx.x == 0) Item::setup(a, sh);
    __syncthreads();
    const int total = dcons_compact_range<Item>(a, sh, 0, a.n, 0, true, wave_tot);
    if (threadIdx.x == 0) a.count[0] = total;
}

// n > DCONS_CHUNK, one workgroup per chunk: the number kept of chunk b at ws[b]
template <class Item>
__global__ void __launch_bounds__(DCONS_BLOCK) dcons_compact_counts_kernel(typename Item::Args a) {
    __shared__ typename Item::Shared sh;
    __shared__ int wave_tot[DCONS_WAVES][1];
    if (threadIdx.x == 0) Item::setup(a, sh);
    __syncthreads();
    const int first = (int)blockIdx.x * DCONS_CHUNK;
    const int end = min(a.n, first + DCONS_CHUNK);
    const int total = dcons_compact_range<Item>(a, sh, first, end, 0, false, wave_tot);
    if (threadIdx.x == 0) a.ws[blockIdx.x] = total;
}

// same grid: every workgroup adds the counts of the chunks before it in chunk order and writes its chunk; the last one leaves the count
template <class Item>
__global__ void __launch_bounds__(DCONS_BLOCK) dcons_compact_write_kernel(typename Item::Args a) {
    __shared__ typename Item::Shared sh;
    __shared__ int wave_tot[DCONS_WAVES][1];
    if (threadIdx.x == 0) Item::setup(a, sh);
    __syncthreads();
    int base = 0;
    for (int b = 0; b < (int)blockIdx.x; ++b) base += a.ws[b];
    const int first = (int)blockIdx.x * DCONS_CHUNK;
    const int end = min(a.n, first + DCONS_CHUNK);
    const int total = dcons_compact_range<Item>(a, sh, first, end, base, true, wave_tot);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) a.count[0] = total;
}

static inline int dcons_chunks(int n) { return (n + DCONS_CHUNK - 1) / DCONS_CHUNK; }

template <class Item>
static int launch_compact(const typename Item::Args& a, hipStream_t s) {
    if (a.n <= DCONS_CHUNK || !a.ws) {
        hipLaunchKernelGGL(dcons_compact_single_kernel<Item>, dim3(1), dim3(DCONS_BLOCK), 0, s, a);
        return hipGetLastError() == hipSuccess ? 0 : 2;
    }
    const int chunks = dcons_chunks(a.n);
    hipLaunchKernelGGL(dcons_compact_counts_kernel<Item>, dim3(chunks), dim3(DCONS_BLOCK), 0, s, a);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(dcons_compact_write_kernel<Item>, dim3(chunks), dim3(DCONS_BLOCK), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

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

// n <= DCONS_CHUNK (or no workspace): one workgroup
__global__ void __launch_bounds__(DCONS_BLOCK) dcons_loss_single_kernel(DconsLossArgs a) {
    __shared__ double red[DCONS_WAVES][DCONS_NACC];
    double acc[DCONS_NACC], tot[DCONS_NACC];
    dcons_loss_loop(a, threadIdx.x, a.n, acc);
    block_totals<DCONS_NACC, DCONS_WAVES>(acc, red, tot);
    if (threadIdx.x == 0) dcons_loss_outputs(a, tot);
}
// n > DCONS_CHUNK, one workgroup per chunk: its totals at ws[b]
__global__ void __launch_bounds__(DCONS_BLOCK) dcons_loss_partial_kernel(DconsLossArgs a) {
    __shared__ double red[DCONS_WAVES][DCONS_NACC];
    double acc[DCONS_NACC], tot[DCONS_NACC];
    const int first = (int)blockIdx.x * DCONS_CHUNK;
    dcons_loss_loop(a, first + (int)threadIdx.x, min(a.n, first + DCONS_CHUNK), acc);
    block_totals<DCONS_NACC, DCONS_WAVES>(acc, red, tot);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < DCONS_NACC; ++j) a.ws[(size_t)blockIdx.x * DCONS_NACC + j] = tot[j];
    }
}
// the partial totals added in workgroup order
__global__ void dcons_loss_finish_kernel(DconsLossArgs a, int chunks) {
    double tot[DCONS_NACC];
    sum_parts<DCONS_NACC>(a.ws, chunks, tot);
    dcons_loss_outputs(a, tot);
}

// ---- launchers (api.hip): n > 0
int64_t dcons_workspace_bytes(int n) { return n > DCONS_CHUNK ? (int64_t)dcons_chunks(n) * DCONS_NACC * (int64_t)sizeof(double) : 0; }

int launch_dcons_project(const DconsProjectArgs& a, hipStream_t s) { return launch_compact<DconsProjectItem>(a, s); }
int launch_dcons_select(const DconsSelectArgs& a, hipStream_t s) { return launch_compact<DconsSelectItem>(a, s); }

int launch_dcons_project_bwd(const DconsProjectArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(dcons_project_bwd_kernel, dim3((a.n + DCONS_BLOCK - 1) / DCONS_BLOCK), dim3(DCONS_BLOCK), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
int launch_dcons_select_bwd(const int32_t* dst, const float* d_uv, const float* d_z, int n, float* d_uv_in, float* d_z_in, hipStream_t s) {
    hipLaunchKernelGGL(dcons_select_bwd_kernel, dim3((n + DCONS_BLOCK - 1) / DCONS_BLOCK), dim3(DCONS_BLOCK), 0, s, dst, d_uv, d_z, n, d_uv_in, d_z_in);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
int launch_dcons_loss(const DconsLossArgs& a, hipStream_t s) {
    if (a.n <= DCONS_CHUNK || !a.ws) {
        hipLaunchKernelGGL(dcons_loss_single_kernel, dim3(1), dim3(DCONS_BLOCK), 0, s, a);
        return hipGetLastError() == hipSuccess ? 0 : 2;
    }
    const int chunks = dcons_chunks(a.n);
    hipLaunchKernelGGL(dcons_loss_partial_kernel, dim3(chunks), dim3(DCONS_BLOCK), 0, s, a);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(dcons_loss_finish_kernel, dim3(1), dim3(1), 0, s, a, chunks);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace sparf
