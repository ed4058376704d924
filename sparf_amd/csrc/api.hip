// C ABI of libsparf_hip.so (see include/sparf_hip.h): argument checking, workspace
// carving and kernel sequencing on the caller's stream.  No allocation, no global state.
#include "pass_plan.h"

namespace sparf {
int build_tables(int prec, int32_t* out);
int launch_pack(int prec, const float* const* param_ptrs_host, const int32_t* tables, void* out, hipStream_t s);
int launch_c2f(const float* progress, int has_c2f, float c2f_start, float c2f_end, float* out, hipStream_t s);
int launch_calib_mfma(int iters, float* sink, int grid, hipStream_t s);
int launch_calib_hbm(const void* src, void* dst, int64_t bytes, int mode, float* sink, int grid, hipStream_t s);
int64_t calib_mfma_flops(int iters, int grid);
// pose.hip: one thread per pose, n > 0
int launch_pose_se3_fwd(const float* xi, const float* base, int n, float* refine_out, float* pose_out, hipStream_t s);
int launch_pose_se3_bwd(const float* xi, const float* base, int n, const float* d_pose, const float* d_refine, float* d_xi, float* d_base, hipStream_t s);
int launch_pose_compose_fwd(const float* a, const float* b, int n, float* out, hipStream_t s);
int launch_pose_compose_bwd(const float* a, const float* b, int n, const float* d_out, float* d_a, float* d_b, hipStream_t s);
int launch_pose_d9_fwd(const float* d9, int invert, int n, float* pose_out, hipStream_t s);
int launch_pose_d9_bwd(const float* d9, int invert, int n, const float* d_pose, float* d_d9, hipStream_t s);
// pose_eval.hip
int launch_pose_eval(const float* pose, const float* pose_gt, int gt_sets, int S, int B, int align, float* stats, float* errors, float* aligned,
                     float* sim3, int* best, float* scores, hipStream_t s);
int launch_pose_backtrack(const float* pose_gt_w2c, int n, const float* sim3, int sim3_stride, float* out, hipStream_t s);
}  // namespace sparf

using namespace sparf;

// layout constants, evaluated at compile time (as plain calls the constexpr functions of
// streams.h would re-run their enumeration loops on the host at every API call)
static constexpr int64_t kWsrcOff[N_PREC] = {tbl_wsrc_off(PREC_BF16), tbl_wsrc_off(PREC_FP32), tbl_wsrc_off(PREC_X3)};
static constexpr int64_t kPackedBytes[N_PREC] = {packed_bytes(PREC_BF16), packed_bytes(PREC_FP32), packed_bytes(PREC_X3)};
static constexpr int64_t kTblCount[N_PREC] = {tbl_count(PREC_BF16), tbl_count(PREC_FP32), tbl_count(PREC_X3)};

static inline bool params_ok(const float* const* ptrs) {      // the 20 parameter tensors W0, b0, ..., W9, b9
    for (int i = 0; ptrs && i < 2 * N_LAYERS; ++i)
        if (!ptrs[i]) return false;
    return ptrs != nullptr;
}
// d_center = d_dir = 0 for the rays [first, last)
static int zero_rays(float* d_center, float* d_dir, int first, int last, hipStream_t s) {
    if (first >= last) return 0;
    const size_t off = (size_t)first * 3, bytes = (size_t)(last - first) * 12;
    return hipMemsetAsync(d_center + off, 0, bytes, s) == hipSuccess && hipMemsetAsync(d_dir + off, 0, bytes, s) == hipSuccess ? 0 : 2;
}
static inline int launch_fwd(const FwdLaunch& l, hipStream_t s) { return launch_mlp_fwd(l.prec, l.save, l.a, mlp_grid(l.prec, l.a.rows), s); }
// the data-gradient launch(es) of a plan, in its order
static int launch_dgrad(const BwdPlan& b, hipStream_t s) {
    int rc = 0;
    for (int i = 0; !rc && i < b.ndgrad; ++i) {
        const BwdLaunch& l = b.dgrad[i];
        rc = launch_mlp_bwd(l.k->prec, l.k->pose, l.k->save, l.k->waves, l.a, mlp_grid(l.k->prec, l.n), s);
    }
    return rc;
}

extern "C" {

int sparf_abi_version(void) { return SPARF_ABI_VERSION; }

int64_t sparf_table_count(int prec) { return prec_ok(prec) ? kTblCount[prec] : -1; }
int sparf_build_tables(int prec, int32_t* host_out) { return host_out ? build_tables(prec, host_out) : 1; }

int sparf_stream_nchunks(int prec, int backward) {
    if (!prec_ok(prec)) return -1;
    return backward ? bwd_nchunks(prec) : fwd_nchunks(prec);
}
int sparf_stream_chunk(int prec, int backward, int id, int32_t out[8]) {
    if (!prec_ok(prec) || !out || id < 0 || id >= sparf_stream_nchunks(prec, backward)) return 1;
    const Chunk c = backward ? bwd_chunk(prec, id) : fwd_chunk(prec, id);
    out[0] = c.layer; out[1] = c.seg; out[2] = c.mb0; out[3] = c.nmb; out[4] = c.ks0; out[5] = c.nks;
    out[6] = (int32_t)(backward ? bwd_chunk_off(prec, id) : fwd_chunk_off(prec, id));
    out[7] = chunk_bytes(prec, c);
    return 0;
}

int64_t sparf_packed_bytes(int prec) { return prec_ok(prec) ? kPackedBytes[prec] : -1; }
int sparf_pack_weights(int prec, const float* const* param_ptrs, const int32_t* tables, void* packed_out, void* stream) {
    if (!prec_ok(prec) || !params_ok(param_ptrs) || !tables || !packed_out) return 1;
    return launch_pack(prec, param_ptrs, tables, packed_out, (hipStream_t)stream);
}

int sparf_c2f_weights(const float* progress, int has_c2f, float c2f_start, float c2f_end, float* out16, void* stream) {
    if (!out16 || (has_c2f && (!progress || !(c2f_end != c2f_start)))) return 1;
    return launch_c2f(progress, has_c2f, c2f_start, c2f_end, out16, (hipStream_t)stream);
}

int sparf_sample_coarse(const float* jitter, float u_const, const float* dmax_ray, const float* range_dev, float dmin, float scale,
                        int inverse, int nrays, int nsamp, float* t_out, void* stream) {
    if (nrays == 0 && nsamp > 0) return 0;
    if (nrays < 0 || nsamp <= 0 || !t_out) return 1;
    return launch_sample_coarse(jitter, u_const, dmax_ray, range_dev, dmin, scale, inverse, (int64_t)nrays * nsamp, nsamp, t_out,
                                (hipStream_t)stream);
}

int sparf_sample_fine(const float* weights, const float* t_coarse, const float* u_mid, const float* range_dev, float dmin, float dmax,
                      int nrays, int n_coarse, int n_fine, float* t_fine, float* t_out, void* stream) {
    if (nrays == 0 && n_coarse > 0 && n_fine > 0) return 0;
    if (nrays < 0 || n_coarse <= 0 || n_fine <= 0 || !weights || !t_coarse || !u_mid || !t_out) return 1;
    SampleFineArgs a{nrays, n_coarse, n_fine, weights, t_coarse, u_mid, dmin, dmax, range_dev, t_fine, t_out, {}};
    return launch_sample_fine(a, (hipStream_t)stream);
}

int sparf_sample_fine_hostgrid(const float* weights, const float* t_coarse, const float* u_mid_host, const float* range_dev, float dmin, float dmax,
                               int nrays, int n_coarse, int n_fine, float* t_fine, float* t_out, void* stream) {
    if (nrays == 0 && n_coarse > 0 && n_fine > 0) return 0;
    if (nrays < 0 || n_coarse <= 0 || n_fine <= 0 || n_fine > SAMPLE_FINE_HOST_MAX || !weights || !t_coarse || !u_mid_host || !t_out) return 1;
    SampleFineArgs a{nrays, n_coarse, n_fine, weights, t_coarse, nullptr, dmin, dmax, range_dev, t_fine, t_out, {}};
    for (int i = 0; i < n_fine; ++i) a.u_host[i] = u_mid_host[i];
    return launch_sample_fine(a, (hipStream_t)stream);
}

int sparf_ray_gen_forward(const float* pose, const float* intr, const float* pixels, const int64_t* ray_idx, int per_image,
                          int width, int nimg, int nrays, float* center, float* ray, void* stream) {
    if (nimg >= 0 && nrays == 0) return 0;                      // empty selection: nothing to write
    if (nimg < 0 || nrays < 0 || !pose || !intr || !center || !ray || ((pixels != nullptr) == (ray_idx != nullptr))) return 1;
    if (ray_idx && width <= 0) return 1;
    RayGenArgs a{nimg, nrays, width, per_image, pose, intr, pixels, ray_idx, center, ray};
    return launch_ray_gen_fwd(a, (hipStream_t)stream);
}

int sparf_ray_gen_backward(const float* pose, const float* intr, const float* pixels, const int64_t* ray_idx, int per_image,
                           int width, int nimg, int nrays, const float* d_center, const float* d_ray, float* d_pose,
                           void* stream) {
    if (nimg < 0 || nrays < 0 || !pose || !intr || !d_pose) return 1;
    if (nrays > 0 && ((pixels != nullptr) == (ray_idx != nullptr))) return 1;    // empty selection: d_pose = 0
    if (ray_idx && width <= 0) return 1;
    RayGenArgs a{nimg, nrays, width, per_image, pose, intr, pixels, ray_idx, nullptr, nullptr};
    return launch_ray_gen_bwd(a, d_center, d_ray, d_pose, (hipStream_t)stream);
}

// ---- pose parameterisations (sparf_hip.h): n == 0 launches nothing, whatever the pointers; then the argument checks
// camera.py:142-157 Lie.se3_to_SE3 with its series :180-205, then Pose.compose([refine, base]) :100-115
int sparf_pose_se3_forward(const float* xi, const float* base, int n, float* refine_out, float* pose_out, void* stream) {
    if (n == 0) return 0;
    if (n < 0 || !xi || !pose_out) return 1;
    return launch_pose_se3_fwd(xi, base, n, refine_out, pose_out, (hipStream_t)stream);
}
// what autograd derives from camera.py:142-157, :180-205 and :108-115
int sparf_pose_se3_backward(const float* xi, const float* base, int n, const float* d_pose, const float* d_refine, float* d_xi, float* d_base,
                            void* stream) {
    if (n == 0) return 0;
    if (n < 0 || !xi || !d_pose || !d_xi || (d_base && !base)) return 1;
    return launch_pose_se3_bwd(xi, base, n, d_pose, d_refine, d_xi, d_base, (hipStream_t)stream);
}
// camera.py:108-115 Pose.compose_pair_b_at_a
int sparf_pose_compose_forward(const float* a, const float* b, int n, float* out, void* stream) {
    if (n == 0) return 0;
    if (n < 0 || !a || !b || !out) return 1;
    return launch_pose_compose_fwd(a, b, n, out, (hipStream_t)stream);
}
int sparf_pose_compose_backward(const float* a, const float* b, int n, const float* d_out, float* d_a, float* d_b, void* stream) {
    if (n == 0) return 0;
    if (n < 0 || !a || !b || !d_out || !d_a || !d_b) return 1;
    return launch_pose_compose_bwd(a, b, n, d_out, d_a, d_b, (hipStream_t)stream);
}
// two_columns.py:42-62 r6d2mat and the concatenation of :147-148 / :177-178; invert: camera.py:92-98 Pose.invert
int sparf_pose_d9_forward(const float* d9, int invert, int n, float* pose_out, void* stream) {
    if (n == 0) return 0;
    if (n < 0 || !d9 || !pose_out) return 1;
    return launch_pose_d9_fwd(d9, invert, n, pose_out, (hipStream_t)stream);
}
int sparf_pose_d9_backward(const float* d9, int invert, int n, const float* d_pose, float* d_d9, void* stream) {
    if (n == 0) return 0;
    if (n < 0 || !d9 || !d_pose || !d_d9) return 1;
    return launch_pose_d9_bwd(d9, invert, n, d_pose, d_d9, (hipStream_t)stream);
}

// ---- pose evaluation (sparf_hip.h): S == 0 / n == 0 launch nothing, whatever the pointers; then the argument checks
// joint_pose_nerf_trainer.py:290-311 evaluate_any_poses with :160-254 prealign_w2c_small_camera_systems and :257-287 evaluate_camera_alignment
int sparf_pose_eval(const sparf_pose_eval_t* e, void* stream) {
    if (!e) return 1;
    if (e->S == 0) return 0;
    if (e->S < 0 || e->B < 1 || e->B > SPARF_POSE_EVAL_MAX_POSES || (e->flags & ~SPARF_POSE_EVAL_ALIGN)) return 1;
    if ((e->flags & SPARF_POSE_EVAL_ALIGN) && e->B < 2) return 1;
    if (e->gt_sets != 1 && e->gt_sets != e->S) return 1;
    if (!e->pose || !e->pose_gt || !e->stats || !e->errors || !e->aligned || !e->sim3 || !e->best) return 1;
    return launch_pose_eval(e->pose, e->pose_gt, e->gt_sets, e->S, e->B, e->flags & SPARF_POSE_EVAL_ALIGN, e->stats, e->errors, e->aligned, e->sim3,
                            e->best, e->scores, (hipStream_t)stream);
}
// align_trajectories.py:94-101 backtrack_from_aligning_the_trajectory
int sparf_pose_backtrack(const float* pose_gt_w2c, int n, const float* sim3, int sim3_stride, float* out, void* stream) {
    if (n == 0) return 0;
    if (n < 0 || sim3_stride < 0 || !pose_gt_w2c || !sim3 || !out) return 1;
    return launch_pose_backtrack(pose_gt_w2c, n, sim3, sim3_stride, out, (hipStream_t)stream);
}

int64_t sparf_adam_workspace_floats(void) { return 256; }

int sparf_adam_step(const float* const* params, const float* grad, float* exp_avg, float* exp_avg_sq, float* workspace,
                    float* norm_out, float lr, float beta1, float beta2, float eps, int step, float max_norm, void* stream) {
    if (!params_ok(params) || !grad || !exp_avg || !exp_avg_sq || step < 1 || (max_norm > 0.0f && !workspace)) return 1;
    return launch_adam(params, grad, exp_avg, exp_avg_sq, workspace, norm_out, lr, beta1, beta2, eps, step, nullptr, max_norm, (hipStream_t)stream);
}

int sparf_adam_step_dev(const float* const* params, const float* grad, float* exp_avg, float* exp_avg_sq, float* workspace,
                        float* norm_out, float lr, float beta1, float beta2, float eps, int* step_dev, float max_norm, void* stream) {
    if (!params_ok(params) || !grad || !exp_avg || !exp_avg_sq || !step_dev || (max_norm > 0.0f && !workspace)) return 1;
    return launch_adam(params, grad, exp_avg, exp_avg_sq, workspace, norm_out, lr, beta1, beta2, eps, 0, step_dev, max_norm, (hipStream_t)stream);
}

int sparf_photometric_loss(const float* pred, const float* pred_fine, const float* target, int64_t n, int kind, float delta,
                           float* loss, float* d_pred, float* d_pred_fine, float* workspace, void* stream) {
    if (n <= 0 || !pred || !target || !loss || (kind != 0 && kind != 1) || (kind == 1 && !(delta > 0.0f))) return 1;
    if (d_pred_fine && !pred_fine) return 1;
    return launch_photometric_loss(pred, pred_fine, target, n, kind, delta, loss, d_pred, d_pred_fine, workspace, (hipStream_t)stream);
}
int64_t sparf_photometric_workspace_floats(void) { return photometric_workspace_floats(); }

int64_t sparf_save_bytes(int prec, int64_t rows) {
    const PassPrec pp = pass_prec(prec);
    return pp.ok && rows >= 0 ? align256(save_area_bytes(pp.af, rows)) : -1;
}

int sparf_pass_forward(const sparf_pass_fwd_t* p, void* stream) {
    FwdPlan f;
    int rc = plan_forward(p, &f);
    if (rc || p->nrays == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = launch_ray_setup(f.main.prec, p->dir, p->nrays, p->c2f + 10, p->venc_ws, p->raylen, s);
    if (!rc) rc = launch_fwd(f.main, s);
    if (!rc && f.far_setup) rc = launch_ray_setup(f.far.prec, p->dir, p->nrays, p->c2f + 10, p->far_venc_ws, p->raylen, s);
    if (!rc && f.far_kind != FAR_NONE) rc = launch_fwd(f.far, s);
    if (!rc && f.far_kind == FAR_ROWS && p->save) rc = launch_far_transplant(f.main.prec, f.masks, p->far_ws, p->save, f.far.a.rows, p->far_count, p->nsamp, s);
    if (!rc) rc = launch_composite_fwd(f.c, s);
    return rc;
}

int64_t sparf_bwd_workspace_bytes(int prec, int nrays, int nsamp, int pose) {
    const PassPrec pp = pass_prec(prec);
    if (!pp.ok || nrays < 0 || nsamp <= 0 || (pp.masks && !pose)) return -1;
    return bwd_ws_layout(pp.af, nrays, nsamp, pose).total;
}
int sparf_pass_backward(const sparf_pass_bwd_t* p, void* stream) {
    BwdPlan b;
    int rc = plan_backward(p, false, &b);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool masks = b.pp.masks;                            // ray-gradient-only: grad_params is not touched, no weight gradient runs
    if (b.rows == 0 || b.no_grad) {                           // empty batch, or no upstream gradient at all: zero results
        if (!masks && hipMemsetAsync(p->grad_params, 0, (size_t)N_PARAMS * sizeof(float), s) != hipSuccess) return 2;
        return b.rows && b.pose && !p->accumulate_rays ? zero_rays(p->d_center, p->d_dir, 0, p->nrays, s) : 0;
    }
    rc = launch_composite_bwd(b.c, s);
    // (A chunked schedule -- dgrad of row range c on this stream with a reduced grid, wgrad of range c-1 on a side stream on the CUs
    // left, matrix-pipe-bound against HBM-bound -- was built and measured in round 4: bit-identical gradients, 3.5-13 % SLOWER than
    // this serial order at 2-8 chunks and 32-96 reserved CUs, profiles/r04e_overlap_schedule_sweep.log.  Removed.)
    if (!rc) rc = launch_dgrad(b, s);
    if (!rc && !masks) rc = launch_wgrad(b.pp.base, b.pp.q8, b.g, b.split.nsplit, p->tables + kWsrcOff[b.pp.base], p->grad_params, s);
    if (rc || !b.pose) return rc;
    // rays outside the active range receive no gradient: zero them unless the caller accumulates onto an earlier pass's
    if (!p->accumulate_rays && (zero_rays(p->d_center, p->d_dir, 0, b.ray0, s) || zero_rays(p->d_center, p->d_dir, b.ray1, p->nrays, s))) return 2;
    return launch_ray_reduce(b.r, s);
}

// ---- stand-alone compositing (sparf_hip.h): the compositing kernels of a pass on caller-built per-sample values
int sparf_composite_forward(const sparf_composite_fwd_t* p, void* stream) {
    if (!p || p->nrays < 0 || p->nsamp <= 0) return 1;
    if (p->nrays == 0) return 0;
    if (!rows_ok((int64_t)p->nrays * p->nsamp)) return 4;
    if (!p->dir || !p->t || !p->density || !p->rgb_samples || !p->raylen || !p->weights || !p->rgb || !p->depth || !p->opacity || !p->depth_var ||
        !p->rgb_var || !p->all_cumulated)
        return 1;
    hipStream_t s = (hipStream_t)stream;
    int rc = launch_ray_setup(-1, p->dir, p->nrays, nullptr, nullptr, p->raylen, s);           // |dir| only
    if (rc) return rc;
    CompositeFwdArgs c{p->nrays, p->nsamp, p->t, p->density, nullptr, 0.0f, p->rgb_samples, p->raylen, p->white_bg,
                       p->weights, nullptr, p->rgb, p->depth, p->opacity, p->depth_var, p->rgb_var, p->all_cumulated, {}};
    c.seg.n = 0;
    c.direct = 1;
    return launch_composite_fwd(c, s);
}
int sparf_composite_backward(const sparf_composite_bwd_t* p, void* stream) {
    if (!p || p->nrays < 0 || p->nsamp <= 0) return 1;
    if (p->nrays == 0) return 0;
    if (!rows_ok((int64_t)p->nrays * p->nsamp)) return 4;
    if (!p->dir || !p->t || !p->density || !p->rgb_samples || !p->raylen || !p->weights || !p->d_density || !p->d_rgb_samples) return 1;
    if (p->d_dir && !p->d_len_ws) return 1;
    hipStream_t s = (hipStream_t)stream;
    CompositeBwdArgs c{p->nrays, p->nsamp, p->t, p->density, nullptr, 0.0f, p->rgb_samples, p->raylen, p->weights,
                       p->white_bg, p->g_rgb, p->g_depth, p->g_opacity, p->g_weights, p->d_density, p->d_rgb_samples, p->d_dir ? p->d_len_ws : nullptr, {}, 0};
    c.seg.n = 0;
    c.g_depth_var = p->g_depth_var; c.g_rgb_var = p->g_rgb_var; c.g_all_cum = p->g_all_cumulated;
    c.direct = 1;
    int rc = launch_composite_bwd(c, s);
    if (rc) return rc;
    if (p->d_dir) rc = launch_len_to_dir(p->dir, p->raylen, p->d_len_ws, p->nrays, p->d_dir, s);
    return rc;
}

// the wgrad split of a pass of `rows_total` rows restricted to an active range of `rows_active` rows (host arithmetic only: the
// split_of_range of plan_backward; tests/test_tables_cpu.py checks that it never exceeds what sparf_bwd_workspace_bytes reserved)
int sparf_debug_wgrad_split(int64_t rows_total, int64_t rows_active, int* nsplit_total, int* nsplit_active, int* rows_per_split_active) {
    if (rows_total < 0 || rows_active < 0 || rows_active > rows_total || !nsplit_total || !nsplit_active || !rows_per_split_active) return 1;
    const Split a = split_of_range(rows_total, rows_active);
    *nsplit_total = wgrad_splits(rows_total).nsplit; *nsplit_active = a.nsplit; *rows_per_split_active = a.rows_per_split;
    return 0;
}

// Host arithmetic only (tests): the byte offsets of a backward workspace (pass_plan.h bwd_ws_layout) in the order they are carved,
// out = {gradient area, d_sigma, d_z, d_len, partial blocks, dp, dv, total = sparf_bwd_workspace_bytes}
int sparf_debug_bwd_workspace(int prec, int nrays, int nsamp, int pose, int64_t out[8]) {
    const PassPrec pp = pass_prec(prec);
    if (!pp.ok || nrays < 0 || nsamp <= 0 || !out) return 1;
    const BwdWs w = bwd_ws_layout(pp.af, nrays, nsamp, pose);
    out[0] = w.grad; out[1] = w.d_sigma; out[2] = w.d_z; out[3] = w.d_len; out[4] = w.partial; out[5] = w.dp; out[6] = w.dv; out[7] = w.total;
    return 0;
}
// Host arithmetic only (tests): the launch plan of the bf16x3 data-gradient kernel over `rows` active rows (pass_plan.h x3_dgrad_rows8):
// rows [0, rows8) in 8 waves, [rows8, rows) in 4; `cus` = the CU count the plan was made for (256 where there is no device)
int sparf_debug_x3_dgrad_plan(int64_t rows, int64_t* rows8, int* cus) {
    if (rows < 0 || !rows8 || !cus) return 1;
    *rows8 = x3_dgrad_rows8(rows);
    *cus = num_cus();
    return 0;
}

// one kernel of the plan of a pass; for the backward kernels the plan of the WHOLE pass, whatever its segment table says
int sparf_launch_kernel(int which, const sparf_pass_fwd_t* f, const sparf_pass_bwd_t* p, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (which == 0) {
        FwdPlan fp;
        const int rc = plan_forward(f, &fp);
        return rc || f->nrays == 0 ? rc : launch_fwd(fp.main, s);
    }
    if (which < 1 || which > 4) return 1;
    BwdPlan b;
    const int rc = plan_backward(p, true, &b, which == 3 ? 8 : which == 4 ? 4 : 0);      // 3 / 4: the bf16x3 kernel pinned to its 8-wave / 4-wave geometry
    if (rc || b.rows == 0) return rc;
    if (which == 2 && b.pp.masks) return 1;                              // a ray-gradient-only pass has no weight gradient
    if (which == 2) return launch_wgrad(b.pp.base, b.pp.q8, b.g, b.split.nsplit, p->tables + kWsrcOff[b.pp.base], p->grad_params, s);
    return launch_dgrad(b, s);
}

// ---- calibration (measurement only, sparf_hip.h): fixed kernels that do not change with the renderer's
int64_t sparf_calib_mfma(int iters, float* sink, void* stream) {
    if (iters <= 0 || iters > (1 << 24) || !sink) return -1;
    const int grid = num_cus();
    if ((int64_t)grid * 512 > SPARF_CALIB_SINK_FLOATS) return -1;
    if (launch_calib_mfma(iters, sink, grid, (hipStream_t)stream)) return -2;
    return calib_mfma_flops(iters, grid);
}
int sparf_calib_hbm(const void* src, void* dst, int64_t bytes, int mode, float* sink, void* stream) {
    if (!src || bytes < 1024 || (bytes & 1023) || (mode != 0 && mode != 1) || (mode == 1 && !dst) || !sink) return 1;
    return launch_calib_hbm(src, dst, bytes, mode, sink, 4 * num_cus(), (hipStream_t)stream);
}

}  // extern "C"
