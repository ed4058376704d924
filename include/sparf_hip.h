/* sparf_hip.h -- C ABI of libsparf_hip.so, the MI355X (gfx950) NeRF renderer hot path.
 *
 * The reference (google-research/sparf) is pure PyTorch: it has NO FFI for this path.
 * Each entry point below therefore replaces a Python-level function of the reference
 * (file:line under /root/reference) rather than an existing binding; INTEGRATION.md
 * shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked HOST; tensors are dense fp32
 *     row-major unless a byte blob is stated; `stream` is a hipStream_t passed as void*;
 *   - return value: 0 = ok, non-zero = error code (never throws, never allocates device
 *     memory, keeps no mutable global state; all work is enqueued on `stream`);
 *   - a "pass" is one network (coarse or fine) evaluated on nrays*nsamp sample rows:
 *     ray setup -> fused MLP -> alpha compositing, and its backward;
 *   - rows = nrays * nsamp <= 2^27 per call (return code 4 above; slice larger batches).  The saved-activation
 *     and gradient areas are addressed per 32-row tile block and have no size limit of their own: a training
 *     pass is bounded by memory only (sparf_save_bytes + sparf_bwd_workspace_bytes, ~9 KB per row in bf16).
 *   - prec: 0 = bf16 MFMA operands / fp32 accumulate, 1 = fp32 MFMA (parity mode), 2 = bf16x3 (operands split into
 *     bf16 head + tail, three bf16 MFMAs per product on the forward / data-gradient chains; saved buffers hold the
 *     bf16 head plane, the weight gradient accumulates head products in fp32).  Measured at the 4096-ray BASELINE
 *     shapes against a float64 referee: outputs <= 2.8e-5 with metric depth; with inverse depth
 *     (samples at |p| ~ 1e8) rendered outputs 5e-5 ... 1.1e-4, per-sample values up to 1.2e-2 -- the Python mirror
 *     therefore routes the last samples of every ray of such passes through mode 1 (far rows, below); parameter gradients 7e-3 relative L2 under a random linear loss,
 *     2e-3 under the photometric loss (fp32: 1e-3 / 3e-4).
 */
#ifndef SPARF_HIP_H
#define SPARF_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPARF_ABI_VERSION 7    /* 7: SPARF_SAVE_MASKS on a pass's precision id (ray-gradient-only passes); 6: upstream gradients of EVERY output of a composite (depth_var, rgb_var, all_cumulated, density, rgb_samples) in
                                  sparf_pass_bwd_t / sparf_segment_t; stand-alone sparf_composite_forward / _backward; 5: SPARF_SAVE_Q8 on a pass's precision id; 4: far rows of a pass (the last K samples of every ray through a second precision); 3: ray segments of a pass (sparf_segment_t), tile-block save areas without a 2^31-byte limit,
                                  device-side Adam step counter; 2: band weights per pass, photometric-loss workspace */
#define SPARF_MAX_SEGMENTS 16
#define SPARF_PREC_BF16 0
#define SPARF_PREC_FP32 1
#define SPARF_PREC_X3 2        /* "bf16x3": bf16 MFMA on head + tail operands, three MFMAs per product; outputs within 1e-4 of fp32 at
                                  metric depth (see the note on inverse depth above) */
/* Save format of a training pass (ABI 5), OR-ed onto the `prec` of sparf_pass_forward / sparf_pass_backward / sparf_save_bytes /
 * sparf_bwd_workspace_bytes (every other entry point takes the plain precision id; weights and tables are those of the plain id):
 * SPARF_PREC_BF16 | SPARF_SAVE_Q8 or SPARF_PREC_X3 | SPARF_SAVE_Q8 keeps what the forward saves for the backward (layer inputs) and
 * what the data-gradient kernel hands the weight-gradient kernel (pre-activation gradients) as 8-bit integers on a linear grid
 * with one fp32 step per sample row and vector, x ~ (u - 128) * max|x| / 127, instead of bf16: half of the ~20 GB a 1M-row training
 * step moves through HBM.  The forward arithmetic -- every output of the pass -- and the data gradients (d_center, d_dir) are those
 * of the plain precision bit for bit; the WEIGHT gradients carry ~1.75x the rounding error of the bf16 saves (measured,
 * DESIGN.md 6).  Not combinable with far rows (far_count > 0). */
#define SPARF_SAVE_Q8 16
/* Ray-gradient-only pass (ABI 7), OR-ed onto `prec` in the same four calls, any base precision: a pass whose only differentiable inputs
 * are its rays (pose optimisation against frozen networks).  The forward with save != NULL leaves the ReLU mask words only:
 * sparf_save_bytes(prec | SPARF_SAVE_MASKS, rows) = 9 216 B per 32-row tile (rows padded to 256).  sparf_pass_backward then requires d_center and
 * d_dir (pose = 0 is an error, also from sparf_bwd_workspace_bytes), ignores grad_params (may be NULL), and runs the composite
 * backward, the data gradient and the ray reduce -- no weight gradient; its workspace holds neither a gradient area nor partial
 * blocks.  Every output of the pass and d_center / d_dir are those of the plain precision bit for bit; segments, the active ray range,
 * accumulate_rays, density noise, every upstream gradient and far rows (far_ws: sparf_save_bytes(far_prec | SPARF_SAVE_MASKS, nrays * K))
 * work as in a training pass.  Not combinable with SPARF_SAVE_Q8 (refused like an invalid precision id).  sparf_launch_kernel takes the
 * flag for which = 0, 1, 3, 4 and returns non-zero for 2. */
#define SPARF_SAVE_MASKS 32
#define SPARF_N_LAYERS 10      /* mlp_feat.0..7, mlp_rgb.0..1 */
#define SPARF_N_PARAMS 530052  /* weights + biases of one network, flat (W0,b0,W1,b1,...) */

int sparf_abi_version(void);

/* ---- static layout tables (host) ------------------------------------------------------
 * int32 gather tables describing the packed weight streams; build once per precision on
 * the host, upload, and pass the device copy to sparf_pack_weights / sparf_pass_backward. */
int64_t sparf_table_count(int prec);                       /* number of int32 entries */
int sparf_build_tables(int prec, int32_t* host_out);       /* HOST pointer */

/* introspection of the packed weight streams (used by the layout tests): chunk `id` of the
 * forward (backward=0) or dgrad (backward=1) stream ->
 * out = {layer, segment, first m-block, m-blocks, first k-step, k-steps, byte offset, bytes} */
int sparf_stream_nchunks(int prec, int backward);
int sparf_stream_chunk(int prec, int backward, int id, int32_t out[8]);   /* HOST pointer */

/* ---- weight packing --------------------------------------------------------------------
 * Replaces the implicit use of nn.Linear weights by F.linear in
 * source/models/frequency_nerf.py:162-170, 215-219.
 * param_ptrs: HOST array of 20 device pointers {W0,b0,...,W9,b9} in nn.Linear layout
 * (W_l is [out][in] row-major: 256x63, 256x256 x3, 256x319, 256x256 x2, 257x256,
 * 128x283, 3x128).  Call again whenever a parameter changes. */
int64_t sparf_packed_bytes(int prec);
int sparf_pack_weights(int prec, const float* const* param_ptrs, const int32_t* tables, void* packed_out, void* stream);

/* BARF coarse-to-fine band weights of NeRF.positional_encoding (frequency_nerf.py:248-253):
 * out16 = {w_0..w_9 (points, L=10), w_0..w_3 (view, L=4), 0, 0} from the DEVICE scalar
 * `progress` (no host sync); all ones when has_c2f == 0 (opt.barf_c2f is None; progress may
 * then be NULL).  Not cached anywhere: trainers rewrite progress through `.data` every
 * iteration (nerf_trainer.py:273-275), so each pass is handed the vector computed for it and
 * its backward receives the same one. */
int sparf_c2f_weights(const float* progress, int has_c2f, float c2f_start, float c2f_end, float* out16, void* stream);

/* ---- depth sampling --------------------------------------------------------------------
 * sparf_sample_coarse replaces Graph.sample_depth (source/models/renderer.py:383-419) and
 * Graph.sample_depth_diff_max_range_per_ray (:595-624):
 *   t[r][i] = (u + i)/nsamp * scale + dmin, u = jitter[r][i] or u_const when jitter==NULL
 *   (0.5 for deterministic modes, 1.0 for the per-ray-max variant);
 *   scale = dmax_ray[r] - dmin when dmax_ray != NULL; inverse != 0 -> t = 1/(t + 1e-8).
 * sparf_sample_fine replaces Graph.sample_depth_from_pdf (:421-456) + cat + sort
 * (:334-336): u_mid[n_fine] are the mid-points of the (shared) sampling grid; writes the
 * sorted union [nrays][n_coarse+n_fine] to t_out and, if t_fine != NULL, the unsorted
 * resampled depths [nrays][n_fine].
 * range_dev (both): optional DEVICE pointer to {dmin, dmax} -- trainers hand the renderer
 * data_dict.depth_range[0], a device tensor (renderer.py:97-108); when non-NULL it replaces the
 * float arguments (scale = range_dev[1] - range_dev[0] in fp32, as torch computes it; with
 * dmax_ray only range_dev[0] is read), so no host readback is needed. */
int sparf_sample_coarse(const float* jitter, float u_const, const float* dmax_ray, const float* range_dev, float dmin, float scale,
                        int inverse, int nrays, int nsamp, float* t_out, void* stream);
int sparf_sample_fine(const float* weights, const float* t_coarse, const float* u_mid, const float* range_dev, float dmin, float dmax,
                      int nrays, int n_coarse, int n_fine, float* t_fine, float* t_out, void* stream);
/* (ABI 6) the same with the grid mid-points as a HOST array of n_fine <= 256 floats, copied into the launch arguments at the call:
 * the reference draws the grid on the CPU (renderer.py:439 `torch.rand(n_samples_fine+1)`), and a host -> device copy per render call
 * sits between the kernels of an otherwise copy-free step (round 5 timeline: every such copy was followed by 50-100 us of idle GPU). */
int sparf_sample_fine_hostgrid(const float* weights, const float* t_coarse, const float* u_mid_host, const float* range_dev, float dmin,
                               float dmax, int nrays, int n_coarse, int n_fine, float* t_fine, float* t_out, void* stream);

/* ---- ray generation ----------------------------------------------------
 * Replaces camera.get_center_and_ray / get_center_and_ray_at_pixels
 * (source/utils/camera.py:347-416; img2cam :296-306, cam2world :321-326) for the pixels a
 * render call actually uses (the reference builds all H*W rays of every image and indexes,
 * renderer.py:273-291):  g = K^-1 [x,y,1];  center = -R^T t;  ray = (R^T g + center) - center,
 * un-normalised.  Exactly one of pixels / ray_idx is non-NULL; flat indices address pixel
 * centres (+0.5, camera.py:365-368), explicit pixels are used as given (:400-406);
 * per_image != 0: one row of pixels / indices per image, else one row shared by all images.
 * sparf_ray_gen_backward: d_pose[nimg][3][4] from d_center / d_ray (either may be NULL);
 * intrinsics carry no gradient. */
int sparf_ray_gen_forward(const float* pose, const float* intr, const float* pixels, const int64_t* ray_idx, int per_image,
                          int width, int nimg, int nrays, float* center, float* ray, void* stream);
int sparf_ray_gen_backward(const float* pose, const float* intr, const float* pixels, const int64_t* ray_idx, int per_image,
                           int width, int nimg, int nrays, const float* d_center, const float* d_ray, float* d_pose,
                           void* stream);

/* ---- pose parameterisations --------------------------------------------
 * The bodies of the pose chain of a trainer, one launch per direction each; parameters,
 * optimiser and autograd graph stay the caller's.  One pose per thread, double arithmetic on
 * the fp32 inputs, one rounding per stored value.  n = number of poses; n == 0 returns 0 and
 * launches nothing, n < 0 or a missing required pointer returns 1 before any HIP call.
 *
 * se(3): xi[n][6] = (w, u).  refine = [R | V u] with R = I + A wx + B wx^2,
 * V = I + B wx + C wx^2 and A, B, C the TRUNCATED series of source/utils/camera.py:180-205
 * (nth = 10: 11 terms in |w|^2), as Lie.se3_to_SE3 evaluates them (:142-157) -- polynomials,
 * not sin / cos, so there is no singularity at w = 0.  With base[n][3][4] the result is
 * Pose.compose([refine, base]) (:100-115): R = R_base R_refine, t = R_base t_refine + t_base;
 * without it pose_out = refine.  refine_out (NULL ok) also receives refine.  The backward is
 * the exact vector-Jacobian product of that polynomial function from d_pose and, NULL ok, an
 * upstream gradient on refine; d_base (NULL ok) needs base.
 *
 * compose: out = Pose.compose_pair_b_at_a(a, b) (:108-115), R = R_b R_a, t = R_b t_a + t_b.
 *
 * d9: d9[n][9] = (t, r1, r2) in the order of pose_to_d9
 * (source/models/poses_models/two_columns.py:23-39: the translation, then the two first ROWS
 * of the rotation).  R = r6d2mat(r1, r2) (:42-62), Gram-Schmidt with F.normalize's
 * v / max(|v|, 1e-12); pose = [R | t]; invert != 0: Pose.invert of it (camera.py:92-98, the
 * transpose form) = [R^T | -R^T t]. */
int sparf_pose_se3_forward(const float* xi, const float* base /*NULL ok*/, int n,
                           float* refine_out /*NULL ok*/, float* pose_out, void* stream);
int sparf_pose_se3_backward(const float* xi, const float* base, int n,
                            const float* d_pose, const float* d_refine /*NULL ok*/,
                            float* d_xi, float* d_base /*NULL ok*/, void* stream);
int sparf_pose_compose_forward(const float* a, const float* b, int n, float* out, void* stream);
int sparf_pose_compose_backward(const float* a, const float* b, int n, const float* d_out,
                                float* d_a, float* d_b, void* stream);
int sparf_pose_d9_forward(const float* d9, int invert, int n, float* pose_out, void* stream);
int sparf_pose_d9_backward(const float* d9, int invert, int n, const float* d_pose,
                           float* d_d9, void* stream);

/* ---- correspondence loss ------------------------------------------------
 * The re-projection terms of source/training/core/corres_loss.py, each with its loss, stats,
 * valid mask and gradient seeds from ONE call; the sampler, the renders and the autograd
 * graph stay the caller's.  One term i -> j over n matches
 * (compute_render_and_repro_loss_w_repro_thres :50-95; batch_project_to_other_img,
 * source/utils/geometry/batched_geometry_utils.py:199-228; compute_diff_loss,
 * source/training/core/base_losses.py:197-224), in the reference's operation order:
 *   x = K_i^-1 [p_i, 1] d_i (closed-form inverse of a general 3x3);  h = T [x, 1];
 *   X = h[0:3] / (h[3] + 1e-6);  y = K_j X;  uv = y[0:2] / (y[2] + 1e-6);  e = uv - q_j;
 *   valid = (|e| <= pix_thresh, if pix_check) & (|d_j - X[2]| / (d_j + 1e-6) <= depth_thresh,
 *   if depth_check);  l = sum_c huber_1(e_c) | sum_c |e_c| | sum_c e_c^2 | |e|  for loss_type
 *   0 huber, 1 l1, 2 mse, 3 epe;  loss = sum_k l_k w_k valid_k / (#valid + 1e-6).
 * All per-match arithmetic is double on the fp32 inputs, every sum is accumulated in double in
 * a fixed order (no atomics: two calls on the same inputs give the same bits), each stored
 * value is rounded once.  The checks are detached: gradients go to depth_i and T only.
 *   out[4] = loss, perc_val_pix_rep, perc_val_depth_rep (0 for a check that is off), and the
 *   mean of depth_i (of the first term: depth_in_corr_loss of corres_loss.py:186).
 *   d_depth_i[n], d_T[16] (row 3 carries what the + 1e-6 of the division lets through),
 *   valid[n] (bytes, 0 / 1): NULL ok.  weights[n]: NULL = 1.  depth_j: NULL ok without the
 *   depth check.
 * sparf_reproj_pair_loss is compute_loss_on_image_pair :183-219 for one view pair: from the
 * two w2c poses [3][4] it forms T_self2other = P_other pose_inverse_4x4(P_self)
 * (source/utils/camera.py:37-61) and its inverse, bottom rows exactly [0,0,0,1]; evaluates
 * self -> other and other -> self on the coarse depths and, if both fine depths are given,
 * on those too; out[0] = their sum / 2 (/ 4), out[1..2] the stats of the LAST term (the
 * reference overwrites stats_dict), out[3] = mean(depth_self).  Seeds (NULL ok each): every
 * depth[n], both poses [3][4] through the VJP of the two compositions.
 * workspace: sparf_reproj_workspace_bytes(n) bytes (0 up to 4096 matches: one workgroup, one
 * launch; above, partial totals of up to 64 workgroups per term, two launches; NULL = the
 * one-workgroup path at any n).  n == 0 launches no kernel and zeroes out, d_T and d_pose.
 * Returns 1 before any HIP call for n < 0, an unknown loss_type, the depth check without
 * depth_j, fine depths (or their seeds) for one view only, or a missing required pointer. */
int64_t sparf_reproj_workspace_bytes(int n);
int sparf_reproj_loss(const float* pixels_i, const float* depth_i, const float* K_i, const float* pixels_j,
                      const float* depth_j /*NULL ok*/, const float* K_j, const float* T_itoj, const float* weights /*NULL ok*/,
                      int n, int loss_type, int pix_check, float pix_thresh, int depth_check, float depth_thresh,
                      float* out, float* d_depth_i /*NULL ok*/, float* d_T /*NULL ok*/, unsigned char* valid /*NULL ok*/,
                      void* workspace /*NULL ok*/, void* stream);
int sparf_reproj_pair_loss(const float* pixels_self, const float* pixels_other, const float* depth_self, const float* depth_other,
                           const float* depth_fine_self /*NULL ok*/, const float* depth_fine_other /*NULL ok*/,
                           const float* K_self, const float* K_other, const float* pose_self, const float* pose_other,
                           const float* weights /*NULL ok*/, int n, int loss_type, int pix_check, float pix_thresh,
                           int depth_check, float depth_thresh, float* out, float* d_depth_self, float* d_depth_other,
                           float* d_depth_fine_self, float* d_depth_fine_other, float* d_pose_self, float* d_pose_other,
                           void* workspace /*NULL ok*/, void* stream);

/* ---- depth-consistency loss ---------------------------------------------
 * The body of DepthConsistencyLoss.compute_loss_at_sampled_pose
 * (source/training/core/depth_cons_loss.py:219-321) around its two renders, as three calls;
 * the renders, the pose sampler and the autograd graph stay the caller's.  All per-point
 * arithmetic is double on the fp32 inputs, each stored value is rounded once, no call uses an
 * atomic: two calls on the same inputs give the same bits.
 * sparf_dcons_project replaces :247-259 and, in its back-projecting form, also :209.  Per point:
 *   with points_w[n][3]: X_w = points_w;  otherwise (batch_backproject_to_3d,
 *   source/utils/geometry/batched_geometry_utils.py:244-247)  x = K_ref^-1 [p, 1] d (closed-form
 *   inverse of a general 3x3);  h = T_c2w [x, 1];  X_w = h[0:3] / (h[3] + 1e-6);
 *   then (batch_project, :262-265)  g = P_unseen [X_w, 1];  X = g[0:3] / (g[3] + 1e-6);
 *   y = K_unseen X;  uv = y[0:2] / (y[2] + 1e-6);  z = X[2].
 *   Poses have ref_rows / unseen_rows = 3 or 4 rows of 4; a missing bottom row is [0,0,0,1].
 *   The mask of :252-254 is decided on the values AS STORED (fp32):  uv.x >= 0, uv.y >= 0,
 *   uv.x <= W-1, uv.y <= H-1, z >= depth_min; depth_min_dev (NULL ok) is the same value in
 *   device memory and then depth_min is not read.
 *   Outputs, an ordered compaction (the boolean indexing of :256-259 is stable): uv[count][2]
 *   and z[count] of the surviving points in source order, dst[n] = output row of source point k
 *   or -1, src[count] = source point of output row j, count[1] in device memory.  uv, z and src
 *   need room for n rows.  Exactly one input form: points_w, or all of pixels_ref[n][2],
 *   depth_ref[n], K_ref[3][3], pose_c2w_ref (the others NULL).
 * sparf_dcons_project_backward: what autograd derives from those lines, as a gather over SOURCE
 *   points through dst (no atomics, no zero-fill pass): from d_uv[count][2] and d_z[count]
 *   (NULL ok each: zero) d_points_w[n][3] in the points form, d_depth_ref[n] in the
 *   back-projecting form (the other NULL); zeros where dst < 0.  Nothing goes to K, the poses
 *   or the reference pixels (:172 detaches the poses).
 * sparf_dcons_select replaces :277-283: keep = vis >= thresh as an fp32 compare
 *   (tensor.ge(0.2)), the same ordered compaction of uv[m][2], z[m] and vis[m], with dst, src
 *   and count as above.  sparf_dcons_select_backward gathers d_uv / d_z (NULL ok each: zero)
 *   through dst into d_uv_in[m][2] / d_z_in[m] (NULL ok each: skipped); vis gets no gradient.
 * sparf_dcons_loss replaces :293-312 over the m kept points:  w = vis opacity (detached);
 *   e = z_pseudo - depth;  l = huber_1(e) | |e| | e^2 for loss_type 0 huber, 1 l1, 2 mse
 *   (compute_diff_loss, source/training/core/base_losses.py:197-224; `epe` is not a kernel
 *   case: on a 1-D difference the reference's norm is that of the whole vector);
 *   out[0] = sum l w / (m + 1e-6), plus the same term on depth_fine / opacity_fine when both
 *   are given (NULL ok, together); out[1] = avg_vis_weight = sum w / (m + 1e-6) of the LAST
 *   term (the reference overwrites the variable).  Seeds (NULL ok each) from the same launch:
 *   d_z_pseudo[m], d_depth[m], d_depth_fine[m].  Sums are accumulated in double in a fixed
 *   order.  The division by gamma (:315-319) stays the caller's.
 * workspace: sparf_dcons_workspace_bytes(n) bytes for a call on n points (0 up to 4096 points:
 *   one workgroup, one launch; above, per chunk of 4096 points a count or partial totals, two
 *   launches; NULL = the one-workgroup path at any n).  n == 0 launches no kernel and looks at
 *   no data pointer (an empty tensor has none); project and select then write count = 0, the
 *   loss zeroes out.
 * Each returns 1 before any HIP call for n < 0, an unknown loss_type, neither or both input
 * forms (or a pose with other than 3 or 4 rows), fine depth without fine opacity (or the
 * reverse, or a fine seed without fine depth), or a missing required pointer. */
int64_t sparf_dcons_workspace_bytes(int n);
int sparf_dcons_project(const float* points_w /*NULL ok*/, const float* pixels_ref /*NULL ok*/, const float* depth_ref /*NULL ok*/,
                        const float* K_ref /*NULL ok*/, const float* pose_c2w_ref /*NULL ok*/, int ref_rows,
                        const float* pose_w2c_unseen, int unseen_rows, const float* K_unseen, int n, int H, int W,
                        float depth_min, const float* depth_min_dev /*NULL ok*/, float* uv, float* z, int32_t* dst, int32_t* src,
                        int32_t* count, void* workspace /*NULL ok*/, void* stream);
int sparf_dcons_project_backward(const float* points_w /*NULL ok*/, const float* pixels_ref /*NULL ok*/,
                                 const float* depth_ref /*NULL ok*/, const float* K_ref /*NULL ok*/,
                                 const float* pose_c2w_ref /*NULL ok*/, int ref_rows, const float* pose_w2c_unseen, int unseen_rows,
                                 const float* K_unseen, int n, const int32_t* dst, const float* d_uv /*NULL ok*/,
                                 const float* d_z /*NULL ok*/, float* d_points_w /*NULL ok*/, float* d_depth_ref /*NULL ok*/,
                                 void* stream);
int sparf_dcons_select(const float* vis, const float* uv, const float* z, int m, float thresh, float* uv_out, float* z_out,
                       float* vis_out, int32_t* dst, int32_t* src, int32_t* count, void* workspace /*NULL ok*/, void* stream);
int sparf_dcons_select_backward(const int32_t* dst, const float* d_uv /*NULL ok*/, const float* d_z /*NULL ok*/, int m,
                                float* d_uv_in /*NULL ok*/, float* d_z_in /*NULL ok*/, void* stream);
int sparf_dcons_loss(const float* z_pseudo, const float* vis, const float* depth, const float* opacity,
                     const float* depth_fine /*NULL ok*/, const float* opacity_fine /*NULL ok*/, int m, int loss_type, float* out,
                     float* d_z_pseudo /*NULL ok*/, float* d_depth /*NULL ok*/, float* d_depth_fine /*NULL ok*/,
                     void* workspace /*NULL ok*/, void* stream);

/* ---- photometric, mask and depth-patch loss --------------------------------
 * BasePhotoandReguLoss.compute_loss (source/training/core/base_losses.py:243-323, with the
 * depth-patch regulariser of :180-194 and regularization_losses.py:51-66) and compute_mse_on_rays
 * (source/training/core/metrics.py:33-75) as ONE call on rows = B N rendered rays: it gathers the
 * ground-truth colours and the mask in place and writes every loss term, the two logged MSEs and
 * the gradient seeds.  The distortion loss is not part of it.  Arithmetic as above: double on the
 * fp32 operands, sums in double in a fixed order, one rounding per stored value, no atomic.
 * Gather: the target of ray r of image b, channel c, is image[b][c][idx] (channel-planar, as
 *   data_dict.image is stored) and its mask value fg_mask[b][idx] (bytes 0 / 1: torch.bool
 *   storage), with idx = ray_idx[r] (per_image = 0, one list for all images), ray_idx[b][r]
 *   (per_image = 1) or r itself (ray_idx NULL: full images, N = HW).  Indices may repeat; they lie
 *   in [0, HW) (one outside is clamped, so that the launch stays inside the image).
 * Per element, with e = pred - target:  kind 0 (MSE_loss, :151-153)  l = e^2;  kind 1
 *   (torch.nn.functional.huber_loss with delta; the module's huber_loss, :155-156, is delta 0.5)
 *   l = 0.5 e^2 if |e| <= delta else delta (|e| - 0.5 delta).
 * Mask (:313-319):  l = |fg - opacity|, derivative -sgn(fg - opacity) with sgn(0) = 0.
 * Depth patch: for every P^2 consecutive rays d_0 .. d_{M-1} of an image (M = P^2, N % M == 0)
 *   l = sum_i sum_j sqrt((d_i - d_j)^2 + charbonnier^2) over all M^2 ordered pairs, diagonal
 *   included;  d l / d d_i = 2 sum_j (d_i - d_j) / sqrt((d_i - d_j)^2 + charbonnier^2).
 * out[0] render      kind 0: sum e^2 / (3 rows + 1e-6);  kind 1: 2 sum l / (3 rows);  plus the same
 *                    on rgb_fine when given (:303-311)
 * out[1] fg_mask     0.5 sum |fg - opacity| / rows, plus the same on opacity_fine; 0 without fg_mask
 * out[2] depth_patch 0.02 sum over patches of l / (rows P^2), plus the same on depth_fine; 0 with
 *                    patch = 0
 * out[3], out[4]     mse, mse_fine: sum e^2 / (3 rows) on rgb and rgb_fine (metrics.py:26-31),
 *                    whatever `kind` is; out[4] = 0 without rgb_fine
 * Seeds (NULL ok each: not computed) from the same launch, each the derivative of ITS OWN out[k]:
 *   d_rgb, d_rgb_fine [rows][3] of out[0]; d_opacity, d_opacity_fine [rows] of out[1]; d_depth,
 *   d_depth_fine [rows] of out[2] (zeros when that term is off).  The caller multiplies each by the
 *   upstream scalar of its loss.
 * workspace: sparf_photo_regu_workspace_bytes(rows) bytes (0 up to 4096 rows: one workgroup, one
 *   launch; above, partial totals per chunk of 4096 rows and a second launch that adds them in
 *   chunk order; NULL = the one-workgroup path at any size).  A row sums over its own patch, so no
 *   patch is split between workgroups.  rows == 0 launches nothing and zeroes out.
 * Returns 1 before any HIP call for a negative size, kind outside {0, 1}, patch < 0 or > 8,
 * patch > 0 with N % P^2 != 0 or without depth, a seed without its tensor, fg_mask without
 * opacity, ray_idx NULL with N != HW, or a missing required pointer (image, rgb, out). */
int64_t sparf_photo_regu_workspace_bytes(int64_t rows);
int sparf_photo_regu_loss(const float* image, const unsigned char* fg_mask /*NULL ok*/, const int64_t* ray_idx /*NULL ok*/,
                          int per_image, int B, int HW, int N, const float* rgb, const float* rgb_fine /*NULL ok*/,
                          const float* opacity /*NULL ok*/, const float* opacity_fine /*NULL ok*/, const float* depth /*NULL ok*/,
                          const float* depth_fine /*NULL ok*/, int kind, float delta, int patch, float charbonnier, float* out,
                          float* d_rgb /*NULL ok*/, float* d_rgb_fine /*NULL ok*/, float* d_opacity /*NULL ok*/,
                          float* d_opacity_fine /*NULL ok*/, float* d_depth /*NULL ok*/, float* d_depth_fine /*NULL ok*/,
                          void* workspace /*NULL ok*/, void* stream);

/* ---- correspondence sampler -------------------------------------------------
 * The torch series of a correspondence iteration between "pair chosen" and its two renders
 * (source/training/core/base_corres_loss.py:260-269, :323-328, :365-369 and
 * source/training/core/corres_loss.py:139-155) as two calls.  Integer and copy work: every result
 * equals the reference's bit for bit.  No atomic, no host synchronisation: `count` is device memory.
 * sparf_match_compact replaces the centre mask of :260-269, mask.sum() of :365 / :369 and the row
 *   order of the five boolean selections of corres_loss.py:139-144: pixel p = y W + x of mask[H][W]
 *   (bytes, torch.bool storage, any alignment) is kept if mask[p] != 0 and y0 <= y < y1 and
 *   x0 <= x < x1 -- the half-open window of mask_center[H//2-dH : H//2+dH-1, W//2-dW : W//2+dW-1],
 *   which may be empty; 0, H, 0, W is no window.  index[H W] (int32) receives the flat indices of
 *   the kept pixels in ascending (row-major) order, the order tensor[mask] produces; count[1] their
 *   number; perc[1] (NULL ok) (float)count / (float)(H W + 1e-6), the perc_valid_corr_mask of :369.
 * sparf_match_gather replaces grid[mask], grid_flat[mask], corres[mask], rounded_flat[mask],
 *   conf[mask] (corres_loss.py:139-144), their five gathers by the permutation (:148-155) and the
 *   rounding of base_corres_loss.py:326-328, for k rows: with p = index[sel ? sel[j] : j],
 *   pixels_self[j] = ((float)(p % W), (float)(p / W));  ray_self[j] = p;
 *   pixels_other[j] = (corres[p], corres[corres_channel_stride + p]) -- the map is read in place,
 *   channel-first, as corres_maps[i] is stored;  ray_other[j] = (int64)rint(cy) W + (int64)rint(cx)
 *   of those two values (round half to even, torch.round);  conf_out[j] = conf[p].
 *   sel (int64, what torch.randperm gives; NULL: the first k entries) holds positions in
 *   [0, count); one outside is the caller's error and is clamped against the device count, and an
 *   index entry against H W, so that the launch stays inside the allocations.  No address depends
 *   on a value read from corres: a non-finite correspondence gives a meaningless ray_other, as in
 *   the reference, never a fault.  k == 0 launches nothing and looks at no pointer.
 * workspace: sparf_match_workspace_bytes(H W) bytes (0 up to 4096 pixels: one workgroup, one
 *   launch; above, a count per chunk of 4096 pixels and two launches; NULL = the one-workgroup path
 *   at any size).  H W == 0 launches nothing and writes count = 0, perc = 0.
 * Each returns 1 before any HIP call for a negative size, H W or k above 2^30, a negative channel
 * stride, or a missing required pointer. */
int64_t sparf_match_workspace_bytes(int64_t n);
int sparf_match_compact(const unsigned char* mask, int H, int W, int y0, int y1, int x0, int x1, int32_t* index, int32_t* count,
                        float* perc /*NULL ok*/, void* workspace /*NULL ok*/, void* stream);
int sparf_match_gather(const int32_t* index, const int32_t* count, const int64_t* sel /*NULL ok*/, int k, int H, int W,
                       const float* corres, int64_t corres_channel_stride, const float* conf, float* pixels_self, int64_t* ray_self,
                       float* pixels_other, int64_t* ray_other, float* conf_out, void* stream);

/* ---- DS-NeRF sparse depth loss ----------------------------------------------
 * What SparseCOLMAPDepthLoss.compute_loss (source/training/core/base_losses.py:326-402) runs around
 * its renders, as three calls over all B images.  No atomic; `count` is device memory, which the
 * caller reads back once (the renders need the row counts on the host).
 * sparf_colmap_compact replaces len(torch.where(colmap_depth > 0)[0]) of :367 and the B calls of
 *   torch.where(colmap_depth_i > 1e-6) of :372: depth is colmap_depth [B][1][H][W] as stored
 *   (float32, dense).  index[b][H W] (int32) receives the flat indices p = h W + w of the pixels
 *   of image b with depth > 1e-6f in ascending (row-major) order, the order torch.where produces;
 *   count[b] their number; count[B + b] the number of pixels of image b with depth > 0.0f.
 * sparf_colmap_gather replaces the indexing by the permutation of :378-380, the two map gathers of
 *   :382-383 and ray_idx of :386 for every image in one launch.  Image b holds
 *   k_b = min(count[b], quota) rows; its row j is p = index[b][sel[b][j]] where count[b] > quota
 *   (strictly: a count equal to the quota draws nothing, :377) and sel is given, else
 *   p = index[b][j].  The rows of all images are packed in image order into K = sum k_b entries:
 *   ray_idx (int64) = p, target = depth[b][p], weight = conf[b][p].  sel (int64 [B][quota], what
 *   torch.randperm gives, cut to the quota; NULL: the first rows everywhere) is read only for the
 *   images above the quota.  A position outside [0, count[b]) is the caller's error and is
 *   clamped against the device count, and an index entry against H W, so that the launch stays
 *   inside the allocations; no address depends on a value read from a map.
 * sparf_colmap_loss replaces the weighted means of :391-398 and :400 over the packed rows, with
 *   image boundaries from k_b = min(count[b], quota) (a caller with explicit row counts passes
 *   them as count and quota = 2^30):
 *   out[0] = (0.1 / B) sum_{b: k_b > 0} (1 / k_b) sum_j w_bj ((d_bj - p_bj)^2 [+ (d_bj - pf_bj)^2])
 *   with B counting the skipped images too; d_depth[r] = (0.1 / B)(2 / k_b) w (p - d), likewise
 *   d_depth_fine (either NULL ok).  Double arithmetic on the fp32 operands, sums in a fixed order
 *   (thread, wave butterfly, waves, chunks in chunk order), one rounding per stored value: the
 *   same bits from call to call.
 * workspace: sparf_colmap_workspace_bytes(B, H W, rows) bytes, the larger of what a compaction of
 *   B images of H W pixels and a loss of `rows` rows need (0 up to 4096 pixels / rows: one launch;
 *   above, per-chunk counts / partial sums and two launches; NULL = the one-launch path at any size).
 * Each returns 1 before any HIP call for a negative size, B <= 0 (or above 65535, the grid's y
 * limit), H W or a row count above 2^30, quota < 0, K above B quota, or a missing required pointer;
 * gather and loss return 0 without a launch, looking at no pointer, for K == 0 (out is then not
 * written).  H W == 0 launches nothing and writes count = 0. */
int64_t sparf_colmap_workspace_bytes(int B, int64_t n, int64_t rows);
int sparf_colmap_compact(const float* depth, int B, int H, int W, int32_t* index, int32_t* count, void* workspace /*NULL ok*/, void* stream);
int sparf_colmap_gather(const int32_t* index, const int32_t* count, const int64_t* sel /*NULL ok*/, int B, int H, int W, int quota, int K,
                        const float* depth, const float* conf, int64_t* ray_idx, float* target, float* weight, void* stream);
int sparf_colmap_loss(const float* target, const float* weight, const int32_t* count, int B, int quota, int K, const float* depth,
                      const float* depth_fine /*NULL ok*/, float* out, float* d_depth /*NULL ok*/, float* d_depth_fine /*NULL ok*/,
                      void* workspace /*NULL ok*/, void* stream);

/* ---- depth errors on rendered rays -------------------------------------------
 * compute_depth_error_on_rays (source/training/core/metrics.py:81-134), which the trainers run
 * once per head on every training iteration (nerf_trainer.py:307-325), as ONE call for both heads:
 * no indexed copy of the maps, no index build, no boolean selection and so no readback.
 * depth_gt [B_maps][HW] (float32) and valid [B_maps][HW] (bytes, torch.bool storage; NULL: every
 *   row is kept) are the maps of the whole scene as stored, read in place.
 * Row r of rendered image b (0 <= b < B, 0 <= r < N) reads map m = img_idx[b] (int64, device; NULL:
 *   m = b), clamped to [0, B_maps), at pixel p = ray_idx[r] (per_image 0: one list for all images),
 *   ray_idx[b][r] (per_image 1) or r itself (ray_idx NULL: full images, N == HW), clamped to
 *   [0, HW).  An index outside its range is the caller's error (torch raises on it); the clamps
 *   keep the launch inside the maps.  No address depends on a value read from a map.
 * The row is kept if valid[m][p] != 0.  A kept row contributes |e| and e^2 with
 *   e = depth_gt[m][p] - depth[b][r] s in double on the fp32 operands; s is scale_dev[0] (one float
 *   in device memory) where scale_dev is given, else scale.  depth_fine (NULL ok) is a second
 *   head on the same rows: the map and the mask are read once for both.
 * out[4] = abs_e, rmse, abs_e_fine, rmse_fine with abs_e = sum |e| / (K + 1e-6) and
 *   rmse = sqrt(sum e^2 / K) over the K kept rows, each rounded to float32 once; K == 0 gives
 *   abs_e 0 and rmse NaN, as the reference's mean of an empty selection does; the fine pair is 0
 *   without depth_fine.  count[0] = K.  B N == 0 gives that K == 0 result and reads no input.
 * Sums in double in a fixed order (thread, wave butterfly, waves, chunks in chunk order), no
 *   atomic, no workgroup waits for another: the same bits from call to call.
 * workspace: sparf_ray_depth_err_workspace_bytes(B N) bytes (0 up to 4096 rows: one workgroup, one
 *   launch; above, five doubles per chunk of 4096 rows and two launches; NULL = the one-workgroup
 *   path at any size).
 * Returns 1 before any HIP call for a negative size, B_maps <= 0, B HW or B N above 2^30,
 * per_image outside {0, 1}, or, when there are rows, ray_idx NULL with N != HW (the empty index
 * list of a call without rows has no address), a missing required pointer (depth_gt, depth, out,
 * count) or HW == 0. */
int64_t sparf_ray_depth_err_workspace_bytes(int64_t rows);
int sparf_ray_depth_err(const float* depth_gt, const unsigned char* valid /*NULL ok*/, const int64_t* img_idx /*NULL ok*/,
                        const int64_t* ray_idx /*NULL ok*/, int per_image, int B_maps, int B, int HW, int N,
                        const float* depth, const float* depth_fine /*NULL ok*/, float scale, const float* scale_dev /*NULL ok*/,
                        float* out, int32_t* count, void* workspace /*NULL ok*/, void* stream);

/* ---- depth-consistency front end and ray sampler ------------------------------
 * sparf_pick_pixels: the pixels of sample_rays / sample_rays_for_patch / RaySamplingStrategy.__call__
 * (source/training/core/sampling_strategies.py:132-296) from permutation prefixes already on the
 * device, ONE launch, one thread per output row.
 * perm_a [n_a], perm_b [n_b] (int64, device; NULL with a count of 0) index two rectangular pools
 *   given by value: pool A is the grid [0,a_w) x [0,a_h), index i -> (i % a_w, i / a_w); pool B is
 *   the box of b_w x b_h pixels at (b_x0, b_y0), row-major (the reference's linspace centre box).
 *   An entry outside [0, pool size) is the caller's error; it is clamped into the pool.
 * Rows: the picks of A, then the picks of B, each expanded by the patch x patch offsets (dy outer,
 *   dx inner): (n_a + n_b) patch^2 rows.  pixels [rows][2] float32 (x, y) and / or rays [rows] int64
 *   = y W + x; either may be NULL (both NULL, or no row: nothing is launched, returns 0).
 * Returns 1 before any HIP call for a negative count, W <= 0, patch outside [1, 1024], more than
 * 2^30 rows, or a pool with picks that has no permutation, a negative origin, no pixel, more than
 * 2^30 pixels, or whose origin + width + patch - 1 exceeds W.
 *
 * sparf_unseen_pose: DepthConsistencyLoss.sample_pose (depth_cons_loss.py:45-63) with the pose
 * preparation in front of it (:103-106, :168-174), ONE launch of one wave.
 * poses_w2c [B][row_floats] float32, row_floats 12 ([B,3,4]) or 16 ([B,4,4]).
 * Camera centres -R^T t in float32; angular distances acos(clip(u_self . u_j, -1, 1)),
 *   u = v / (|v| + 1e-6), in double on the float32 centres; the self entry is 1e3; id_other = the
 *   first index of the minimum (B == 1: 0).
 * pose_w2c_ref = poses_w2c[id_self] as a 4 x 4, pose_c2w_ref its transpose inverse, pose_c2w_other
 *   the transpose inverse of poses_w2c[id_other], pose_w2c_at_unseen the transpose inverse of
 *   w c2w_ref + one_minus_w c2w_other (element-wise: two rounded products, one rounded sum).
 * Returns 1 before any HIP call for row_floats outside {12, 16}, B < 1 or above 2^20, id_self
 * outside [0, B) or a missing pointer. */
int sparf_pick_pixels(const int64_t* perm_a /*NULL ok*/, int n_a, const int64_t* perm_b /*NULL ok*/, int n_b, int a_w, int a_h,
                      int b_x0, int b_y0, int b_w, int b_h, int W, int patch, float* pixels /*NULL ok*/, int64_t* rays /*NULL ok*/,
                      void* stream);
int sparf_unseen_pose(const float* poses_w2c, int row_floats, int B, int id_self, float w, float one_minus_w, float* pose_w2c_ref,
                      float* pose_c2w_ref, float* pose_c2w_other, float* pose_w2c_at_unseen, int32_t* id_other, void* stream);

/* ---- evaluation metrics ----------------------------------------------------
 * compute_metrics / compute_metrics_masked / compute_depth_error (source/training/core/metrics.py:
 * 136-268, called per head by source/training/base.py:475-499 and nerf_trainer.py:387-405) with the
 * SSIM of third_party/pytorch_ssim/ssim.py:8-50 (window 11, sigma 1.5, padding 5, size_average) as
 * ONE call on B images of H x W, three channels: one or two predictions against one ground truth.
 * LPIPS is not part of it.  Arithmetic as above: double on the fp32 operands, sums in double in a
 * fixed order (thread, wave butterfly, waves, tiles in tile order), one rounding per stored value,
 * no atomic, no host synchronisation: the same bits from call to call.
 * Operands are read in place by ELEMENT strides, none negative: the images by (batch, channel, row,
 *   column) -- a channel-last render under a permuted [B,3,H,W] view and a channel-first ground
 *   truth alike --, fg_mask [B][H][W] (bytes 0 / 1) by (batch, row, column), the depth rows
 *   [B][H W] by (batch, pixel).  pred_fine NULL: one head.
 * SSIM: the 11 x 11 window runs separably (rows, then columns) over the five moment maps, zero
 *   outside the image.  With fg_mask both images are composited first, x m + (1 - m), and padded
 *   with zero after that (metrics.py:208-212).
 * Depth (metrics.py:158-184): over the pixels with valid_depth_gt != 0 (NULL: every pixel),
 *   e = depth_gt - s depth at s = 1 and at s = depth_scale.
 * out[2][10], one row per head: mse, psnr = -10 log10 mse, ssim -- means over all 3 B H W
 *   elements --; mse_masked (over the foreground elements), psnr_masked, ssim_masked (the mean of
 *   the composites' SSIM map); abs_e = sum |e| / (n + 1e-6), rmse = sqrt(sum e^2 / n) at s = 1;
 *   abs_e_scaled, rmse_scaled at depth_scale.  mse == 0 gives psnr +inf; no foreground pixel gives
 *   mse_masked and psnr_masked NaN; no valid pixel gives abs_e 0 and rmse NaN; what was not asked
 *   for (no second head, no mask, no depth of that head) is NaN.
 * counts[2]: foreground pixels, valid depth pixels (0 without fg_mask / depth_gt).
 * workspace: sparf_image_metrics_workspace_bytes(B, H, W) bytes -- the partial totals of every
 *   16 x 32 tile --, 0 for sizes the call refuses.  Two launches: the tiles, then their sum.
 * Returns 1 before any HIP call for a NULL argument or required pointer (pred, gt, out, counts,
 * workspace), B, H or W < 1, B H W above 2^30, a negative stride, depth or depth_fine without
 * depth_gt, depth_fine without pred_fine, or workspace_bytes below what the size needs. */
typedef struct {
    int B, H, W;
    const float* pred;                      int64_t pred_stride[4];
    const float* pred_fine; /*NULL ok*/     int64_t pred_fine_stride[4];
    const float* gt;                        int64_t gt_stride[4];
    const unsigned char* fg_mask; /*NULL ok*/        int64_t fg_mask_stride[3];
    const float* depth; /*NULL ok*/         int64_t depth_stride[2];
    const float* depth_fine; /*NULL ok*/    int64_t depth_fine_stride[2];
    const float* depth_gt; /*NULL ok*/      int64_t depth_gt_stride[2];
    const unsigned char* valid_depth_gt; /*NULL ok*/ int64_t valid_depth_gt_stride[2];
    float depth_scale;
    float* out;                             /* [2][10] */
    int32_t* counts;                        /* [2] */
    void* workspace;
    int64_t workspace_bytes;
} sparf_image_metrics_t;
int64_t sparf_image_metrics_workspace_bytes(int B, int H, int W);
int sparf_image_metrics(const sparf_image_metrics_t* m, void* stream);

/* ---- pose evaluation ---------------------------------------------------
 * CommonPoseEvaluation.evaluate_any_poses (source/training/joint_pose_nerf_trainer.py:290-311)
 * with prealign_w2c_small_camera_systems (:160-254, its alignment_function :173-213) and
 * evaluate_camera_alignment (:257-287, rotation_distance of source/utils/camera.py:466-471) as
 * ONE launch on S sets of B world-to-camera poses; and backtrack_from_aligning_the_trajectory
 * (source/utils/geometry/align_trajectories.py:94-101) as one more.  Arithmetic as above: double
 * on the fp32 operands, one rounding per stored value, no atomic, no host synchronisation: the
 * same bits from call to call.
 * Candidates: every ordered pair (a, b), a != b, of the first n = min(B, 10) views, a outermost
 *   (:233-236); candidate p scales the estimated camera centres by |c_gt[a] - c_gt[b]| /
 *   |c[a] - c[b]|, applies T = GT_c2w[a] o inverse(scaled[a]) to all B poses and scores the
 *   result by (mean rotation error in degrees, mean centre distance, their product), means in
 *   index order.  The rotation error clamps at the reference's bound as its fp32 tensor holds
 *   it, (float)(1 - 1e-7).  The choice is np.argmin on the products (:249): the lowest index
 *   that is NaN if any is, otherwise the lowest index of the minimum.
 * flags: SPARF_POSE_EVAL_ALIGN runs the search; without it (n_first_fixed_poses > 1, :219-223, or
 *   a bare evaluate_camera_alignment) the aligned poses are the inputs, the similarity is the
 *   identity with s = 1, and best is -1.
 * pose[S][B][12]; pose_gt[gt_sets][B][12] with gt_sets 1 (shared) or S.
 * stats[S][4]: error_R_before_align (degrees), error_t_before_align, error_R (degrees), error_t
 *   (:299-311).  errors[S][2][B][2]: before / after alignment x (rotation error in radians,
 *   centre distance) of every pose.  aligned[S][B][12]: the chosen candidate's aligned
 *   world-to-camera poses.  sim3[S][13]: its R (9, rows), t (3) and s, the reference's
 *   ssim_est_gt_c2w (:210-211).  best[S]: its index.  scores[S][90][3] (NULL ok): the triple of
 *   every candidate; rows from n (n - 1) on are left untouched.
 * Returns 0 without a launch for S == 0; 1 before any HIP call for a NULL struct or required
 * pointer, S or B < 0, B == 0, B > 64 (SPARF_POSE_EVAL_MAX_POSES: the caller takes another path),
 * gt_sets not 1 or S, an unknown flag, or SPARF_POSE_EVAL_ALIGN with B < 2. */
#define SPARF_POSE_EVAL_ALIGN 1
#define SPARF_POSE_EVAL_MAX_POSES 64
#define SPARF_POSE_EVAL_MAX_PAIRS 90
typedef struct {
    const float* pose;
    const float* pose_gt;
    int gt_sets;
    int S, B, flags;
    float* stats;
    float* errors;
    float* aligned;
    float* sim3;
    int32_t* best;
    float* scores; /*NULL ok*/
} sparf_pose_eval_t;
int sparf_pose_eval(const sparf_pose_eval_t* e, void* stream);
/* align_trajectories.py:94-101 on n poses, forward only (the reference runs it under no_grad on
 * ground-truth poses): out = invert([R^T R_c | (R^T / s) (t_c - t)]), [R_c | t_c] =
 * invert(pose_gt_w2c).  sim3: 13 floats (R rows, t, s) on the device, every sim3_stride floats
 * (0: one similarity for all poses).  n == 0 returns 0 without a launch; n < 0, a negative
 * stride or a missing pointer returns 1. */
int sparf_pose_backtrack(const float* pose_gt_w2c, int n, const float* sim3, int sim3_stride,
                         float* out, void* stream);

/* ---- optimiser step ----------------------------------------------------
 * torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm) (source/training/base.py:96-97,
 * engine after_backward; skipped when max_norm <= 0) followed by torch.optim.Adam.step()
 * (source/training/nerf_trainer.py:181-185: betas, eps, no weight decay / amsgrad) for ONE
 * network: params = the 20 tensors W0,b0,...,W9,b9 (updated in place), grad = the flat
 * N_PARAMS gradient written by sparf_pass_backward, exp_avg / exp_avg_sq = flat Adam state,
 * step = 1-based update count, workspace = sparf_adam_workspace_floats() floats,
 * norm_out (optional) receives the gradient norm before clipping. */
int64_t sparf_adam_workspace_floats(void);
int sparf_adam_step(const float* const* params, const float* grad, float* exp_avg, float* exp_avg_sq, float* workspace,
                    float* norm_out, float lr, float beta1, float beta2, float eps, int step, float max_norm, void* stream);
/* the same update with the step count kept on the DEVICE: *step_dev (int32, start at 0) is advanced by the call and
 * Adam's bias corrections are computed from it in the kernel.  For training steps captured in a hipGraph, whose
 * replays repeat the launch arguments verbatim (a host-side step number would freeze at its capture value). */
int sparf_adam_step_dev(const float* const* params, const float* grad, float* exp_avg, float* exp_avg_sq, float* workspace,
                        float* norm_out, float lr, float beta1, float beta2, float eps, int* step_dev, float max_norm, void* stream);

/* BaseLoss.MSE_loss (kind 0) / huber_loss with delta (kind 1) of source/training/core/base_losses.py:151-156
 * on pred[n] and, if non-NULL, pred_fine[n] against target[n], summed as in base_losses.py:303-311;
 * writes the scalar loss and (where non-NULL) its derivatives w.r.t. pred / pred_fine.  workspace:
 * sparf_photometric_workspace_floats() floats (may be NULL for n <= 65536: single-workgroup path);
 * larger inputs (full images) are reduced by up to 256 workgroups in a fixed order. */
int64_t sparf_photometric_workspace_floats(void);
int sparf_photometric_loss(const float* pred, const float* pred_fine, const float* target, int64_t n, int kind, float delta,
                           float* loss, float* d_pred, float* d_pred_fine, float* workspace, void* stream);

/* ---- ray segments of a pass -------------------------------------------------
 * The SPARF losses issue 5-6 independent render calls per iteration (corres_loss.py:158-166,
 * depth_cons_loss.py:192,267,291).  Rays are independent, so several calls can share ONE pass: their rays
 * sit back to back in the pass's ray buffers (ray generation and depth sampling write each call's rows at
 * its offset) and a segment table tells the per-ray kernels what differs per call: the density-noise
 * scale (noise only on train-mode calls, frequency_nerf.py:191-192) and, in the backward, where each
 * call's upstream gradients live (autograd hands them over per call: no gather / scatter copies).
 * nseg == 0: the pass is one segment described by the pass-level fields.  Segments must tile
 * [0, nrays) in order.  HOST array, at most SPARF_MAX_SEGMENTS entries, copied at the call. */
typedef struct {
    int ray0, nrays;           /* rays [ray0, ray0 + nrays) of the pass */
    float noise_scale;         /* this segment's density-noise scale (0: no noise even if the pass has a noise tensor) */
    const float *g_rgb, *g_depth, *g_opacity, *g_weights;   /* backward only: THIS segment's upstream gradients
                                                               ([nrays][3], [nrays], [nrays], [nrays][nsamp]) or NULL */
    /* (ABI 6) ... and of the other outputs of the composite: [nrays] x 3, [nrays][nsamp], [nrays][nsamp][3], or NULL */
    const float *g_depth_var, *g_rgb_var, *g_all_cumulated, *g_density, *g_rgb_samples;
} sparf_segment_t;

/* ---- one network pass, forward ---------------------------------------------------------
 * Replaces NeRF.forward_samples + NeRF.composite
 * (source/models/frequency_nerf.py:260-281, 172-226, 283-343; camera.py:418-437). */
typedef struct {
    int prec, nrays, nsamp;
    const float* center;       /* [nrays][3] ray origins */
    const float* dir;          /* [nrays][3] ray directions, unnormalised */
    const float* t;            /* [nrays][nsamp] sample depths */
    const float* noise;        /* [nrays][nsamp] N(0,1) draws or NULL (frequency_nerf.py:191-192) */
    float noise_scale;         /* opt.nerf.density_noise_reg */
    int white_bg;              /* opt.nerf.setbg_opaque or opt.mask_img (frequency_nerf.py:337-338) */
    const void* packed;        /* sparf_pack_weights output for this network */
    const float* c2f;          /* [16] sparf_c2f_weights output for this pass */
    void* save;                /* sparf_save_bytes() bytes to keep for backward, or NULL (inference) */
    void* venc_ws;             /* scratch: nrays * 32 * (prec==0 ? 2 : 4) bytes */
    /* outputs */
    float* raylen;             /* [nrays] |dir| */
    float* sigma_raw;          /* [nrays][nsamp] density before noise/softplus */
    float* rgb_samples;        /* [nrays][nsamp][3] */
    float* density;            /* [nrays][nsamp] softplus(raw + noise) */
    float* weights;            /* [nrays][nsamp] */
    float* rgb;                /* [nrays][3] */
    float *depth, *opacity, *depth_var, *rgb_var, *all_cumulated;   /* [nrays] */
    int nseg;                  /* 0, or the number of ray segments */
    const sparf_segment_t* seg;   /* HOST array [nseg] (only ray0, nrays, noise_scale are read here) */
    /* far rows (ABI 4): far_count = K > 0 sends the LAST K samples of every ray through the kernels of far_prec as well -- a
     * second fused-MLP launch over nrays*K rows whose raw density / colour replace the main launch's for those samples before
     * compositing.  For inverse-depth sampling (source/models/renderer.py:413-416: sample i sits at t = 1/(1 - (u+i)/N + 1e-8),
     * the last one at t = N/(1-u), up to 1e8; after the merge of renderer.py:334-336 the last coarse samples are still the last
     * samples of the fine pass) under prec 2: the network is evaluated at |p| ~ t, a head + tail operand loses 8 bits against
     * fp32 there, and the samples at large t are where the rendered outputs miss 1e-4 (profiles/r04_inverse_routing_study.json:
     * all rows bf16x3 1.1e-4, last sample fp32 6.8e-5, last 8 samples fp32 1.2e-5).  0 < K < nsamp; far_prec must be 1 (fp32: the
     * kernels row routing is compiled into) and prec 0 or 2.  far_packed: the weights packed for far_prec; far_venc_ws: scratch of
     * nrays * 32 * 4 bytes; far_ws (training passes, save != NULL): scratch of sparf_save_bytes(far_prec, nrays*K) bytes, free
     * again when the call's work has run: what the far launch saved there -- activations and ReLU masks of the far rows -- is copied
     * into `save` at those rows (rounded to the main precision's bf16 plane), so that sparf_pass_backward, which knows nothing
     * about far rows, differentiates the forward that was composited: same operands as for every other row, the fp32 forward's
     * ReLU decisions. */
    int far_count, far_prec;
    const void* far_packed;
    void* far_ws;
    void* far_venc_ws;
    /* far_count = -1: far TILES by value, inference passes only (save == NULL), nsamp % 32 == 0, prec 2 only (the two launches must
     * cut the rows into the same 128-row workgroup tiles: prec 0 runs 256-row tiles and is refused), depth samples increasing along
     * every ray: each 128-row tile whose largest depth sample exceeds far_thr is evaluated by the far_prec kernel, every other tile
     * by the prec kernel -- for render_to_max passes (renderer.py:595-624: samples up to a per-ray far bound, so "the last K
     * samples" means nothing) under inverse depth: a ray is rendered up to a depth that is usually small, and only where it is
     * not does the pass need fp32. */
    float far_thr;
} sparf_pass_fwd_t;
int64_t sparf_save_bytes(int prec, int64_t rows);
int sparf_pass_forward(const sparf_pass_fwd_t* a, void* stream);

/* ---- one network pass, backward --------------------------------------------------------
 * Replaces torch.autograd through the functions above.  Upstream gradients may be NULL
 * (treated as zero).  grad_params receives d loss / d (W0,b0,...) flat, SPARF_N_PARAMS
 * floats.  d_center / d_dir (both or neither) request the gradients w.r.t. the rays
 * (joint pose optimisation); depth samples, `progress` and the noise receive none, as in
 * the reference (renderer.py:323 no_grad, frequency_nerf.py:251 .data). */
typedef struct {
    int prec, nrays, nsamp;
    const float *center, *dir, *t, *noise;
    float noise_scale;
    int white_bg;
    const void* packed;
    const float* c2f;          /* the vector the forward of this pass was given */
    const int32_t* tables;     /* device copy of sparf_build_tables output */
    const void* save;          /* written by sparf_pass_forward */
    const float *raylen, *sigma_raw, *rgb_samples, *weights;   /* forward outputs */
    const float *g_rgb, *g_depth, *g_opacity, *g_weights;      /* [nrays][3], [nrays], [nrays], [nrays][nsamp] */
    void* ws;                  /* sparf_bwd_workspace_bytes() bytes */
    float* grad_params;        /* [SPARF_N_PARAMS] */
    float *d_center, *d_dir;   /* [nrays][3] or NULL */
    int nseg;                  /* 0 (g_* above cover the whole pass), or the number of ray segments: then the */
    const sparf_segment_t* seg;   /* upstream gradients are read per segment from this HOST array [nseg] */
    /* (ABI 6) NeRF.composite is plain autograd in the reference: EVERY key it returns carries a gradient
     * (source/models/frequency_nerf.py:317-338).  Upstream gradients of depth_var / rgb_var / all_cumulated [nrays], of the
     * per-sample density [nrays][nsamp] (after softplus) and colour [nrays][nsamp][3] (after the sigmoid); any may be NULL. */
    const float *g_depth_var, *g_rgb_var, *g_all_cumulated, *g_density, *g_rgb_samples;
    /* (ABI 6) != 0: d_center / d_dir are ADDED to what the buffers hold (the fine pass of a render on top of its coarse pass: both
     * passes differentiate the same rays, source/models/renderer.py:304-343) */
    int accumulate_rays;
} sparf_pass_bwd_t;
int64_t sparf_bwd_workspace_bytes(int prec, int nrays, int nsamp, int pose);
int sparf_pass_backward(const sparf_pass_bwd_t* a, void* stream);

/* ---- stand-alone compositing (ABI 6) -----------------------------------------------------
 * NeRF.composite (source/models/frequency_nerf.py:283-343) as a function of caller-built per-sample values: `density`
 * [nrays][nsamp] (already through softplus), `rgb_samples` [nrays][nsamp][3] (already through the sigmoid), depth samples `t`
 * [nrays][nsamp], ray directions `dir` [nrays][3] (only their length enters: dist = delta * |dir|, :302-308).  The fused pass
 * above composites its own samples; this entry point serves callers that evaluate the network themselves (NeRF.forward /
 * forward_samples on explicit points) and composite afterwards.  Outputs as in sparf_pass_fwd_t; raylen [nrays] is written too.
 * Backward: upstream gradients of all seven outputs (any may be NULL) -> d_density [nrays][nsamp], d_rgb_samples [nrays][nsamp][3],
 * d_dir [nrays][3] (NULL to skip).  The depth samples receive no gradient (they carry none anywhere in the reference's callers:
 * renderer.py:323 no_grad, :405-407 fresh draws); the Python mirror refuses depth samples that require one. */
typedef struct {
    int nrays, nsamp, white_bg;
    const float *dir, *t, *density, *rgb_samples;
    float *raylen, *weights, *rgb, *depth, *opacity, *depth_var, *rgb_var, *all_cumulated;
} sparf_composite_fwd_t;
int sparf_composite_forward(const sparf_composite_fwd_t* a, void* stream);
typedef struct {
    int nrays, nsamp, white_bg;
    const float *dir, *t, *density, *rgb_samples, *raylen, *weights;       /* raylen, weights: written by the forward */
    const float *g_rgb, *g_depth, *g_opacity, *g_weights, *g_depth_var, *g_rgb_var, *g_all_cumulated;
    float *d_density, *d_rgb_samples;      /* [nrays][nsamp], [nrays][nsamp][3] */
    float *d_dir;                          /* [nrays][3] or NULL */
    float *d_len_ws;                       /* scratch [nrays] (needed when d_dir != NULL) */
} sparf_composite_bwd_t;
int sparf_composite_backward(const sparf_composite_bwd_t* a, void* stream);

/* ---- single-kernel entry points (measurement only) --------------------------------------
 * Launch exactly one of the three heavy kernels of a pass with the arguments the pass-level
 * calls would give it, so that bench.py can time each with stream events and rocprofv3 can
 * be cross-checked kernel by kernel.  which: 0 = fused MLP forward (saves activations iff
 * fwd->save != NULL), 1 = fused MLP dgrad, 2 = wgrad (+ its reduce kernel); 3 / 4 = the dgrad
 * kernel pinned to its 256-row (8 waves) / 128-row (4 waves) workgroup geometry -- bf16x3 has both
 * and sparf_pass_backward picks one per launch from the row count; other modes ignore the pin.
 * For 1 - 4 the workspace must already hold d_sigma / d_z (i.e. a full sparf_pass_backward ran). */
int sparf_launch_kernel(int which, const sparf_pass_fwd_t* fwd, const sparf_pass_bwd_t* bwd, void* stream);

/* ---- calibration (measurement only) -----------------------------------------------------
 * Two fixed kernels that know nothing of the renderer (csrc/calib.hip), for bench.py to time before and after its measurement:
 * the renderer's kernels change from round to round, these do not: they say what state (clocks under the power cap) a lease
 * found the chip in.  No reference counterpart (the reference has no device code).
 * sparf_calib_mfma: `iters` x 16 back-to-back v_mfma_f32_32x32x16_bf16 per wave on operands with random bits, two waves per SIMD on
 *   every CU; returns the bf16 flops the launch issues (> 0), or < 0 on bad arguments / launch failure.
 * sparf_calib_hbm: mode 0 = read [src, src + bytes) once through LDS-DMA (global_load_lds_dwordx4 nt, the weight-gradient kernel's
 *   operand path); mode 1 = copy it to dst (16-byte loads, non-temporal stores).  bytes: a multiple of 1024.
 * sink: SPARF_CALIB_SINK_FLOATS floats of device memory (never written in practice; keeps the kernels' results alive). */
#define SPARF_CALIB_SINK_FLOATS (1 << 18)
int64_t sparf_calib_mfma(int iters, float* sink, void* stream);
int sparf_calib_hbm(const void* src, void* dst, int64_t bytes, int mode, float* sink, void* stream);

/* Host arithmetic only (tests): the split-K decomposition sparf_pass_backward uses for the weight gradient of a pass of
 * rows_total sample rows whose active range (segments with an upstream gradient) covers rows_active rows.  nsplit_total is
 * what sparf_bwd_workspace_bytes reserved partial blocks for; nsplit_active <= nsplit_total always holds. */
int sparf_debug_wgrad_split(int64_t rows_total, int64_t rows_active, int* nsplit_total, int* nsplit_active, int* rows_per_split_active);
/* Host arithmetic only (tests): byte offsets inside the workspace of sparf_pass_backward, in the order they are carved:
 * out = {gradient area, d_sigma, d_z, d_len, split-K partial blocks, dp, dv, total}; total = sparf_bwd_workspace_bytes; dp == dv ==
 * total for a pass without pose gradients.  `prec` may carry SPARF_SAVE_Q8. */
int sparf_debug_bwd_workspace(int prec, int nrays, int nsamp, int pose, int64_t out[8]);
/* Host arithmetic only (tests): the launch plan of the bf16x3 data-gradient kernel over `rows` active rows: the leading *rows8 rows
 * (0, rows, or a whole number of rounds of 256-row tiles over *cus compute units) run in the 8-wave kernel, the rest in the 4-wave
 * kernel.  *cus is the compute-unit count of the current device, 256 where there is none. */
int sparf_debug_x3_dgrad_plan(int64_t rows, int64_t* rows8, int* cus);

#ifdef __cplusplus
}
#endif
#endif
