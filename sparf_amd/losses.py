"""The correspondence loss and, below it, the depth-consistency loss, the photometric, mask and
depth-patch loss, the correspondence sampler, the DS-NeRF sparse depth loss
and the depth-consistency front end and ray sampler.

The correspondence loss: SPARF's re-projection of rendered depth at matched pixels through the current relative
pose (corres_loss.py:50-95, :183-219; batched_geometry_utils.py:199-228; base_losses.py:197-224).

The renders and the autograd graph stay PyTorch's (the sampler: the last section).  The BODY -- four re-projection terms and the two compositions of the
relative pose -- is one library call behind ops.ReprojLoss / ops.ReprojPairLoss for dense-able float32 tensors on the GPU, and a plain
torch restatement of the same formulas, in this file, for everything else: CPU, float64, intrinsics / pixels / weights that require a
gradient (the kernels give none to them), and `unfused()`.  `install()` puts the method under a trainer's own name.  Nothing in this
package calls any of it; there is no `opt.hip` key.

The depth-consistency loss (depth_cons_loss.py:219-321 compute_loss_at_sampled_pose; batched_geometry_utils.py:231-266) follows the same
plan: its three renders stay the caller's, the chains between them are `depth_consistency_project` (ops.DconsProject), `visibility_select`
(ops.DconsSelect) and `depth_consistency_loss` (ops.DconsLoss), each with a torch restatement here, and
`install_depth_consistency()` puts the method under the reference's name.  The two masked selections become ordered compactions on the
device; what is read back is the two ray counts the following renders need on the host.

The photometric, mask and depth-patch loss (base_losses.py:243-323, :180-194; metrics.py:33-75) is ONE call, `photo_and_regu_loss`
(ops.PhotoReguLoss), that gathers the ground-truth pixels in the kernel; `mse_on_rays` is the same call without seeds, and
`install_photometric()` puts the method and, if asked, the metric under the reference's names.  It reads nothing back.

The correspondence sampler (base_corres_loss.py:260-269, :323-328, :365-369; corres_loss.py:139-155) is `select_matches`:
an ordered compaction of the valid-correspondence mask (ops.match_compact), one readback of the count, torch.randperm as the reference
calls it, and one gather of the selected rows (ops.match_gather); `install_sampler()` puts the three methods that hold those lines under
the reference's names.

The DS-NeRF sparse depth loss (base_losses.py:326-402) is `sparse_depth_select` -- one ordered compaction of the
valid pixels of every COLMAP map (ops.colmap_compact), one readback of the 2 B counts, torch.randperm as the reference calls it, a
gather of the selected rows (ops.colmap_gather) -- and `sparse_depth_loss` (ops.ColmapLoss: the value and both seeds in one call);
`install_colmap_depth()` puts a method under the reference's name that issues every render before it reads any.

The depth-consistency front end and the ray sampler (depth_cons_loss.py:45-63, :103-106, :168-188;
sampling_strategies.py:132-296) are `sample_pixels` (ops.pick_pixels: one launch behind one copy of the drawn permutation prefix) and
`sample_unseen_pose` (ops.unseen_pose: the nearest other camera, the blend and the inverses in one launch, no readback), each with a
torch restatement; `install_depth_consistency_sampler()` and `install_ray_sampler()` put the methods that hold those lines under the
reference's names.  The random draws stay the reference's.
"""
import collections
import contextlib

import numpy as np
import torch

from . import ops
from .patcher import Patcher

LOSS_TYPES = tuple(ops.REPROJ_LOSS_TYPES)
STAT_KEYS = ("perc_val_pix_rep", "perc_val_depth_rep", "depth_in_corr_loss")
_unfused = 0


@contextlib.contextmanager
def unfused():
    """Inside the block everything below takes its torch restatement, whatever its inputs: for a caller that needs a second
    derivative (the kernels' backward is once-differentiable) and for measuring the kernels against what an unmodified trainer runs
    (tools/corres_loss_bench.py --leg series)."""
    global _unfused
    _unfused += 1
    try:
        yield
    finally:
        _unfused -= 1


def _takes_kernel(values, constants):
    """`values` get a gradient from the kernels, `constants` (K, pixels, weights) do not: float32 (integer pixel grids are cast, as
    the reference's .float() does) on the renderer's device, and no gradient asked of a constant"""
    if _unfused:
        return False
    ok = lambda t: t.device.type == "cuda" and t.layout == torch.strided
    return (all(ok(t) and t.dtype == torch.float32 for t in values if t is not None) and
            all(ok(t) and not (t.requires_grad and torch.is_grad_enabled()) for t in constants if t is not None))


# ---------------------------------------------------------------------------------------------- the torch restatement
def _to_hom(x):
    return torch.cat([x, torch.ones_like(x[..., :1])], dim=-1)


def _from_hom(x):
    return x[..., :-1] / (x[..., -1:] + 1e-6)


def pose_inverse_4x4_torch(mat):
    """camera.py:37-61, the transpose form: [4,4] -> [4,4] with the bottom row [0,0,0,1]"""
    R_inv = mat[:3, :3].transpose(-1, -2)
    out = torch.zeros_like(mat)
    out[3, 3] = 1
    out[:3] = torch.cat([R_inv, -R_inv @ mat[:3, 3:]], dim=-1)
    return out


def _to_4x4(pose):
    if pose.shape[-2] == 4:
        return pose
    return torch.cat([pose, pose.new_tensor([[0.0, 0.0, 0.0, 1.0]])], dim=0)


def project_to_other_img_torch(kpi, di, Ki, Kj, T_itoj):
    """batched_geometry_utils.py:199-228 batch_project_to_other_img with return_depth: -> (pixels in j [n,2], depth in j [n])"""
    if di.dim() == kpi.dim():
        di = di.squeeze(-1)
    x = _to_hom(kpi) @ torch.inverse(Ki).transpose(-1, -2) * di[..., None]
    X = _from_hom(_to_hom(x) @ T_itoj.transpose(-1, -2))
    return _from_hom(X @ Kj.transpose(-1, -2)), X[..., -1]


def diff_loss_torch(loss_type, diff, weights=None, mask=None):
    """base_losses.py:197-224 compute_diff_loss (without its variance branch)"""
    kind = loss_type.lower()
    if kind == "epe":
        loss = torch.norm(diff, 2, -1, keepdim=True)
    elif kind == "l1":
        loss = torch.abs(diff)
    elif kind == "mse":
        loss = diff ** 2
    elif kind == "huber":
        loss = torch.nn.functional.huber_loss(diff, torch.zeros_like(diff), reduction="none", delta=1.0)
    else:
        raise ValueError("Wrong loss type: {}".format(loss_type))
    if weights is not None:
        loss = loss * weights
    if mask is not None:
        loss = loss * mask.to(loss.dtype)
        return loss.sum() / (mask.to(loss.dtype).sum() + 1e-6)
    return loss.sum() / (loss.nelement() + 1e-6)


def reprojection_loss_torch(pixels_i, depth_i, intr_i, pixels_j, depth_j, intr_j, T_itoj, weights, loss_type, pixel_thresh, depth_thresh):
    """corres_loss.py:73-91 -> (loss, stats, valid [n,1])"""
    dtype = depth_i.dtype
    uv, z = project_to_other_img_torch(pixels_i.to(dtype), depth_i.reshape(-1), intr_i, intr_j, T_itoj)
    diff = uv - pixels_j
    err = torch.norm(diff, dim=-1, keepdim=True)
    valid = torch.ones_like(err).bool()
    stats = {}
    if pixel_thresh is not None:
        valid_pixel = err.detach().le(pixel_thresh)
        valid = valid & valid_pixel
        stats["perc_val_pix_rep"] = valid_pixel.sum().to(dtype) / (valid_pixel.nelement() + 1e-6)
    if depth_thresh is not None:
        dj = depth_j.reshape(-1)
        valid_depth = (torch.abs(dj - z) / (dj + 1e-6)).detach().le(depth_thresh)
        valid = valid & valid_depth.unsqueeze(-1)
        stats["perc_val_depth_rep"] = valid_depth.sum().to(dtype) / (valid_depth.nelement() + 1e-6)
    w = weights.reshape(-1, 1) if weights is not None else None
    return diff_loss_torch(loss_type, diff, w, valid), stats, valid


def correspondence_pair_loss_torch(pixels_self, pixels_other, depth_self, depth_other, intr_self, intr_other, pose_w2c_self, pose_w2c_other,
                                   weights, depth_fine_self, depth_fine_other, loss_type, pixel_thresh, depth_thresh):
    """corres_loss.py:183-219 -> (loss, stats)"""
    stats = {"depth_in_corr_loss": depth_self.detach().mean()}
    T_s2o = _to_4x4(pose_w2c_other) @ pose_inverse_4x4_torch(_to_4x4(pose_w2c_self))
    loss = 0
    pairs = [(depth_self, depth_other)] + ([(depth_fine_self, depth_fine_other)] if depth_fine_self is not None else [])
    for d_s, d_o in pairs:
        l, st, _ = reprojection_loss_torch(pixels_self, d_s, intr_self, pixels_other, d_o, intr_other, T_s2o, weights, loss_type, pixel_thresh,
                                           depth_thresh)
        stats.update(st)
        loss = loss + l
        l, st, _ = reprojection_loss_torch(pixels_other, d_o, intr_other, pixels_self, d_s, intr_self, pose_inverse_4x4_torch(T_s2o), weights,
                                           loss_type, pixel_thresh, depth_thresh)
        stats.update(st)
        loss = loss + l
    return loss / (2.0 * len(pairs)), stats


# ---------------------------------------------------------------------------------------------- the public functions
def _stats(pixel_thresh, depth_thresh, pix, dep):
    stats = {}
    if pixel_thresh is not None:
        stats["perc_val_pix_rep"] = pix
    if depth_thresh is not None:
        stats["perc_val_depth_rep"] = dep
    return stats


def reprojection_loss(pixels_i, depth_i, intr_i, pixels_j, depth_j, intr_j, T_itoj, weights=None, *, loss_type="huber", pixel_thresh=None,
                      depth_thresh=None, return_valid_mask=False):
    """One re-projection term i -> j over n matches: pixels [n,2] (integer grids are cast), depths [n] or [n,1], intrinsics [3,3],
    T_itoj [4,4], weights [n,1] or None.  A threshold of None switches that check off.  -> (loss, stats[, valid [n,1]]); stats holds
    perc_val_pix_rep / perc_val_depth_rep for the checks that are on, as 0-dim tensors."""
    if depth_thresh is not None and depth_j is None:
        raise ValueError("reprojection_loss: the depth check needs depth_j")
    if _takes_kernel((depth_i, depth_j if depth_thresh is not None else None, T_itoj), (pixels_i, pixels_j, intr_i, intr_j, weights)):
        loss, pix, dep, valid = ops.ReprojLoss.apply(pixels_i, depth_i, intr_i, pixels_j, depth_j if depth_thresh is not None else None, intr_j,
                                                     T_itoj, weights, loss_type, pixel_thresh, depth_thresh, return_valid_mask)
        stats = _stats(pixel_thresh, depth_thresh, pix, dep)
    else:
        loss, stats, valid = reprojection_loss_torch(pixels_i, depth_i, intr_i, pixels_j, depth_j, intr_j, T_itoj, weights, loss_type,
                                                     pixel_thresh, depth_thresh)
    return (loss, stats, valid) if return_valid_mask else (loss, stats)


def correspondence_pair_loss(pixels_self, pixels_other, depth_self, depth_other, intr_self, intr_other, pose_w2c_self, pose_w2c_other, weights,
                             depth_fine_self=None, depth_fine_other=None, *, loss_type="huber", pixel_thresh=None, depth_thresh=None):
    """The correspondence loss of one view pair (corres_loss.py:183-219): self -> other and other -> self on the rendered depths and,
    if given, on the fine ones, through T_self2other = P_other P_self^-1 of the two w2c poses ([3,4] or [4,4]); their mean.
    -> (loss, stats) with depth_in_corr_loss and the checks' stats as the reference's call order leaves them (the last term's)."""
    if (depth_fine_self is None) != (depth_fine_other is None):
        raise ValueError("correspondence_pair_loss: fine depths for one view only")
    if _takes_kernel((depth_self, depth_other, depth_fine_self, depth_fine_other, pose_w2c_self, pose_w2c_other),
                     (pixels_self, pixels_other, intr_self, intr_other, weights)):
        loss, pix, dep, mean = ops.ReprojPairLoss.apply(pixels_self, pixels_other, depth_self, depth_other, depth_fine_self, depth_fine_other,
                                                        intr_self, intr_other, pose_w2c_self, pose_w2c_other, weights, loss_type, pixel_thresh,
                                                        depth_thresh)
        stats = {"depth_in_corr_loss": mean, **_stats(pixel_thresh, depth_thresh, pix, dep)}
        return loss, stats
    return correspondence_pair_loss_torch(pixels_self, pixels_other, depth_self, depth_other, intr_self, intr_other, pose_w2c_self,
                                          pose_w2c_other, weights, depth_fine_self, depth_fine_other, loss_type, pixel_thresh, depth_thresh)


def compute_render_and_repro_loss_w_repro_thres(self, opt, pixels_in_self_int, depth_rendered_self, intr_self, pixels_in_other,
                                                depth_rendered_other, intr_other, T_self2other, conf_values, stats_dict,
                                                return_valid_mask=False):
    """The method of CorrespondencesPairRenderDepthAndGet3DPtsAndReproject (corres_loss.py:50-95) under its own signature and return
    convention: reads opt.diff_loss_type and the four renderrepro_* keys, fills stats_dict."""
    pixel_thresh = opt.renderrepro_pixel_reprojection_thresh if opt.renderrepro_do_pixel_reprojection_check else None
    depth_thresh = opt.renderrepro_depth_reprojection_thresh if opt.renderrepro_do_depth_reprojection_check else None
    loss, stats, valid = reprojection_loss(pixels_in_self_int, depth_rendered_self, intr_self, pixels_in_other, depth_rendered_other, intr_other,
                                           T_self2other, conf_values, loss_type=opt.diff_loss_type, pixel_thresh=pixel_thresh,
                                           depth_thresh=depth_thresh, return_valid_mask=True)
    stats_dict.update(stats)
    if return_valid_mask:
        return loss, stats_dict, valid
    return loss, stats_dict


METHOD = "compute_render_and_repro_loss_w_repro_thres"
_corres = Patcher("sparf_amd.losses.install", "uninstall")


def install(corres_loss_module):
    """Opt-in: put the method above on `corres_loss_module.CorrespondencesPairRenderDepthAndGet3DPtsAndReproject` until `uninstall()`.
    Nothing in this package calls it."""
    _corres.guard()
    _corres.put(corres_loss_module.CorrespondencesPairRenderDepthAndGet3DPtsAndReproject, METHOD, compute_render_and_repro_loss_w_repro_thres)


def uninstall():
    _corres.restore()


# ================================================================================================ the depth-consistency loss
DCONS_LOSS_TYPES = tuple(ops.DCONS_LOSS_TYPES)


# ---------------------------------------------------------------------------------------------- the torch restatement
def backproject_to_3d_torch(kpi, di, Ki, T_itoj):
    """batched_geometry_utils.py:231-248 batch_backproject_to_3d"""
    x = _to_hom(kpi) @ torch.inverse(Ki).transpose(-1, -2) * di[..., None]
    return _from_hom(_to_hom(x) @ T_itoj.transpose(-1, -2))


def project_torch(points, T_itoj, Kj):
    """batched_geometry_utils.py:251-266 batch_project with return_depth: -> (pixels [n,2], depth [n])"""
    X = _from_hom(_to_hom(points) @ T_itoj.transpose(-1, -2))
    return _from_hom(X @ Kj.transpose(-1, -2)), X[..., -1]


def _index_of(mask):
    return torch.nonzero(mask).reshape(-1).to(torch.int32)


def depth_consistency_project_torch(points_w, pose_w2c_unseen, intr_unseen, H, W, depth_min, pixels_ref=None, depth_ref=None, intr_ref=None,
                                    pose_c2w_ref=None):
    """depth_cons_loss.py:209 (without points_w) and :247-259 -> (pixels [c,2], pseudo_depth [c], index [c])"""
    if points_w is None:
        dtype = depth_ref.dtype
        points_w = backproject_to_3d_torch(pixels_ref.to(dtype), depth_ref.reshape(-1), intr_ref, _to_4x4(pose_c2w_ref))
    uv, z = project_torch(points_w, _to_4x4(pose_w2c_unseen), intr_unseen)
    valid = uv[:, 0].ge(0.) & uv[:, 1].ge(0.) & uv[:, 0].le(W - 1) & uv[:, 1].le(H - 1) & z.ge(depth_min)
    return uv[valid], z[valid], _index_of(valid)


def visibility_select_torch(vis, pixels, pseudo_depth, thresh=0.2):
    """depth_cons_loss.py:277-283 -> (pixels [c,2], pseudo_depth [c], vis [c], index [c])"""
    vis = vis.reshape(-1)
    valid = vis.ge(thresh)
    return pixels[valid], pseudo_depth.reshape(-1)[valid], vis[valid], _index_of(valid)


def depth_consistency_loss_torch(pseudo_depth, vis, depth, opacity, depth_fine=None, opacity_fine=None, loss_type="huber"):
    """depth_cons_loss.py:293-312 -> (loss, avg_vis_weight)"""
    zp, v = pseudo_depth.reshape(-1), vis.detach().reshape(-1)
    w = v * opacity.detach().reshape(-1)
    loss = diff_loss_torch(loss_type, zp - depth.reshape(-1), weights=w)
    if depth_fine is not None:
        w = v * opacity_fine.detach().reshape(-1)
        loss = loss + diff_loss_torch(loss_type, zp - depth_fine.reshape(-1), weights=w)
    return loss, w.sum() / (w.nelement() + 1e-6)


# ---------------------------------------------------------------------------------------------- the public functions
def depth_consistency_project(points_w, pose_w2c_unseen, intr_unseen, H, W, depth_min, *, pixels_ref=None, depth_ref=None, intr_ref=None,
                              pose_c2w_ref=None):
    """Pseudo ground-truth points into an unseen view, and the ones that land in it: world points [n,3], or -- with points_w None --
    pixels_ref [n,2] and depth_ref [n] of a reference view with intr_ref [3,3] and pose_c2w_ref ([3,4] or [4,4]), back-projected first.
    pose_w2c_unseen [3,4] or [4,4], intr_unseen [3,3]; depth_min a float or a 0-dim tensor (depth_range[0][0]).  A point is kept if its
    pixel lies in [0, W-1] x [0, H-1] and its depth is >= depth_min.  -> (pixels [c,2], pseudo_depth [c], index [c] int32) in source
    order; index gathers whatever else the caller filters (pixels_in_ref[index]).  Gradients go to points_w / depth_ref only."""
    back = (pixels_ref, depth_ref, intr_ref, pose_c2w_ref)
    if any(t is None for t in back) if points_w is None else any(t is not None for t in back):      # one form, whole, on either route
        raise ValueError("depth_consistency_project: either world points, or all of pixels_ref, depth_ref, intr_ref and pose_c2w_ref")
    if isinstance(depth_min, torch.Tensor) and depth_min.device.type == "cpu":
        depth_min = float(depth_min)                      # host memory: no synchronisation in reading it
    dmin = depth_min if isinstance(depth_min, torch.Tensor) else None
    if _takes_kernel((points_w, depth_ref), (pose_w2c_unseen, intr_unseen, pixels_ref, intr_ref, pose_c2w_ref, dmin)):
        return ops.DconsProject.apply(points_w, pixels_ref, depth_ref, intr_ref, pose_c2w_ref, pose_w2c_unseen, intr_unseen, H, W, depth_min)
    return depth_consistency_project_torch(points_w, pose_w2c_unseen, intr_unseen, H, W, depth_min, pixels_ref, depth_ref, intr_ref, pose_c2w_ref)


def visibility_select(vis, pixels, pseudo_depth, thresh=0.2):
    """The visibility threshold: the rows with vis >= thresh of pixels [m,2], pseudo_depth [m] and vis [m] (or [m,1]), in order.
    -> (pixels [c,2], pseudo_depth [c], vis [c], index [c] int32).  vis gets no gradient."""
    if _takes_kernel((pixels, pseudo_depth), (vis,)):
        return ops.DconsSelect.apply(vis, pixels, pseudo_depth, thresh)
    return visibility_select_torch(vis, pixels, pseudo_depth, thresh)


def depth_consistency_loss(pseudo_depth, vis, depth, opacity, depth_fine=None, opacity_fine=None, loss_type="huber"):
    """The weighted difference of the pseudo depth and the rendered depth over the m kept points: w = vis opacity (both detached),
    loss = sum l(pseudo_depth - depth) w / (m + 1e-6), plus the same on depth_fine / opacity_fine when given.
    -> (loss, avg_vis_weight = sum w / (m + 1e-6) of the last term)."""
    if (depth_fine is None) != (opacity_fine is None):
        raise ValueError("depth_consistency_loss: depth_fine and opacity_fine come together")
    if loss_type.lower() not in DCONS_LOSS_TYPES + ("epe",):
        raise ValueError("Wrong loss type: {}".format(loss_type))
    if loss_type.lower() != "epe" and _takes_kernel((pseudo_depth, depth, depth_fine), (vis.detach(), opacity.detach(),
                                                                                        opacity_fine.detach() if opacity_fine is not None else None)):
        return ops.DconsLoss.apply(pseudo_depth, vis, depth, opacity, depth_fine, opacity_fine, loss_type)
    return depth_consistency_loss_torch(pseudo_depth, vis, depth, opacity, depth_fine, opacity_fine, loss_type)


def compute_loss_at_sampled_pose(self, data_dict, pose_w2c_at_unseen, intr_at_unseen, pseudo_gt_3dpts_in_w, H, W, pixels_in_ref):
    """The method of DepthConsistencyLoss (depth_cons_loss.py:219-321) under its own signature and return convention: reads
    self.opt.diff_loss_type, gradually_decrease_depth_cons_loss and depth_cons_loss_reduct_at_x_iter, calls self.net's two render
    methods as :267 and :291 do.  (The reference also filters pixels_in_ref and the world points and never reads them again; its
    assert on the visibility, a host synchronisation, is left out.)"""
    iteration = data_dict['iter']
    stats_dict, plotting_dict = {'nbr_px_sampling': pseudo_gt_3dpts_in_w.shape[0]}, {}
    empty = lambda: ({'depth_cons': torch.tensor(0., requires_grad=True).to(self.device)}, {}, {})
    pixels, pseudo_depth, _ = depth_consistency_project(pseudo_gt_3dpts_in_w, pose_w2c_at_unseen, intr_at_unseen, H, W,
                                                        data_dict.depth_range[0][0])
    if pseudo_depth.shape[0] == 0:
        return empty()
    with torch.no_grad():
        ret_max = self.net.render_up_to_maxdepth_at_specific_pose_and_rays(self.opt, data_dict, pose_w2c_at_unseen[:3], intr_at_unseen, H, W,
                                                                           depth_max=pseudo_depth, pixels=pixels, mode='train', iter=iteration)
        vis = ret_max['all_cumulated_fine'] if 'all_cumulated_fine' in ret_max.keys() else ret_max['all_cumulated']
    pixels, pseudo_depth, vis, _ = visibility_select(vis.squeeze(0), pixels, pseudo_depth, 0.2)
    if pseudo_depth.shape[0] == 0:
        return empty()
    ret = self.net.render_image_at_specific_pose_and_rays(self.opt, data_dict, pose_w2c_at_unseen[:3], intr_at_unseen, H, W, pixels=pixels,
                                                          mode='train', iter=iteration)
    fine = 'rgb_fine' in ret.keys()
    loss, avg = depth_consistency_loss(pseudo_depth, vis, ret.depth, ret.opacity, ret.depth_fine if fine else None,
                                       ret.opacity_fine if fine else None, loss_type=self.opt.diff_loss_type)
    stats_dict['avg_vis_weight'] = avg
    if self.opt.gradually_decrease_depth_cons_loss:
        loss = loss / 2 ** (iteration // self.opt.depth_cons_loss_reduct_at_x_iter)
    return {'depth_cons': loss}, stats_dict, plotting_dict


DCONS_METHOD = "compute_loss_at_sampled_pose"
_dcons = Patcher("sparf_amd.losses.install_depth_consistency", "uninstall_depth_consistency")


def install_depth_consistency(depth_cons_loss_module):
    """Opt-in, and independent of install(): put the method above on `depth_cons_loss_module.DepthConsistencyLoss` until
    `uninstall_depth_consistency()`.  Nothing in this package calls it."""
    _dcons.guard()
    _dcons.put(depth_cons_loss_module.DepthConsistencyLoss, DCONS_METHOD, compute_loss_at_sampled_pose)


def uninstall_depth_consistency():
    _dcons.restore()


# ================================================================================================ the photometric, mask and depth-patch loss
# BasePhotoandReguLoss.compute_loss (base_losses.py:243-323 with compute_regularization_losses' depth-patch term,
# :180-194, regularization_losses.py:51-66) and compute_mse_on_rays (metrics.py:33-75), the loss module every trainer runs on every
# iteration.  One library call (ops.PhotoReguLoss) gathers the ground-truth colours and the mask in place and leaves every term, the two
# logged MSEs and the gradient seeds; the torch restatement below serves everything else.  The distortion loss is not part of it: a config
# with loss_weight.distortion set is handed to the original method.
PHOTO_METHOD = "compute_loss"
MSE_NAME = "compute_mse_on_rays"


# ---------------------------------------------------------------------------------------------- the torch restatement
def gather_rays_torch(per_pixel, ray_idx):
    """base_losses.py:285-301 and metrics.py:58-68 on a [B, H*W, C] tensor: -> [B, N, C] (None: the whole images)"""
    if ray_idx is None:
        return per_pixel
    B = per_pixel.shape[0]
    if len(ray_idx.shape) == 2 and ray_idx.shape[0] == B:
        n_rays = ray_idx.shape[-1]
        batch_idx_flattened = torch.arange(start=0, end=B).unsqueeze(-1).repeat(1, n_rays).long().view(-1)
        return per_pixel[batch_idx_flattened, ray_idx.reshape(-1).long()].reshape(B, n_rays, -1)
    return per_pixel[:, ray_idx]


def colour_loss_torch(pred, label, huber):
    """base_losses.py:151-156 MSE_loss / huber_loss"""
    if huber:
        return torch.nn.functional.huber_loss(pred, label, reduction="mean", delta=ops.PHOTO_HUBER_DELTA) * 2.
    loss = (pred.contiguous() - label) ** 2
    return loss.sum() / (loss.nelement() + 1e-6)


def fg_mask_loss_torch(fg, opacity):
    """base_losses.py:315-316 on the gathered mask [B,N,1] (float) and opacity [B,N,1]"""
    return 0.5 * torch.abs(fg - opacity).mean()


def depth_patch_loss_torch(depths, patch_size, charbonnier=0.001):
    """regularization_losses.py:51-66 depth_patch_loss on [B, N(, 1)] depths, times base_losses.py:182's strength"""
    B = depths.shape[0]
    depths = depths.reshape(B, -1, patch_size ** 2)
    resid_sq = (depths[..., None] - depths[..., None, :]) ** 2
    return 0.02 * torch.sqrt(resid_sq + charbonnier ** 2).mean()


def _mse_torch(pred, label):
    """metrics.py:26-31 MSE_loss without a mask"""
    return ((pred.contiguous() - label) ** 2).mean()


def photo_and_regu_loss_torch(image, ray_idx, rgb, rgb_fine=None, *, fg_mask=None, opacity=None, opacity_fine=None, depth=None, depth_fine=None,
                              huber=False, patch_size=None, charbonnier=0.001):
    """base_losses.py:274-319 and :180-194 in the reference's operation order -> (dict of the terms that are on, dict(mse, mse_fine))"""
    B = image.shape[0]
    target = gather_rays_torch(image.reshape(B, 3, -1).permute(0, 2, 1), ray_idx)
    loss = dict(render=colour_loss_torch(rgb.reshape(B, -1, 3), target, huber))
    mse = dict(mse=_mse_torch(rgb.detach().reshape(B, -1, 3), target.detach()), mse_fine=None)
    if rgb_fine is not None:
        loss["render"] = loss["render"] + colour_loss_torch(rgb_fine.reshape(B, -1, 3), target, huber)
        mse["mse_fine"] = _mse_torch(rgb_fine.detach().reshape(B, -1, 3), target.detach())
    if fg_mask is not None:
        fg = gather_rays_torch(fg_mask.float().view(B, -1, 1), ray_idx)
        loss["fg_mask"] = fg_mask_loss_torch(fg, opacity.reshape(B, -1, 1))
        if opacity_fine is not None:
            loss["fg_mask"] = loss["fg_mask"] + fg_mask_loss_torch(fg, opacity_fine.reshape(B, -1, 1))
    if patch_size is not None:
        loss["depth_patch"] = depth_patch_loss_torch(depth.reshape(B, -1), patch_size, charbonnier)
        if depth_fine is not None:
            loss["depth_patch"] = loss["depth_patch"] + depth_patch_loss_torch(depth_fine.reshape(B, -1), patch_size, charbonnier)
    return loss, mse


def _rendered_images(image, idx_img_rendered):
    """metrics.py:52-56 image[idx_img_rendered]; a host-side index that names every image in order selects nothing and copies nothing"""
    B = image.shape[0]
    if not (isinstance(idx_img_rendered, torch.Tensor) and idx_img_rendered.device.type != "cpu"):
        if [int(i) for i in idx_img_rendered] == list(range(B)):
            return image
    return image[idx_img_rendered]


def mse_on_rays_torch(data_dict, output_dict):
    """metrics.py:33-75 compute_mse_on_rays -> (mse_coarse, mse_fine or None)"""
    batch_size = len(data_dict.idx)
    image = data_dict.image.reshape(batch_size, 3, -1).permute(0, 2, 1)
    nbr = len(output_dict.idx_img_rendered)
    image = gather_rays_torch(image[output_dict.idx_img_rendered].reshape(nbr, -1, 3), output_dict.ray_idx if 'ray_idx' in output_dict.keys() else None)
    mse_fine = None
    if 'rgb_fine' in output_dict.keys():
        mse_fine = _mse_torch(output_dict.rgb_fine.reshape(nbr, -1, 3), image)
    return _mse_torch(output_dict.rgb.reshape(nbr, -1, 3), image), mse_fine


# ---------------------------------------------------------------------------------------------- the public functions
def _photo_takes_kernel(image, ray_idx, fg_mask, values, patch_size):
    return (_takes_kernel(values, (image, ray_idx, fg_mask)) and image.dtype == torch.float32 and
            (ray_idx is None or ray_idx.dtype == torch.int64) and (fg_mask is None or fg_mask.dtype == torch.bool) and
            (patch_size is None or 0 < patch_size <= ops.PHOTO_MAX_PATCH))


def photo_and_regu_loss(image, ray_idx, rgb, rgb_fine=None, *, fg_mask=None, opacity=None, opacity_fine=None, depth=None, depth_fine=None,
                        huber=False, patch_size=None, charbonnier=0.001):
    """The photometric loss of rendered rays against image [B,3,H,W] with, if asked for, the foreground-mask loss and the depth-patch
    regulariser: rgb / rgb_fine [B,N,3]; ray_idx int64 [N] (the same rays of every image), [B,N] (per image) or None (full images,
    N = H W); fg_mask (torch.bool, one element per pixel) switches the mask term on and needs opacity [B,N,1]; patch_size = P switches
    the depth-patch term on and needs depth [B,N,1] with N a multiple of P^2; a fine tensor adds the same term on the fine head.
    huber: the module's Huber loss (delta 0.5, x 2) in place of the MSE.
    -> (dict(render, fg_mask, depth_patch) with the terms that are on, dict(mse, mse_fine: None without rgb_fine)): 0-dim tensors; the
    mse values carry no gradient.  Gradients go to the six rendered tensors, none to the image."""
    if fg_mask is not None and opacity is None:
        raise ValueError("photo_and_regu_loss: the mask term needs opacity")
    if patch_size is not None and depth is None:
        raise ValueError("photo_and_regu_loss: the depth-patch term needs depth")
    on = lambda t, used: t if used else None
    values = (rgb, rgb_fine, on(opacity, fg_mask is not None), on(opacity_fine, fg_mask is not None), on(depth, patch_size is not None),
              on(depth_fine, patch_size is not None))
    if _photo_takes_kernel(image, ray_idx, fg_mask, values, patch_size):
        render, mask, dpatch, mse, mse_fine = ops.PhotoReguLoss.apply(image, fg_mask, ray_idx, *values, "huber" if huber else "mse",
                                                                      ops.PHOTO_HUBER_DELTA, patch_size or 0, charbonnier)
        loss = dict(render=render)
        if fg_mask is not None:
            loss["fg_mask"] = mask
        if patch_size is not None:
            loss["depth_patch"] = dpatch
        return loss, dict(mse=mse, mse_fine=mse_fine if rgb_fine is not None else None)
    return photo_and_regu_loss_torch(image, ray_idx, rgb, rgb_fine, fg_mask=fg_mask, opacity=opacity, opacity_fine=opacity_fine, depth=depth,
                                     depth_fine=depth_fine, huber=huber, patch_size=patch_size, charbonnier=charbonnier)


def mse_on_rays(data_dict, output_dict):
    """compute_mse_on_rays (metrics.py:33-75) under its own signature and return convention, indexing by idx_img_rendered included:
    the same kernel with no seeds and no other term.  -> (mse_coarse, mse_fine or None)"""
    ray_idx = output_dict.ray_idx if 'ray_idx' in output_dict.keys() else None
    rgb = output_dict.rgb.detach()
    rgb_fine = output_dict.rgb_fine.detach() if 'rgb_fine' in output_dict.keys() else None
    image = data_dict.image
    if not _photo_takes_kernel(image, ray_idx, None, (rgb, rgb_fine), None):
        return mse_on_rays_torch(data_dict, output_dict)
    image = _rendered_images(image.reshape(len(data_dict.idx), 3, -1), output_dict.idx_img_rendered)
    nbr = len(output_dict.idx_img_rendered)
    _, _, _, mse, mse_fine = ops.PhotoReguLoss.apply(image, None, ray_idx, rgb.reshape(nbr, -1, 3), rgb_fine.reshape(nbr, -1, 3) if rgb_fine is not None
                                                     else None, None, None, None, None, "mse", ops.PHOTO_HUBER_DELTA, 0, 0.001)
    return mse, (mse_fine if rgb_fine is not None else None)


_photo = Patcher("sparf_amd.losses.install_photometric", "uninstall_photometric")     # keeps the class's own compute_loss: the distortion hand-over calls it


def compute_loss(self, opt, data_dict, output_dict, iteration, mode=None, plot=False, **kwargs):
    """The method of BasePhotoandReguLoss (base_losses.py:243-323) under its own signature and return convention: reads
    self.opt.start_iter.photometric, huber_loss_for_photometric and depth_regu_patch_size, opt.loss_weight.fg_mask / depth_patch and
    opt.nerf.rand_rays.  A config with opt.loss_weight.distortion set goes to the original method, untouched: the distortion loss
    needs gradients to per-sample weights that the call does not give."""
    from .edict import EasyDict as edict
    if opt.loss_weight.distortion is not None:
        original = _photo.original(PHOTO_METHOD)
        if original is None:
            raise RuntimeError("sparf_amd.losses.compute_loss: loss_weight.distortion is set and there is no original method to hand it to "
                               "(install_photometric() saves it)")
        return original(self, opt, data_dict, output_dict, iteration, mode=mode, plot=plot, **kwargs)
    loss_dict = edict(render=torch.tensor(0., requires_grad=True).to(self.device))
    if iteration < self.opt.start_iter.photometric:
        return loss_dict, {}, {}
    batch_size = len(data_dict.idx)
    assert len(output_dict.idx_img_rendered) == batch_size
    with_mask, with_patch = opt.loss_weight.fg_mask is not None, opt.loss_weight.depth_patch is not None
    has = lambda key: output_dict[key] if key in output_dict.keys() else None
    sampled = (hasattr(opt, 'nerf') and opt.nerf.rand_rays) and mode in ["train", "test-optim"]
    shape = lambda t, c: t.reshape(batch_size, -1, c) if t is not None else None
    terms, _ = photo_and_regu_loss(data_dict.image.reshape(batch_size, 3, -1), output_dict.ray_idx if sampled else None,
                                   shape(output_dict.rgb, 3), shape(has('rgb_fine'), 3),
                                   fg_mask=data_dict.fg_mask if with_mask else None, opacity=shape(output_dict.opacity, 1) if with_mask else None,
                                   opacity_fine=shape(has('opacity_fine'), 1) if with_mask else None,
                                   depth=shape(output_dict['depth'], 1) if with_patch else None,
                                   depth_fine=shape(has('depth_fine'), 1) if with_patch else None,
                                   huber=bool(self.opt.huber_loss_for_photometric),
                                   patch_size=self.opt.depth_regu_patch_size if with_patch else None)
    loss_dict.update(terms)
    return loss_dict, {}, {}


def install_photometric(base_losses_module, trainer_module=None):
    """Opt-in, and independent of install() and install_depth_consistency(): put compute_loss above on
    `base_losses_module.BasePhotoandReguLoss` and, with `trainer_module` (a module that imported the name, as nerf_trainer does), mse_on_rays
    under its `compute_mse_on_rays`, until `uninstall_photometric()`.  Nothing in this package calls it."""
    _photo.guard()
    cls = base_losses_module.BasePhotoandReguLoss
    _photo.save(PHOTO_METHOD, getattr(cls, PHOTO_METHOD, None))
    _photo.put(cls, PHOTO_METHOD, compute_loss)
    if trainer_module is not None:
        _photo.put(trainer_module, MSE_NAME, mse_on_rays)


def uninstall_photometric():
    _photo.restore()


# ================================================================================================ the correspondence sampler
# what CorrespondenceBasedLoss runs between "pair chosen" and the two renders of compute_loss_on_image_pair
# (base_corres_loss.py:260-269, :323-328, :365-369; corres_loss.py:139-155) -- the centre mask, the rounded index map of the whole image,
# mask.sum(), five boolean selections, randperm and five gathers -- as `select_matches`: one ordered compaction (ops.match_compact), ONE
# readback of the count (the renders need it on the host), torch.randperm as the reference calls it, and one gather (ops.match_gather)
# that rounds the selected rows only.  Nothing here carries a gradient.  `install_sampler()` puts the three methods that hold those lines
# under the reference's names.
SAMPLER_METHODS = ("compute_loss_pairwise", "compute_loss_at_given_img_indexes", "compute_loss_on_image_pair")
_unfused_sampler = 0


@contextlib.contextmanager
def unfused_sampler():
    """Inside the block select_matches alone takes its torch restatement; every other function above keeps its route (for comparing the
    two samplers under the same renders and the same loss kernel)."""
    global _unfused_sampler
    _unfused_sampler += 1
    try:
        yield
    finally:
        _unfused_sampler -= 1


def _map_forms(mask, corres_map, conf_map):
    """-> (mask [H,W], correspondences [H,W,2], confidences [H,W,1]) as the reference indexes them, from any accepted form"""
    m = mask.detach()
    m = m.squeeze(-1) if m.dim() == 3 else m
    H, W = m.shape
    c = corres_map.detach()
    c = c if tuple(c.shape) == (H, W, 2) else c.permute(1, 2, 0)
    f = conf_map.detach()
    f = f if tuple(f.shape) == (H, W, 1) else f.reshape(H, W, 1)
    return m, c, f


def _empty_matches(device):
    e = lambda *shape, dtype: torch.empty(*shape, device=device, dtype=dtype)
    return (e(0, 2, dtype=torch.float32), e(0, dtype=torch.int64), e(0, 2, dtype=torch.float32), e(0, dtype=torch.int64),
            e(0, 1, dtype=torch.float32))


_grids = {}


def _pixel_grid(H, W, device):
    """base_corres_loss.py:45-50 self.grid [H,W,2] and self.grid_flat [H,W]: built once per image size and device, as the reference's
    constructor does"""
    key = (H, W, str(device))
    if key not in _grids:
        xx = torch.arange(0, W).view(1, -1).repeat(H, 1)
        yy = torch.arange(0, H).view(-1, 1).repeat(1, W)
        grid = torch.stack((xx, yy), dim=-1).to(device).float()
        _grids[key] = (grid, (grid[:, :, 1] * W + grid[:, :, 0]).to(device).long())
    return _grids[key]


def select_matches_torch(mask, corres_map, conf_map, max_matches, *, window=None, perm=None, min_matches=0):
    """base_corres_loss.py:267-269, :323-328, :365-369 and corres_loss.py:139-155 in the reference's operation order; arguments and
    results as select_matches"""
    m, corres, conf = _map_forms(mask, corres_map, conf_map)
    m = m if m.dtype == torch.bool else m.bool()
    H, W = m.shape
    dev = m.device
    if window is not None:
        mask_center = torch.zeros_like(m)
        mask_center[window[0]:window[1], window[2]:window[3]] = 1
        m = m & mask_center
    grid, grid_flat = _pixel_grid(H, W, dev)
    rounded = torch.round(corres).long()
    rounded_flat = rounded[:, :, 1] * W + rounded[:, :, 0]
    total = m.sum()
    # (the reference divides by the Python float; on the device torch then multiplies by the rounded reciprocal, which can differ in the
    # last bit from the division the CPU does: dividing by a float32 tensor is the CPU's value on either device)
    perc = total.to(torch.float32) / torch.full((), m.nelement() + 1e-6, dtype=torch.float32, device=dev)
    count = int(total)
    if count == 0 or count < min_matches:
        return (*_empty_matches(dev), count, perc)
    pixels_self, ray_self = grid[m], grid_flat[m]
    pixels_other, ray_other, conf_values = corres[m], rounded_flat[m], conf[m]
    if count > max_matches:
        random_values = (torch.randperm(count, device=dev) if perm is None else perm)[:max_matches]
        ray_self, pixels_self = ray_self[random_values], pixels_self[random_values]
        pixels_other, ray_other, conf_values = pixels_other[random_values], ray_other[random_values], conf_values[random_values]
    return pixels_self, ray_self, pixels_other, ray_other, conf_values, count, perc


def select_matches(mask, corres_map, conf_map, max_matches, *, window=None, perm=None, min_matches=0):
    """The matches of one view pair that a correspondence iteration renders: the pixels of mask ([H,W] or [H,W,1]) inside window -- (y0,
    y1, x0, x1) as the slices mask[y0:y1, x0:x1] of base_corres_loss.py:268 read them, None for the whole image -- in row-major order;
    if there are more than max_matches, the rows perm[:max_matches] of them, with perm = torch.randperm(count, device=mask.device) when
    none is given (the reference's own call: the same seed draws the same matches and leaves the generator in the same state).
    corres_map [H,W,2] (the reference's permuted view; read in place) or channel-first [2,H,W]; conf_map [H,W,1], [1,H,W] or [H,W].
    -> (pixels_self [k,2] float32, ray_self [k] int64, pixels_other [k,2] float32, ray_other [k] int64: the flat index of the rounded
    correspondence, conf [k,1] float32, count: a Python int, the ONE readback, perc_valid = count / (H W + 1e-6) as a 0-dim tensor).
    With count == 0 or count < min_matches the five tensors are empty and nothing is drawn or gathered."""
    if (_unfused_sampler or mask.dtype != torch.bool or corres_map.dtype != torch.float32 or conf_map.dtype != torch.float32 or
            not _takes_kernel((corres_map, conf_map), (mask,))):
        return select_matches_torch(mask, corres_map, conf_map, max_matches, window=window, perm=perm, min_matches=min_matches)
    H, W = mask.shape[:2]
    index, count_dev, perc = ops.match_compact(mask, window)
    count = int(count_dev.item()) if H * W else 0         # the one readback
    perc = perc[0]
    if count == 0 or count < min_matches:
        return (*_empty_matches(mask.device), count, perc)
    sel = None
    if count > max_matches:
        sel = (torch.randperm(count, device=mask.device) if perm is None else perm)[:max_matches]
    rows = ops.match_gather(index, count_dev, sel, min(count, max_matches), H, W, corres_map, conf_map)
    return (*rows, count, perc)


_sampler = Patcher("sparf_amd.losses.install_sampler", "uninstall_sampler")     # keeps the classes' own methods: the debug configurations are handed to them


def _opt(opt, key, default=None):
    return getattr(opt, key, default) if not isinstance(opt, dict) else opt.get(key, default)


def _handed_over(self, name):
    original = _sampler.original(name)
    if original is None:
        raise RuntimeError(f"sparf_amd.losses.{name}: a debug configuration (use_gt_correspondences / skip_verif=False) and there is no "
                           "original method to hand it to (install_sampler() saves it)")
    return original


def _window_mask_torch(mask, window):
    if window is None:
        return mask
    mask_center = torch.zeros_like(mask)
    mask_center[window[0]:window[1], window[2]:window[3]] = 1
    return mask & mask_center


def compute_loss_pairwise(self, opt, data_dict, output_dict, iteration, mode=None, plot=False):
    """The method of CorrespondenceBasedLoss (base_corres_loss.py:217-273) under its own signature and return convention: the pre-crop
    phase hands the window of :268 on instead of building mask_center."""
    if _opt(self.opt, 'use_gt_correspondences', False):
        return _handed_over(self, SAMPLER_METHODS[0])(self, opt, data_dict, output_dict, iteration, mode, plot)
    zero = lambda: torch.tensor(0., requires_grad=True).to(self.device)
    stats_dict, plotting_dict, loss_dict = {}, {}, {'corres': zero(), 'render_matches': zero()}
    if mode != 'train' or iteration < self.opt.start_iter.corres or len(self.filtered_flow_pairs) == 0:
        return loss_dict, stats_dict, plotting_dict
    id_self, id_matching_view, corres_map, conf_map, variance, mask = self.sample_valid_image_pair()
    window = None
    if iteration < self.opt.precrop_iters:
        H, W = data_dict.image.shape[-2:]
        dH, dW = int(H // 2 * self.opt.precrop_frac), int(W // 2 * self.opt.precrop_frac)
        window = (H // 2 - dH, H // 2 + dH - 1, W // 2 - dW, W // 2 + dW - 1)
    return self.compute_loss_at_given_img_indexes(opt, data_dict, id_self, id_matching_view, corres_map, conf_map, variance, mask, loss_dict,
                                                  stats_dict, plotting_dict, plot, **({} if window is None else dict(window=window)))


def compute_loss_at_given_img_indexes(self, opt, data_dict, id_self, id_matching_view, corres_map_self_to_other_, conf_map_self_to_other_,
                                      variance_self_to_other_, mask_correct_corr, loss_dict, stats_dict, plotting_dict, plot=False,
                                      skip_verif=True, window=None):
    """The method of CorrespondenceBasedLoss (base_corres_loss.py:275-374) under its own signature and return convention, with `window`
    (see select_matches) in addition.  The rounded index map of the whole image and the mask.sum() readback are gone: the
    min_nbr_matches test and the perc_valid_corr_mask stat sit behind the one readback of compute_loss_on_image_pair."""
    if not skip_verif or _opt(self.opt, 'use_gt_correspondences', False):
        return _handed_over(self, SAMPLER_METHODS[1])(self, opt, data_dict, id_self, id_matching_view, corres_map_self_to_other_,
                                                      conf_map_self_to_other_, variance_self_to_other_,
                                                      _window_mask_torch(mask_correct_corr, window), loss_dict, stats_dict, plotting_dict, plot,
                                                      skip_verif)
    images = data_dict.image.permute(0, 2, 3, 1)
    poses_w2c, intrs = data_dict.poses_w2c, data_dict.intr
    pose_w2c_self, pose_w2c_other = _to_4x4(poses_w2c[id_self]), _to_4x4(poses_w2c[id_matching_view])
    return self.compute_loss_on_image_pair(data_dict, images, poses_w2c, intrs, id_self, id_matching_view, corres_map_self_to_other_.detach(), None,
                                           conf_map_self_to_other_.detach(), mask_correct_corr.detach().squeeze(-1), pose_w2c_self,
                                           pose_w2c_other, intrs[id_self], intrs[id_matching_view], loss_dict, stats_dict, plotting_dict,
                                           **({} if window is None else dict(window=window)))


def compute_loss_on_image_pair(self, data_dict, images, poses_w2c, intrs, id_self, id_matching_view, corres_map_self_to_other,
                               corres_map_self_to_other_rounded_flat, conf_map_self_to_other, mask_correct_corr, pose_w2c_self, pose_w2c_other,
                               intr_self, intr_other, loss_dict, stats_dict, plotting_dict, window=None):
    """The method of CorrespondencesPairRenderDepthAndGet3DPtsAndReproject (corres_loss.py:97-220) under its own signature and return
    convention, with `window` in addition: select_matches, the two renders, correspondence_pair_loss.  The rounded index map it is
    handed is ignored (None is fine) and recomputed for the selected rows; the min_nbr_matches test of base_corres_loss.py:365-369 is
    made here, on the count that is read back anyway, and below it the dictionaries come back untouched."""
    if _opt(self.opt, 'use_gt_correspondences', False):
        return _handed_over(self, SAMPLER_METHODS[2])(self, data_dict, images, poses_w2c, intrs, id_self, id_matching_view, corres_map_self_to_other,
                                                      corres_map_self_to_other_rounded_flat, conf_map_self_to_other,
                                                      _window_mask_torch(mask_correct_corr, window), pose_w2c_self, pose_w2c_other, intr_self,
                                                      intr_other, loss_dict, stats_dict, plotting_dict)
    iteration = data_dict['iter']
    B, H, W = images.shape[:3]
    min_matches = _opt(self.opt, 'min_nbr_matches', 0)
    pixels_self, ray_self, pixels_other, ray_other, conf_values, count, perc = select_matches(
        mask_correct_corr, corres_map_self_to_other, conf_map_self_to_other, self.opt.nerf.rand_rays // 2, window=window, min_matches=min_matches)
    if count < min_matches:
        return loss_dict, stats_dict, plotting_dict
    stats_dict['perc_valid_corr_mask'] = perc
    render = lambda pose, intr, pixels: self.net.render_image_at_specific_pose_and_rays(self.opt, data_dict, pose[:3], intr, H, W, pixels=pixels,
                                                                                       mode='train', iter=iteration)
    ret_self = render(pose_w2c_self, intr_self, pixels_self)
    ret_other = render(pose_w2c_other, intr_other, pixels_other)
    if _opt(self.opt, 'compute_photo_on_matches', False):
        image_self = images[id_self].view(-1, 3)[ray_self]
        image_other = images[id_matching_view].view(-1, 3)[ray_other]
        loss_photo_self = self.MSE_loss(ret_self.rgb.view(-1, 3), image_self)
        loss_photo_other = self.MSE_loss(ret_other.rgb.view(-1, 3), image_other)
        if 'rgb_fine' in ret_self.keys():
            loss_photo_self += self.MSE_loss(ret_self.rgb_fine.view(-1, 3), image_self)
            loss_photo_other += self.MSE_loss(ret_other.rgb_fine.view(-1, 3), image_other)
        loss_dict['render_matches'] += (loss_photo_other + loss_photo_self) / 2.
    fine = 'depth_fine' in ret_other.keys()
    flat = lambda d: d.squeeze(0).squeeze(-1)
    pixel_thresh = self.opt.renderrepro_pixel_reprojection_thresh if self.opt.renderrepro_do_pixel_reprojection_check else None
    depth_thresh = self.opt.renderrepro_depth_reprojection_thresh if self.opt.renderrepro_do_depth_reprojection_check else None
    loss, stats = correspondence_pair_loss(pixels_self, pixels_other, flat(ret_self.depth), flat(ret_other.depth), intr_self, intr_other,
                                           pose_w2c_self, pose_w2c_other, conf_values, flat(ret_self.depth_fine) if fine else None,
                                           flat(ret_other.depth_fine) if fine else None, loss_type=self.opt.diff_loss_type,
                                           pixel_thresh=pixel_thresh, depth_thresh=depth_thresh)
    stats_dict.update(stats)
    loss_dict['corres'] = loss
    return loss_dict, stats_dict, plotting_dict


def install_sampler(corres_loss_module, base_corres_loss_module):
    """Opt-in, and independent of install(), install_depth_consistency() and install_photometric(): put compute_loss_pairwise and
    compute_loss_at_given_img_indexes above on `base_corres_loss_module.CorrespondenceBasedLoss` and compute_loss_on_image_pair on
    `corres_loss_module.CorrespondencesPairRenderDepthAndGet3DPtsAndReproject`, until `uninstall_sampler()`.  A module configured with
    use_gt_correspondences, or a call with skip_verif=False, goes to the original methods.  Nothing in this package calls it."""
    _sampler.guard()
    base = base_corres_loss_module.CorrespondenceBasedLoss
    pair = corres_loss_module.CorrespondencesPairRenderDepthAndGet3DPtsAndReproject
    new = dict(zip(SAMPLER_METHODS, (compute_loss_pairwise, compute_loss_at_given_img_indexes, compute_loss_on_image_pair)))
    for cls, name in ((base, SAMPLER_METHODS[0]), (base, SAMPLER_METHODS[1]), (pair, SAMPLER_METHODS[2])):
        _sampler.save(name, getattr(cls, name, None))
        _sampler.put(cls, name, new[name])


def uninstall_sampler():
    _sampler.restore()


# ================================================================================================ the DS-NeRF sparse depth loss
# SparseCOLMAPDepthLoss.compute_loss (base_losses.py:326-402), the loss of the DS-NeRF baseline trainer and of the
# joint trainer under load_colmap_depth.  The reference runs, per image, a torch.where with a host readback, a randperm, six index and
# gather operations, a render of its own whose depth it reads at once, and two weighted means -- B + 1 readbacks and B small renders.
# Here: `sparse_depth_select` (ops.colmap_compact over all images, ONE readback of the 2 B counts, torch.randperm as the reference calls
# it, ops.colmap_gather) and `sparse_depth_loss` (ops.ColmapLoss, one call for the value and both seeds); `install_colmap_depth()` puts
# a method under the reference's name that issues every render before it reads any, so that deferred renders run as one batch.
COLMAP_METHOD = "compute_loss"
SparseCounts = collections.namedtuple("SparseCounts", "valid positive rows quota device")
SparseCounts.__doc__ = """what sparse_depth_select read back: per image the valid pixels (depth > 1e-6), the positive pixels (depth > 0) and the
rows selected, min(valid, quota), as Python ints; `device`: the int32 [2 B] tensor the ints were read from (None on the torch route)"""


def _colmap_takes_kernel(*maps):
    return _takes_kernel((), maps) and all(m.dtype == torch.float32 for m in maps)


def _zero_loss(device):
    return torch.tensor(0., requires_grad=True).to(device)       # base_losses.py:356


# ---------------------------------------------------------------------------------------------- the torch restatement
def sparse_depth_select_torch(colmap_depth, colmap_conf, rand_rays, perms=None):
    """base_losses.py:363-386 without the renders, in the reference's operation order; arguments and results as sparse_depth_select"""
    H, W = colmap_depth.shape[-2:]
    depth, conf = colmap_depth.detach().reshape(-1, H, W), colmap_conf.detach().reshape(-1, H, W)
    B, dev = depth.shape[0], depth.device
    quota = rand_rays // B
    perc = len(torch.where(depth > 0)[0]) / depth.nelement()
    positive = [int((depth[b] > 0).sum()) for b in range(B)]
    rays, targets, weights, valid = [], [], [], []
    for b in range(B):
        h, w = torch.where(depth[b] > 1e-6)
        valid.append(len(h))
        if len(h) > quota:
            random = (perms[b] if perms is not None and perms[b] is not None else torch.randperm(len(h), device=dev))[:quota]
            h, w = h[random], w[random]
        rays.append(h * W + w)
        targets.append(depth[b][h, w].reshape(-1))
        weights.append(conf[b][h, w].reshape(-1))
    counts = SparseCounts(valid, positive, [min(v, quota) for v in valid], quota, None)
    return rays, torch.cat(targets), torch.cat(weights), counts, perc


def _rows_of(counts_or_rows):
    return list(counts_or_rows.rows) if isinstance(counts_or_rows, SparseCounts) else [int(k) for k in counts_or_rows]


def sparse_depth_loss_torch(target, weight, counts_or_rows, depths, depths_fine=None, batch_size=None):
    """base_losses.py:391-400 on the packed rows, with out-of-place adds (the reference's `loss += ...` on a leaf cannot run under
    autograd on CPU tensors); arguments and result as sparse_depth_loss"""
    rows = _rows_of(counts_or_rows)
    batch_size = len(rows) if batch_size is None else batch_size
    kept = [k for k in rows if k > 0]
    if len(depths) != len(kept) or (depths_fine is not None and len(depths_fine) != len(kept)):
        raise ValueError(f"sparse_depth_loss: {len(depths)} rendered depths for {len(kept)} images with rows")
    if not kept:
        return _zero_loss(target.device)
    loss, off = 0, 0
    for i, k in enumerate(kept):
        t, w = target[off:off + k], weight[off:off + k]
        loss = loss + torch.mean(((t - depths[i].reshape(-1)) ** 2) * w)
        if depths_fine is not None:
            loss = loss + torch.mean(((t - depths_fine[i].reshape(-1)) ** 2) * w)
        off += k
    return 0.1 * loss / batch_size


# ---------------------------------------------------------------------------------------------- the public functions
def _split(t, rows):
    return list(torch.split(t, rows))


def sparse_depth_select(colmap_depth, colmap_conf, rand_rays, perms=None):
    """The rays a DS-NeRF iteration renders: per image of colmap_depth [B,1,H,W] the pixels with depth > 1e-6 in row-major order; where an
    image has MORE than quota = rand_rays // B of them, the rows perm[:quota] of them, with perm = torch.randperm(count, device=...) drawn
    per image in image order when `perms` (a list per image, entries None for no permutation) gives none: the reference's own calls, so
    the same seed draws the same rays and leaves the generator in the same state.  The maps are read in place.
    -> (ray_idx: a list of B int64 tensors, flat indices h W + w, empty for an image without valid pixels; target [K] and weight [K]
    float32, the two maps at those pixels packed in image order; counts: a SparseCounts, the ONE readback; perc_col_depth: the share of
    pixels with depth > 0, a Python float, the reference's division)."""
    if not _colmap_takes_kernel(colmap_depth, colmap_conf):
        return sparse_depth_select_torch(colmap_depth, colmap_conf, rand_rays, perms)
    B, (H, W) = colmap_depth.shape[0], colmap_depth.shape[-2:]
    quota = rand_rays // B
    index, count = ops.colmap_compact(colmap_depth)
    counts, perc = _read_counts(count, B, H * W, quota)
    K = sum(counts.rows)
    sel = None
    for b in range(B):
        if counts.valid[b] > quota:
            perm = perms[b] if perms is not None and perms[b] is not None else torch.randperm(counts.valid[b], device=colmap_depth.device)
            if sel is None:
                sel = torch.zeros(B, quota, device=colmap_depth.device, dtype=torch.int64)
            sel[b].copy_(perm[:quota])
    ray_idx, target, weight = ops.colmap_gather(index, count, sel, quota, K, H, W, colmap_depth, colmap_conf)
    return _split(ray_idx, counts.rows), target, weight, counts, perc


def _read_counts(count, B, n, quota):
    """the one readback: the 2 B ints of ops.colmap_compact -> (SparseCounts, perc_col_depth as base_losses.py:367 divides it)"""
    both = count.tolist()
    valid, positive = both[:B], both[B:]
    return SparseCounts(valid, positive, [min(v, quota) for v in valid], quota, count), sum(positive) / (B * n)


def sparse_depth_loss(target, weight, counts_or_rows, depths, depths_fine=None, batch_size=None):
    """The DS-NeRF depth loss of the selected rows: target / weight [K] as sparse_depth_select packs them; counts_or_rows its SparseCounts,
    or the rows per image as ints (zeros included); depths / depths_fine: the rendered depths of the images WITH rows, in image order,
    k_b elements each in any shape.  batch_size (default: the number of images) divides the sum, skipped images counted, as
    base_losses.py:400 does.  L = (0.1 / B) sum_b (1 / k_b) sum_j w ((d - p)^2 [+ (d - pf)^2]); gradients go to the rendered depths.
    -> a 0-dim tensor; with no rows at all the zero loss with requires_grad, and no launch."""
    rows = _rows_of(counts_or_rows)
    batch_size = len(rows) if batch_size is None else batch_size
    depths = list(depths)
    depths_fine = list(depths_fine) if depths_fine is not None else None
    values = depths + (depths_fine or [])
    if not values or not _takes_kernel(values, (target, weight)) or target.dtype != torch.float32 or weight.dtype != torch.float32:
        return sparse_depth_loss_torch(target, weight, rows, depths, depths_fine, batch_size)
    kept = [k for k in rows if k > 0]
    if len(depths) != len(kept) or (depths_fine is not None and len(depths_fine) != len(kept)):
        raise ValueError(f"sparse_depth_loss: {len(depths)} rendered depths for {len(kept)} images with rows")
    if isinstance(counts_or_rows, SparseCounts) and counts_or_rows.device is not None:
        count, quota = counts_or_rows.device, counts_or_rows.quota
    else:
        count, quota = torch.tensor(rows, dtype=torch.int32).to(target.device), ops.COLMAP_ALL_ROWS
    return ops.ColmapLoss.apply(target, weight, count, quota, batch_size, len(depths), *values)


def _render_rays(self, data_dict, pose, intr, H, W, iteration, b, ray_idx):
    return self.net.render_image_at_specific_pose_and_rays(self.opt, data_dict, pose[b], intr[b], H, W, ray_idx=ray_idx, mode='train',
                                                           iter=iteration)


def _colmap_loop_torch(self, opt, data_dict, pose, intr, H, W, iteration):
    """base_losses.py:363-400, the reference's loop in its own order -- per image the selection, the randperm and the render -- except
    that no result is read before every call is made, and that the adds are out of place.  -> (loss, perc_col_depth)"""
    depth, conf = data_dict.colmap_depth.view(-1, H, W), data_dict.colmap_conf.view(-1, H, W)
    B = pose.shape[0]
    quota = opt.nerf.rand_rays // B
    perc = len(torch.where(depth > 0)[0]) / depth.nelement()
    rets, targets, weights, rows = [], [], [], []
    for b in range(B):
        h, w = torch.where(depth[b] > 1e-6)
        if len(h) == 0:
            rows.append(0)
            continue
        if len(h) > quota:
            random = torch.randperm(len(h), device=self.device)[:quota]
            h, w = h[random], w[random]
        rows.append(len(h))
        targets.append(depth[b][h, w].reshape(-1))
        weights.append(conf[b][h, w].reshape(-1))
        rets.append(_render_rays(self, data_dict, pose, intr, H, W, iteration, b, h * W + w))
    if not rets:
        return _zero_loss(self.device), perc
    fine = 'depth_fine' in rets[0].keys()
    return sparse_depth_loss_torch(torch.cat(targets), torch.cat(weights), rows, [r.depth for r in rets],
                                   [r.depth_fine for r in rets] if fine else None, B), perc


def compute_colmap_depth_loss(self, opt, data_dict, output_dict, iteration, mode=None, plot=False, **kwargs):
    """The method of SparseCOLMAPDepthLoss (base_losses.py:335-402) under its own signature and return convention: reads
    opt.nerf.rand_rays, data_dict.colmap_depth / colmap_conf [B,1,H,W], image and intr, and calls self.net.get_w2c_pose and, per image with
    a valid pixel, self.net.render_image_at_specific_pose_and_rays as :387 does.  One compaction of all images, ONE readback of the 2 B
    counts; then image by image its randperm (if the reference draws one) and its render call, in the reference's order, so that the
    generators see the reference's sequence; no result is read before every call is made, so deferred renders (opt.hip.lazy_batch) run
    as one batch.  A gather launch covers the images from one that draws up to the next that draws: the rows of an image are on the
    device before its render is called, and no permutation is drawn ahead of a render the reference makes first."""
    from .edict import EasyDict as edict
    if mode != 'train':
        return {}, {}, {}
    H, W = data_dict.image.shape[-2:]
    pose = self.net.get_w2c_pose(opt, data_dict, mode=mode)
    intr = data_dict.intr
    colmap_depth, colmap_conf = data_dict.colmap_depth, data_dict.colmap_conf
    B = pose.shape[0]
    if not _colmap_takes_kernel(colmap_depth, colmap_conf):
        loss, perc = _colmap_loop_torch(self, opt, data_dict, pose, intr, H, W, iteration)
        return edict(colmap_depth=loss), {'perc_col_depth': perc}, {}
    quota = opt.nerf.rand_rays // B
    index, count = ops.colmap_compact(colmap_depth)
    counts, perc = _read_counts(count, B, H * W, quota)                  # the one readback
    stats_dict = {'perc_col_depth': perc}
    rows, K = counts.rows, sum(counts.rows)
    if K == 0:
        return edict(colmap_depth=_zero_loss(self.device)), stats_dict, {}
    dev = colmap_depth.device
    outs = (torch.empty(K, device=dev, dtype=torch.int64), torch.empty(K, device=dev, dtype=torch.float32),
            torch.empty(K, device=dev, dtype=torch.float32))
    offs = [0]
    for k in rows:
        offs.append(offs[-1] + k)
    draws = [b for b in range(B) if counts.valid[b] > quota]
    gathered, rets = 0, []
    for b in range(B):
        if rows[b] == 0:
            continue
        if b >= gathered:
            sel = torch.randperm(counts.valid[b], device=self.device)[:quota] if counts.valid[b] > quota else None
            gathered = next((d for d in draws if d > b), B)
            ops.colmap_gather(index, count, sel, quota, offs[gathered] - offs[b], H, W, colmap_depth, colmap_conf, images=(b, gathered),
                              outs=tuple(o[offs[b]:offs[gathered]] for o in outs))
        rets.append(_render_rays(self, data_dict, pose, intr, H, W, iteration, b, outs[0][offs[b]:offs[b + 1]]))
    fine = 'depth_fine' in rets[0].keys()                                 # the first read: the deferred renders launch here, as one batch
    loss = sparse_depth_loss(outs[1], outs[2], counts, [r.depth for r in rets], [r.depth_fine for r in rets] if fine else None, batch_size=B)
    return edict(colmap_depth=loss), stats_dict, {}


_colmap = Patcher("sparf_amd.losses.install_colmap_depth", "uninstall_colmap_depth")


def install_colmap_depth(base_losses_module):
    """Opt-in, and independent of the other installs: put compute_colmap_depth_loss on `base_losses_module.SparseCOLMAPDepthLoss` under
    the name compute_loss until `uninstall_colmap_depth()`.  Nothing in this package calls it."""
    _colmap.guard()
    _colmap.put(base_losses_module.SparseCOLMAPDepthLoss, COLMAP_METHOD, compute_colmap_depth_loss)


def uninstall_colmap_depth():
    _colmap.restore()


# ================================================================================================ the depth-consistency front end and the ray sampler
# what runs in front of the renders.  DepthConsistencyLoss.sample_pose (depth_cons_loss.py:45-63: a readback of every
# pose, get_nearest_pose_ids in numpy, a blend and two pose_inverse_4x4 chains), the pose preparation of compute_loss and
# compute_loss_from_existing_pixels (:103-106, :168-174: a [0,0,0,1] row from numpy, repeat, cat, a batched inverse) and sample_rays
# (sampling_strategies.py:250-296: a host meshgrid of the whole image and a synchronous copy) become `sample_unseen_pose` (ops.unseen_pose,
# one launch) and `sample_pixels` (ops.pick_pixels, one launch behind one copy of the drawn permutation prefix);
# RaySamplingStrategy.__call__ (:132-188) takes the same kernel.  The random draws stay the reference's, on the generators and in the order
# and amounts it uses: they are the parity contract with an unmodified trainer.  The in-mask pool (cv2.dilate in the constructor) is not
# part of it: a config with sample_fraction_in_fg_mask > 0 is handed to the original method.
def _on_gpu(device):
    """the device test of the routes below (the tests' stand-in for the library replaces it)"""
    return device.type == "cuda"


def _centre_box(H, W, precrop_frac):
    """sampling_strategies.py:105-115, :265-271: the linspace centre box as (x0, y0, width, height); its values are exact integers"""
    dH, dW = int(H // 2 * precrop_frac), int(W // 2 * precrop_frac)
    return W // 2 - dW, H // 2 - dH, 2 * dW, 2 * dH


def _pick_counts(nbr, fraction_in_center):
    """(picks of the whole pool, picks of the centre box) of sample_rays / sample_rays_for_patch"""
    n_center = int(nbr * fraction_in_center) if fraction_in_center > 0. else 0
    return nbr - n_center, n_center


def _patched_torch(x_ind, y_ind, patch):
    """sampling_strategies.py:198-201, :240-243: every pick expanded by the patch offsets, dy outer, dx inner -> [n, patch^2, 2]"""
    r = torch.arange(patch, dtype=torch.long, device=x_ind.device)
    Y, X = torch.meshgrid(r, r, indexing="ij")
    x_ind = (x_ind[:, None].repeat(1, patch ** 2) + X.reshape(-1)).reshape(-1)
    y_ind = (y_ind[:, None].repeat(1, patch ** 2) + Y.reshape(-1)).reshape(-1)
    return torch.stack([x_ind, y_ind], dim=-1).reshape(-1, patch ** 2, 2)


def sample_pixels_torch(H, W, nbr=None, *, precrop_frac=0.5, fraction_in_center=0., patch_size=None, perm=None, perm_center=None, device=None):
    """sampling_strategies.py:250-296 sample_rays (patch_size None: -> pixels [n,2], rays [n]) and :191-247 sample_rays_for_patch
    (-> [n, patch^2, 2], [n, patch^2]) in the reference's operations: the pool of (H - 1)(W - 1) pixels, or (H - (patch - 1))(W - (patch
    - 1)); with a centre fraction int(nbr fraction) picks of the centre box behind nbr - that many of the pool; with nbr None nothing is
    drawn and the whole pool comes back, centre fraction or not.  perm / perm_center: the drawn prefixes (None: torch.randperm on the
    CPU generator, sliced, the pool's first).  pixels float32; rays int64 (the reference leaves float32 rays behind a centre fraction,
    the same integers)."""
    dev = ops._resolve(device if device is not None else perm.device if perm is not None else "cpu")
    border = 1 if patch_size is None else patch_size - 1
    Y, X = torch.meshgrid(torch.arange(H - border, dtype=torch.long), torch.arange(W - border, dtype=torch.long), indexing="ij")
    x_ind, y_ind = X.reshape(-1).to(dev), Y.reshape(-1).to(dev)
    if nbr is not None:
        n_all, n_center = _pick_counts(nbr, fraction_in_center)
        if perm is None:
            perm = torch.randperm(len(x_ind))[:n_all]
        perm = perm.to(dev)
        x_ind, y_ind = x_ind[perm], y_ind[perm]
        if fraction_in_center > 0.:
            x0, y0, bw, bh = _centre_box(H, W, precrop_frac)
            Yc, Xc = torch.meshgrid(torch.linspace(y0, y0 + bh - 1, bh), torch.linspace(x0, x0 + bw - 1, bw), indexing="ij")
            centre = torch.stack([Xc, Yc], -1).view(-1, 2)
            if perm_center is None:
                perm_center = torch.randperm(len(centre))[:n_center]
            centre = centre.to(dev)[perm_center.to(dev)].long()
            x_ind, y_ind = torch.cat((x_ind, centre[..., 0])), torch.cat((y_ind, centre[..., 1]))
    if patch_size is None:
        coords = torch.stack([x_ind, y_ind], dim=-1).reshape(len(x_ind), -1)
    else:
        coords = _patched_torch(x_ind, y_ind, patch_size)
    return coords.float(), coords[..., 1] * W + coords[..., 0]


def sample_pixels(H, W, nbr=None, *, precrop_frac=0.5, fraction_in_center=0., patch_size=None, perm=None, perm_center=None, device=None):
    """The pixels of sample_rays (patch_size None) / sample_rays_for_patch as `sample_pixels_torch` describes them, on `device`:
    -> (pixels float32, rays int64).  The permutations are drawn as the reference draws them -- torch.randperm of the pool on the CPU
    generator, the pool's before the centre box's, sliced -- and only the prefixes go to the device, in one non-blocking copy; one launch
    (ops.pick_pixels) writes both results.  Prefixes already on the device are used where they are.  CPU, nbr None and a centre box whose
    patches leave the image take the restatement."""
    H, W = int(H), int(W)
    dev = ops._resolve(device if device is not None else perm.device if perm is not None else "cpu")
    patch = 1 if patch_size is None else int(patch_size)
    border = 1 if patch_size is None else patch - 1
    a_w, a_h = W - border, H - border
    box = _centre_box(H, W, precrop_frac) if fraction_in_center > 0. else None
    takes = (not _unfused and _on_gpu(dev) and nbr is not None and patch >= 1 and a_w > 0 and a_h > 0 and
             all(t is None or (t.dtype == torch.int64 and t.dim() == 1) for t in (perm, perm_center)) and
             (box is None or (box[0] >= 0 and box[1] >= 0 and box[2] > 0 and box[3] > 0 and box[0] + box[2] + patch - 1 <= W)))
    if not takes:
        return sample_pixels_torch(H, W, nbr, precrop_frac=precrop_frac, fraction_in_center=fraction_in_center, patch_size=patch_size, perm=perm,
                                   perm_center=perm_center, device=dev)
    n_all, n_center = _pick_counts(nbr, fraction_in_center)
    if perm is None:
        perm = torch.randperm(a_w * a_h)[:n_all]
    if box is None:
        perm_center = None
    elif perm_center is None:
        perm_center = torch.randperm(box[2] * box[3])[:n_center]
    perm, perm_center = _prefixes_to(dev, perm, perm_center)
    pixels, rays = ops.pick_pixels(perm, perm_center, (a_w, a_h), box, W, patch, device=dev)
    if patch_size is None:
        return pixels, rays
    return pixels.reshape(-1, patch ** 2, 2), rays.reshape(-1, patch ** 2)


def _prefixes_to(dev, perm, perm_center):
    """both prefixes on `dev` (resolved: with its index): the ones elsewhere travel together, as one non-blocking copy"""
    there = lambda t: ops._resolve(t.device) == dev
    host = [t for t in (perm, perm_center) if t is not None and not there(t)]
    if not host:
        return perm, perm_center
    both = (host[0] if len(host) == 1 else torch.cat(host)).to(dev, non_blocking=True)
    parts = list(both.split([t.numel() for t in host]))
    take = lambda t: t if t is None or there(t) else parts.pop(0)
    return take(perm), take(perm_center)


def _pose_inverse_batched_torch(mat):
    """camera.py:44-55, the transpose form on [B,4,4]"""
    out = torch.zeros_like(mat)
    out[:, 3, 3] = 1
    R_inv = mat[:, :3, :3].transpose(-1, -2)
    out[:, :3] = torch.cat([R_inv, (-R_inv @ mat[:, :3, 3:])[..., 0][..., None]], dim=-1)
    return out


def nearest_other_pose_torch(centres, id_self):
    """get_nearest_pose_ids (data_utils.py:248-311) with one neighbour, 'vector' and the scene centre 0, in float64 on the float32 camera
    centres [B,3] as numpy computes it; the self entry is 1e3.  -> the first index of the minimum, a 0-dim int32 tensor: no readback"""
    v = centres.double()
    unit = v / (((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).sqrt()[:, None] + 1e-6)
    p = unit[id_self][None] * unit
    dists = torch.acos(torch.clamp((p[:, 0] + p[:, 1]) + p[:, 2], -1.0, 1.0))
    dists[id_self] = 1e3
    index = torch.arange(len(dists), device=dists.device)
    return torch.where(dists == dists.min(), index, len(dists)).min().to(torch.int32)


def _blend_and_invert_torch(pose_c2w_self, pose_c2w_other, w):
    """depth_cons_loss.py:61-62"""
    return pose_inverse_4x4_torch(w * pose_c2w_self + (1 - w) * pose_c2w_other)


def sample_unseen_pose_torch(poses_w2c, id_self, w):
    """The pose preparation of DepthConsistencyLoss.compute_loss (depth_cons_loss.py:168-174, :187-188) and sample_pose (:45-63) on
    poses_w2c [B,3,4] or [B,4,4], detached as the reference detaches them, in the reference's torch operations; the nearest search is
    `nearest_other_pose_torch`, with no numpy round trip.  -> edict(pose_w2c_ref, pose_c2w_ref, pose_c2w_other, pose_w2c_at_unseen [4,4];
    id_other, 0-dim int32 on the poses' device)."""
    from .edict import EasyDict as edict
    poses = poses_w2c.detach()
    if poses.shape[1] == 3:
        poses = torch.cat((poses, poses.new_tensor([0., 0., 0., 1.]).reshape(1, 1, 4).repeat(len(poses), 1, 1)), dim=1)
    poses_c2w = _pose_inverse_batched_torch(poses)
    id_other = nearest_other_pose_torch(poses_c2w[:, :3, 3], int(id_self))
    pose_w2c_ref = poses[id_self]
    pose_c2w_other = poses_c2w.index_select(0, id_other.long().reshape(1))[0]
    unseen = _blend_and_invert_torch(pose_inverse_4x4_torch(pose_w2c_ref), pose_c2w_other, w)
    return edict(pose_w2c_ref=pose_w2c_ref, pose_c2w_ref=poses_c2w[id_self], pose_c2w_other=pose_c2w_other, pose_w2c_at_unseen=unseen, id_other=id_other)


def sample_unseen_pose(poses_w2c, id_self, w):
    """An unseen pose between camera id_self and its nearest other camera, as DepthConsistencyLoss prepares and samples it: the four
    matrices and the index of `sample_unseen_pose_torch`, in one launch (ops.unseen_pose) and without a readback for float32 poses on
    the GPU that ask for no gradient; everything else takes the restatement."""
    from .edict import EasyDict as edict
    if _unfused or not (_on_gpu(poses_w2c.device) and poses_w2c.dtype == torch.float32 and poses_w2c.layout == torch.strided
                        and not (poses_w2c.requires_grad and torch.is_grad_enabled())):
        return sample_unseen_pose_torch(poses_w2c, id_self, w)
    out, id_other = ops.unseen_pose(poses_w2c, id_self, w)
    return edict(pose_w2c_ref=out[0], pose_c2w_ref=out[1], pose_c2w_other=out[2], pose_w2c_at_unseen=out[3], id_other=id_other[0])


# ---------------------------------------------------------------------------------------------- under the reference's names
def sample_pose(self, poses_c2w, id_self, pose_w2c_self):
    """DepthConsistencyLoss.sample_pose (depth_cons_loss.py:45-63) under its own signature: the camera-to-world poses are what it is
    handed, so the nearest search runs on their centres (`nearest_other_pose_torch`) and the blend and the inverse in the reference's
    operations; one np.random.rand(), as there; no readback.  -> pose_w2c_at_unseen [4,4]"""
    id_other = nearest_other_pose_torch(poses_c2w.detach()[:, :3, 3], int(id_self))
    w = np.random.rand()
    pose_c2w_other = poses_c2w.detach().index_select(0, id_other.long().reshape(1))[0]
    return _blend_and_invert_torch(pose_inverse_4x4_torch(pose_w2c_self).detach(), pose_c2w_other, w)


def _dcons_starts(opt, iteration):
    start = opt.start_ratio.depth_cons * opt.max_iter if opt.start_ratio.depth_cons is not None else opt.start_iter.depth_cons
    return iteration >= start


def _at_sampled_pose(self, data_dict, prep, pixels, depth_ref, intr_ref, H, W):
    """depth_cons_loss.py:115-125, :209-217: the pseudo ground-truth points, then whatever compute_loss_at_sampled_pose the class holds"""
    points = backproject_to_3d_torch(pixels, depth_ref, intr_ref, prep.pose_c2w_ref)
    return self.compute_loss_at_sampled_pose(data_dict, pose_w2c_at_unseen=prep.pose_w2c_at_unseen, intr_at_unseen=intr_ref.clone(),
                                             pseudo_gt_3dpts_in_w=points, H=H, W=W, pixels_in_ref=pixels)


def compute_loss_from_existing_pixels(self, opt, data_dict, iteration, pixels_in_ref, id_ref, depth_ref=None):
    """DepthConsistencyLoss.compute_loss_from_existing_pixels (depth_cons_loss.py:65-125) under its own signature and return convention;
    its one draw is np.random.rand()"""
    if not _dcons_starts(opt, iteration):
        return {}, {}, {}
    B, _, H, W = data_dict.image.shape
    prep = sample_unseen_pose(data_dict.poses_w2c.detach(), id_ref, np.random.rand())
    return _at_sampled_pose(self, data_dict, prep, pixels_in_ref, depth_ref, data_dict.intr[id_ref], H, W)


def dcons_compute_loss(self, opt, data_dict, output_dict, iteration, mode=None, plot=False, **kwargs):
    """DepthConsistencyLoss.compute_loss (depth_cons_loss.py:128-217) under its own signature and return convention.  The draws are the
    reference's, in its order: np.random.randint(B), the one or two CPU torch.randperm of sample_rays, and -- behind the reference render,
    as there -- np.random.rand().  Between entry and that render: one copy of the permutation prefix to the device and one launch; the
    render takes poses_w2c[id_self] where it lies; behind it one launch leaves every matrix.  Nothing is read back."""
    if mode != 'train':
        return {}, {}, {}
    if not _dcons_starts(opt, iteration):
        return {}, {}, {}
    B, _, H, W = data_dict.image.shape
    poses_w2c = data_dict.poses_w2c.detach()
    id_self = np.random.randint(B)
    pixels_ref, _ = sample_pixels(H, W, nbr=max(1024, self.opt.nerf.rand_rays), fraction_in_center=self.opt.sampled_fraction_in_center,
                                  device=self.device)
    intr_ref = data_dict.intr[id_self]
    ret_ref = self.net.render_image_at_specific_pose_and_rays(self.opt, data_dict, pose=poses_w2c[id_self][:3], intr=intr_ref, H=H, W=W,
                                                              pixels=pixels_ref, mode='train', iter=iteration)
    fine = 'depth_fine' in ret_ref.keys()
    if fine and hasattr(opt.nerf, 'ratio_start_fine_sampling_at_x') and opt.nerf.ratio_start_fine_sampling_at_x is not None \
            and iteration < opt.max_iter * (opt.nerf.ratio_start_fine_sampling_at_x + 0.05):
        fine = False
    depth_ref = (ret_ref.depth_fine if fine else ret_ref.depth).squeeze(0).squeeze(-1)
    prep = sample_unseen_pose(poses_w2c, id_self, np.random.rand())
    return _at_sampled_pose(self, data_dict, prep, pixels_ref, depth_ref, intr_ref, H, W)


DCONS_SAMPLER_METHODS = {"sample_pose": sample_pose, "compute_loss": dcons_compute_loss,
                         "compute_loss_from_existing_pixels": compute_loss_from_existing_pixels}
_dcons_sampler = Patcher("sparf_amd.losses.install_depth_consistency_sampler", "uninstall_depth_consistency_sampler")


def install_depth_consistency_sampler(depth_cons_loss_module):
    """Opt-in, and independent of install_depth_consistency() (the methods here call whatever compute_loss_at_sampled_pose the class
    holds when they run, so the two compose in either order): put sample_pose, compute_loss and compute_loss_from_existing_pixels on
    `depth_cons_loss_module.DepthConsistencyLoss` until `uninstall_depth_consistency_sampler()`.  Nothing in this package calls it."""
    _dcons_sampler.guard()
    for name, fn in DCONS_SAMPLER_METHODS.items():
        _dcons_sampler.put(depth_cons_loss_module.DepthConsistencyLoss, name, fn)


def uninstall_depth_consistency_sampler():
    _dcons_sampler.restore()


RAY_SAMPLER_METHOD = "__call__"
_ray_sampler = Patcher("sparf_amd.losses.install_ray_sampler", "uninstall_ray_sampler")     # keeps the class's own __call__: the in-mask configs are handed to it


def ray_sampler_call(self, nbr_pixels, sample_in_center=False, idx_imgs=None):
    """RaySamplingStrategy.__call__ (sampling_strategies.py:132-188) under its own signature: the same device torch.randperm draws, the
    centre fraction's before the main one, and the same rays, in one launch (ops.pick_pixels) instead of two index operations, the patch
    expansion and the ray arithmetic.  The pools are rectangles: the grid behind self.all_possible_pixels and the centre box behind
    self.all_center_pixels.  A config with sample_fraction_in_fg_mask > 0, a sampler off the GPU and pools of another size than their
    rectangles are handed to the original method."""
    original = _ray_sampler.original(RAY_SAMPLER_METHOD)
    opt, H, W = self.opt, self.H, self.W
    dev = ops._resolve(self.device)
    patch = opt.depth_regu_patch_size if opt.loss_weight.depth_patch is not None else None
    p = 1 if patch is None else int(patch)
    a_w, a_h = (W, H) if patch is None else (W - p - 1, H - p - 1)
    box = _centre_box(H, W, opt.precrop_frac)
    if (opt.sample_fraction_in_fg_mask > 0. or _unfused or not _on_gpu(dev) or a_w <= 0 or a_h <= 0 or len(self.all_possible_pixels) != a_w * a_h
            or len(self.all_center_pixels) != box[2] * box[3] or box[2] <= 0 or box[3] <= 0 or box[0] + box[2] + p - 1 > W):
        return original(self, nbr_pixels, sample_in_center=sample_in_center, idx_imgs=idx_imgs)
    nbr_images = self.nbr_images if idx_imgs is None else len(idx_imgs)
    n_rand = nbr_pixels // nbr_images
    if patch is not None:
        n_rand = n_rand // p ** 2
    perm_center = None
    if opt.sampled_fraction_in_center > 0:
        n_center = int(n_rand * opt.sampled_fraction_in_center)
        n_rand = n_rand - n_center
        perm_center = torch.randperm(box[2] * box[3], device=dev)[:n_center]
    if sample_in_center:                                # the main picks are of the centre box too, and come first
        perm = torch.randperm(box[2] * box[3], device=dev)[:n_rand]
        perm_a, perm_b = None, perm if perm_center is None else torch.cat((perm, perm_center))
    else:
        perm_a, perm_b = torch.randperm(a_w * a_h, device=dev)[:n_rand], perm_center
    return ops.pick_pixels(perm_a, perm_b, (a_w, a_h), box, W, p, pixels=False, device=dev)[1]


def install_ray_sampler(sampling_module):
    """Opt-in, and independent of the other installs: put the method above on `sampling_module.RaySamplingStrategy` until
    `uninstall_ray_sampler()`.  Nothing in this package calls it."""
    _ray_sampler.guard()
    cls = sampling_module.RaySamplingStrategy
    _ray_sampler.save(RAY_SAMPLER_METHOD, cls.__call__)
    _ray_sampler.put(cls, RAY_SAMPLER_METHOD, ray_sampler_call)


def uninstall_ray_sampler():
    _ray_sampler.restore()
