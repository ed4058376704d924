"""The correspondence loss: SPARF's re-projection of rendered depth at matched pixels through the current relative
pose (corres_loss.py:50-95, :183-219; batched_geometry_utils.py:199-228; base_losses.py:197-224).

The sampler, the renders and the autograd graph stay PyTorch's.  The BODY -- four re-projection terms and the two compositions of the
relative pose -- is one library call behind ops.ReprojLoss / ops.ReprojPairLoss for dense-able float32 tensors on the GPU, and a plain
torch restatement of the same formulas, in this file, for everything else: CPU, float64, intrinsics / pixels / weights that require a
gradient (the kernels give none to them), and `unfused()`.  `install()` puts the method under a trainer's own name.  Nothing in this
package calls any of it; there is no `opt.hip` key.
"""
import contextlib

import torch

from . import ops

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
_patched = []


def install(corres_loss_module):
    """Opt-in: put the method above on `corres_loss_module.CorrespondencesPairRenderDepthAndGet3DPtsAndReproject` until `uninstall()`.
    Nothing in this package calls it."""
    if _patched:
        raise RuntimeError("sparf_amd.losses.install: already installed; call uninstall() first")
    cls = corres_loss_module.CorrespondencesPairRenderDepthAndGet3DPtsAndReproject
    _patched.append((cls, METHOD, METHOD in vars(cls), vars(cls).get(METHOD)))
    setattr(cls, METHOD, compute_render_and_repro_loss_w_repro_thres)


def uninstall():
    while _patched:
        obj, name, own, old = _patched.pop()
        if own:
            setattr(obj, name, old)
        else:
            delattr(obj, name)
