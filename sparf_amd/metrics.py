"""Evaluation metrics: what the reference's trainers run on every validation step and every test view --
compute_metrics / compute_metrics_masked / compute_depth_error (source/training/core/metrics.py:136-268; base.py:475-499,
nerf_trainer.py:387-405) with the SSIM of third_party/pytorch_ssim/ssim.py -- as ONE library call for both heads (ops.image_metrics:
csrc/metrics.hip), and a plain torch restatement of the same lines, in this file, for everything the kernel does not take: CPU tensors,
operands that are not float32, one-channel images, a float mask, and `unfused()`.

`image_metrics` returns device tensors and reads nothing back.  `compute_metrics`, `compute_metrics_masked` and `ssim` carry the
reference's own signatures, key names and return types; `install()` puts them under the reference's names on the modules that imported
them.  LPIPS stays the caller's callable.  Nothing in this package calls install(); there is no `opt.hip` key.

Depth errors on rendered rays: compute_depth_error_on_rays (metrics.py:81-134), what the trainers log on every
training iteration, as ONE library call for both heads without a readback (ops.ray_depth_err: csrc/depth_err.hip) -- `depth_error_on_rays`,
its restatement `depth_error_on_rays_torch`, `compute_depth_error_on_rays` under the reference's signature, and
`install_depth_error_on_rays()` with a patcher of its own.
"""
import contextlib
import math

import torch

from . import ops
from .edict import EasyDict as edict
from .patcher import Patcher

OUTS = ops.METRICS_OUTS
WINDOW_SIZE, SIGMA = 11, 1.5
_unfused = 0


@contextlib.contextmanager
def unfused():
    """Inside the block everything below takes its torch restatement, whatever its inputs (tools/image_metrics_bench.py --leg series)."""
    global _unfused
    _unfused += 1
    try:
        yield
    finally:
        _unfused -= 1


# ---------------------------------------------------------------------------------------------- the torch restatement
def gaussian_window(window_size=WINDOW_SIZE, sigma=SIGMA):
    """ssim.py:8-10: float32 weights, normalised in float32"""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)], dtype=torch.float32)
    return g / g.sum()


def window_2d(window_size, channel):
    """ssim.py:12-16: the outer product in float32, one copy per channel [C,1,K,K]"""
    g = gaussian_window(window_size).unsqueeze(1)
    return g.mm(g.t()).float()[None, None].expand(channel, 1, window_size, window_size).contiguous()


def ssim_torch(img1, img2, window_size=WINDOW_SIZE, size_average=True):
    """ssim.py:18-50 in the reference's operation order: five grouped convolutions with zero padding, then the map"""
    channel = img1.shape[1]
    assert (img1.shape[1] == 3 or img1.shape[1] == 1) and (img2.shape[1] == 3 or img2.shape[1] == 1)
    window = window_2d(window_size, channel).to(img1.device).type_as(img1)
    conv = lambda x: torch.nn.functional.conv2d(x, window, padding=window_size // 2, groups=channel)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(img1 * img1) - mu1_sq
    sigma2_sq = conv(img2 * img2) - mu2_sq
    sigma12 = conv(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean() if size_average else ssim_map


def _mse_torch(pred, label, mask=None):
    """MSE_loss (metrics.py:26-31); mask [B,1,H,W] bool selects elements"""
    loss = (pred.contiguous() - label) ** 2
    if mask is not None:
        loss = loss[mask.repeat(1, loss.shape[1], 1, 1)]
    return loss.mean()


def _composites(pred, gt, mask_float):
    """metrics.py:208-209"""
    return pred * mask_float + (1. - mask_float), gt * mask_float + (1. - mask_float)


def _depth_errors_torch(depth_gt, pred_depth):
    """compute_metric of metrics.py:158-165 on the selected pixels, without its readbacks"""
    abs_e = torch.abs(depth_gt - pred_depth)
    abs_e = abs_e.sum() / (abs_e.nelement() + 1e-6)
    return abs_e, torch.sqrt((depth_gt - pred_depth).pow(2).mean())


def _mask4(fg_mask, B, H, W):
    return fg_mask.reshape(B, 1, H, W)


def image_metrics_torch(pred, gt, *, pred_fine=None, fg_mask=None, depth=None, depth_fine=None, depth_gt=None, valid_depth_gt=None,
                        depth_scale=1.0):
    """The torch restatement of image_metrics: the reference's lines in the reference's order, in the operands' own dtype.
    -> the same dict; the float32 rounding of `vector` is the only thing added."""
    B, _, H, W = gt.shape
    nan = torch.full((), float("nan"), device=gt.device, dtype=gt.dtype)
    rows = []
    n_fg = n_valid = 0
    if fg_mask is not None:
        mask_float = _mask4(fg_mask, B, H, W).to(gt.dtype)
        mask = mask_float == 1.
        n_fg = mask.sum()
    if depth_gt is not None:
        valid = valid_depth_gt.reshape(B, -1).bool() if valid_depth_gt is not None else torch.ones(B, H * W, dtype=torch.bool, device=gt.device)
        gt_sel = depth_gt.reshape(B, -1, 1)[valid]
        n_valid = valid.sum()
    for p, d in ((pred, depth), (pred_fine, depth_fine)):
        if p is None:
            rows.append(torch.stack([nan] * len(OUTS)))
            continue
        mse = _mse_torch(p, gt)
        row = [mse, -10 * mse.log10(), ssim_torch(p, gt)]
        if fg_mask is not None:
            p_fg, gt_fg = _composites(p, gt, mask_float)
            mse_m = _mse_torch(p_fg, gt_fg, mask)
            row += [mse_m, -10 * mse_m.log10(), ssim_torch(p_fg, gt_fg)]
        else:
            row += [nan] * 3
        if d is not None:
            if depth_gt is None:
                raise ValueError("image metrics: a depth needs depth_gt")
            d_sel = d.reshape(B, -1, 1)[valid]
            row += [*_depth_errors_torch(gt_sel, d_sel), *_depth_errors_torch(gt_sel, d_sel.clone() * depth_scale)]
        else:
            row += [nan] * 4
        rows.append(torch.stack([r.to(gt.dtype) for r in row]))
    vector = torch.stack(rows).float()
    counts = torch.stack([torch.as_tensor(n_fg, device=gt.device), torch.as_tensor(n_valid, device=gt.device)]).to(torch.int32)
    return _result(vector, counts, pred_fine is not None, fg_mask is not None, (depth is not None, depth_fine is not None))


# ---------------------------------------------------------------------------------------------- the public functions
def _result(vector, counts, fine, masked, depths):
    """vector [2,10] / counts [2] -> dict of 0-dim views under the names of OUTS (`_fine` for the second head) for what was asked for,
    with n_fg / n_valid, the vector and the counts themselves"""
    res = edict(vector=vector, counts=counts)
    for h, sfx in enumerate(("", "_fine")[:2 if fine else 1]):
        for i, key in enumerate(OUTS):
            if i < 3 or (i < 6 and masked) or (i >= 6 and depths[h]):
                res[key + sfx] = vector[h, i]
    if masked:
        res.n_fg = counts[0]
    if any(depths):
        res.n_valid = counts[1]
    return res


def _takes_kernel(pred, gt, pred_fine, fg_mask, depths, depth_gt, valid_depth_gt):
    """float32 three-channel images, float32 depths, a bool (or 0/1 byte) mask, all on the GPU"""
    if _unfused:
        return False
    on_gpu = lambda t: t.device.type == "cuda" and t.layout == torch.strided
    f32 = lambda t: t is None or (on_gpu(t) and t.dtype == torch.float32)
    byte = lambda t: t is None or (on_gpu(t) and t.dtype in (torch.bool, torch.uint8))
    return (gt.dim() == 4 and gt.shape[1] == 3 and pred.shape == gt.shape and all(f32(t) for t in (pred, gt, pred_fine, depth_gt, *depths)) and
            byte(fg_mask) and byte(valid_depth_gt) and (fg_mask is None or fg_mask.numel() == gt.shape[0] * gt.shape[2] * gt.shape[3]))


def image_metrics(pred, gt, *, pred_fine=None, fg_mask=None, depth=None, depth_fine=None, depth_gt=None, valid_depth_gt=None, depth_scale=1.0):
    """PSNR, SSIM, their foreground-masked variants and the depth errors of one or two predicted images against one ground truth:
    pred / pred_fine / gt [B,3,H,W] in any strides (a channel-last render under a permuted view is read in place); fg_mask torch.bool
    [B,1,H,W] or [B,H,W]; depth / depth_fine [B,H W,1] with depth_gt and valid_depth_gt (bool) of as many elements; depth_scale the
    similarity scale of the prediction.
    -> dict of 0-dim device tensors: mse, psnr, ssim; with fg_mask mse_masked, psnr_masked, ssim_masked; with a depth abs_e, rmse,
    abs_e_scaled, rmse_scaled; each again with `_fine` for pred_fine; n_fg, n_valid (int32); `vector` [2,10] float32 and `counts` [2]
    hold all of it (a row per head, NaN for what was not asked for).  One kernel call, no readback."""
    if not _takes_kernel(pred, gt, pred_fine, fg_mask, (depth, depth_fine), depth_gt, valid_depth_gt):
        return image_metrics_torch(pred, gt, pred_fine=pred_fine, fg_mask=fg_mask, depth=depth, depth_fine=depth_fine, depth_gt=depth_gt,
                                   valid_depth_gt=valid_depth_gt, depth_scale=depth_scale)
    vector, counts = ops.image_metrics(pred, gt, pred_fine, fg_mask, depth, depth_fine, depth_gt, valid_depth_gt, depth_scale)
    return _result(vector, counts, pred_fine is not None, fg_mask is not None, (depth is not None, depth_fine is not None))


def ssim(img1, img2, window_size=WINDOW_SIZE, size_average=True):
    """third_party.pytorch_ssim.ssim.ssim (ssim.py:41-50): the mean SSIM as a 0-dim tensor.  Another window size, the map itself
    (size_average=False) or a gradient asked of an image take the restatement."""
    wants_grad = torch.is_grad_enabled() and (img1.requires_grad or img2.requires_grad)
    if window_size != WINDOW_SIZE or not size_average or wants_grad or img1.shape != img2.shape or \
            not _takes_kernel(img1, img2, None, None, (), None, None):
        return ssim_torch(img1, img2, window_size, size_average)
    return image_metrics(img1, img2).ssim


# ---------------------------------------------------------------------------------------------- under the reference's names
_installer = Patcher("sparf_amd.metrics.install", "uninstall")     # keeps the reference's own functions: a three-channel mask is handed to them
NAMES = ("compute_metrics", "compute_metrics_masked", "ssim_loss")


def _handed_over(name):
    original = _installer.original(name)
    if original is None:
        raise RuntimeError(f"sparf_amd.metrics.{name}: a three-channel fg_mask goes to the reference's own function and there is none "
                           "(install() saves it)")
    return original


def _three_channel(data_dict):
    return 'fg_mask' in data_dict.keys() and data_dict.fg_mask.dim() == 4 and data_dict.fg_mask.shape[1] != 1


def compute_metrics_masked(data_dict, pred_rgb_map, gt_rgb_map, lpips_loss, suffix=''):
    """metrics.py:186-215 under its own signature: a dict of Python floats psnr_masked, ssim_masked, lpips_masked (+ suffix).  One
    kernel call and one readback of its vector; lpips_loss is called as the reference calls it, on the composites x 2 - 1."""
    assert 'fg_mask' in data_dict.keys()
    if _three_channel(data_dict):
        return _handed_over("compute_metrics_masked")(data_dict, pred_rgb_map, gt_rgb_map, lpips_loss, suffix)
    res = image_metrics(pred_rgb_map, gt_rgb_map, fg_mask=data_dict.fg_mask)
    v = res.vector[0].tolist()
    mask_float = data_dict.fg_mask.float()
    rgb_map_fg, gt_rgb_map_fg = _composites(pred_rgb_map, gt_rgb_map, mask_float)
    lpips_masked = lpips_loss(rgb_map_fg * 2 - 1, gt_rgb_map_fg * 2 - 1).item()
    return {'psnr_masked' + suffix: v[4], 'ssim_masked' + suffix: v[5], 'lpips_masked' + suffix: lpips_masked}


def compute_metrics(data_dict, output_dict, pred_rgb_map, pred_depth, gt_rgb_map, lpips_loss, scaling_factor_for_pred_depth=1., suffix=''):
    """metrics.py:217-268 under its own signature: an edict of Python floats psnr, ssim, lpips, abse_depth, rmse_depth and, with
    data_dict.fg_mask, the three masked ones (+ suffix).  One kernel call and one readback of its vector."""
    if _three_channel(data_dict):
        return _handed_over("compute_metrics")(data_dict, output_dict, pred_rgb_map, pred_depth, gt_rgb_map, lpips_loss,
                                               scaling_factor_for_pred_depth, suffix)
    masked, with_depth = 'fg_mask' in data_dict.keys(), 'depth_gt' in data_dict.keys()
    kw = {}
    if with_depth:
        idx = output_dict.idx_img_rendered
        B = len(idx)
        kw = dict(depth=pred_depth.view(B, -1, 1), depth_gt=data_dict.depth_gt[idx].view(B, -1, 1), valid_depth_gt=data_dict.valid_depth_gt[idx].view(B, -1),
                  depth_scale=scaling_factor_for_pred_depth)
    res = image_metrics(pred_rgb_map, gt_rgb_map, fg_mask=data_dict.fg_mask if masked else None, **kw)
    v = res.vector[0].tolist()
    lpips = lpips_loss(pred_rgb_map * 2 - 1, gt_rgb_map * 2 - 1).item()
    abs_e, rmse = float('nan'), float('nan')
    if with_depth:
        abs_e, rmse = v[6], v[7]
        if scaling_factor_for_pred_depth != 1.:
            # metrics.py:253-257 on :176-180: Python's min in the reference's argument order (it matters for a NaN)
            abs_e = min(abs_e, min(abs_e, v[8]))
            rmse = min(rmse, min(rmse, v[9]))
    results = edict({'psnr' + suffix: v[1], 'ssim' + suffix: v[2], 'lpips' + suffix: lpips, 'abse_depth' + suffix: abs_e, 'rmse_depth' + suffix: rmse})
    if masked:
        mask_float = data_dict.fg_mask.float()
        rgb_map_fg, gt_rgb_map_fg = _composites(pred_rgb_map, gt_rgb_map, mask_float)
        lpips_masked = lpips_loss(rgb_map_fg * 2 - 1, gt_rgb_map_fg * 2 - 1).item()
        results.update({'psnr_masked' + suffix: v[4], 'ssim_masked' + suffix: v[5], 'lpips_masked' + suffix: lpips_masked})
    return results


# ---------------------------------------------------------------------------------------------- depth errors on rendered rays
# compute_depth_error_on_rays (metrics.py:81-134), what make_result_dict runs once per head on every training
# iteration (nerf_trainer.py:307-325), as ONE library call for both heads (ops.ray_depth_err: csrc/depth_err.hip), with its restatement.
def _rays_head_torch(depth_gt_maps, valid_maps, idx_img_rendered, ray_idx, pred_depth, scaling_factor_for_pred_depth):
    """metrics.py:103-134 for one head, line by line, on the maps of the scene -> (abs_e, rmse, the selection)"""
    B = len(idx_img_rendered)
    depth_gt = depth_gt_maps[idx_img_rendered].view(B, -1, 1)
    valid_depth = valid_maps[idx_img_rendered].view(B, -1)
    pred_depth = pred_depth.view(B, -1, 1)
    if ray_idx is not None:
        if len(ray_idx.shape) == 2 and ray_idx.shape[0] == B:
            n_rays = ray_idx.shape[-1]
            batch_idx_flattened = torch.arange(start=0, end=B).unsqueeze(-1).repeat(1, n_rays).long().view(-1)
            ray_idx_flattened = ray_idx.reshape(-1).long()
            depth_gt = depth_gt[batch_idx_flattened, ray_idx_flattened]
            depth_gt = depth_gt.reshape(B, n_rays, -1)
            valid_depth = valid_depth[batch_idx_flattened, ray_idx_flattened]
            valid_depth = valid_depth.reshape(B, n_rays, -1)
        else:
            depth_gt = depth_gt[:, ray_idx]
            valid_depth = valid_depth[:, ray_idx]
    depth_gt = depth_gt[valid_depth]
    pred_depth = pred_depth[valid_depth] * scaling_factor_for_pred_depth
    abs_e = torch.abs(depth_gt - pred_depth)
    abs_e = abs_e.sum() / (abs_e.nelement() + 1e-6)
    rmse = torch.sqrt((depth_gt - pred_depth).pow(2).mean())         # compute_rmse(depth_gt, pred_depth), metrics.py:78-79
    return abs_e, rmse, valid_depth


def _rays_maps(depth_gt, valid_depth_gt):
    """the maps as data_dict holds them; without a mask every pixel is valid"""
    if valid_depth_gt is None:
        valid_depth_gt = torch.ones(depth_gt.shape, dtype=torch.bool, device=depth_gt.device)
    return depth_gt, valid_depth_gt.reshape(depth_gt.shape).bool()


def _rays_result(vector, count, fine):
    """vector [4] / count [1] -> dict of 0-dim views: abs_e, rmse, with a fine head abs_e_fine, rmse_fine, and n_valid"""
    res = edict(vector=vector, count=count)
    for i, key in enumerate(ops.DEPTH_ERR_OUTS[:4 if fine else 2]):
        res[key] = vector[i]
    res.n_valid = count[0]
    return res


def depth_error_on_rays_torch(depth_gt, valid_depth_gt, depth, depth_fine=None, *, ray_idx=None, img_idx=None, scale=1.0):
    """The torch restatement of depth_error_on_rays: the reference's lines in the reference's order, once per head, in the operands' own
    dtype, with their indexed copies and the readbacks of their boolean selections.  -> the same dict; the float32 rounding of `vector`
    is the only thing added."""
    maps, valid = _rays_maps(depth_gt, valid_depth_gt)
    idx = img_idx if img_idx is not None else torch.arange(depth.shape[0], device=depth_gt.device)
    values, kept = [], None
    for d in (depth, depth_fine):
        if d is None:
            values += [torch.zeros((), device=depth_gt.device, dtype=depth_gt.dtype)] * 2
            continue
        abs_e, rmse, kept = _rays_head_torch(maps, valid, idx, ray_idx, d, scale)
        values += [abs_e, rmse]
    vector = torch.stack([v.to(depth_gt.dtype) for v in values]).float()
    return _rays_result(vector, kept.sum().to(torch.int32).reshape(1), depth_fine is not None)


def _on_gpu(device):
    return device.type == "cuda"


def _rays_take_kernel(depth_gt, valid_depth_gt, depths, ray_idx, img_idx, scale):
    """float32 maps and depths, a bool (or 0/1 byte) mask and int64 indices, all on one GPU, and no gradient asked of a depth"""
    if _unfused:
        return False
    dev = depth_gt.device
    here = lambda t, dtypes: t is None or (t.device == dev and t.layout == torch.strided and t.dtype in dtypes)
    depths = [d for d in depths if d is not None]
    if torch.is_grad_enabled() and any(d.requires_grad for d in depths):
        return False
    if torch.is_tensor(scale) and (scale.numel() != 1 or scale.is_complex()):
        return False
    B = depths[0].shape[0]
    return (_on_gpu(dev) and all(here(t, (torch.float32,)) for t in (depth_gt, *depths)) and here(valid_depth_gt, (torch.bool, torch.uint8)) and
            here(ray_idx, (torch.int64,)) and here(img_idx, (torch.int64,)) and
            (ray_idx is None or ray_idx.dim() == 1 or (ray_idx.dim() == 2 and ray_idx.shape[0] == B)))


def depth_error_on_rays(depth_gt, valid_depth_gt, depth, depth_fine=None, *, ray_idx=None, img_idx=None, scale=1.0):
    """The depth errors of one or two rendered heads against the ground-truth maps of the scene, on the rendered rays only:
    depth_gt [B_maps,H,W] or [B_maps,1,H,W] float32 and valid_depth_gt (bool, as many elements; None: every pixel) are read in place;
    depth / depth_fine [B,N,1] or [B,N]; ray_idx int64 [N] (one list for all images), [B,N] (two-dimensional with shape[0] == B: one
    list per image, the reference's rule) or None (full images); img_idx int64 [B] on the device names the map of each rendered image
    (None: the first B maps in order); scale a Python or numpy number or a one-element tensor (one on the GPU is never read back).
    -> dict of 0-dim device tensors abs_e, rmse, with depth_fine abs_e_fine, rmse_fine, and n_valid (int32): views of `vector` [4]
    and `count` [1].  One kernel call, no readback.  Another dtype, a tensor off the GPU, `unfused()` or a gradient asked of a depth
    take depth_error_on_rays_torch."""
    if not _rays_take_kernel(depth_gt, valid_depth_gt, (depth, depth_fine), ray_idx, img_idx, scale):
        return depth_error_on_rays_torch(depth_gt, valid_depth_gt, depth, depth_fine, ray_idx=ray_idx, img_idx=img_idx, scale=scale)
    vector, count = ops.ray_depth_err(depth_gt, valid_depth_gt, depth, depth_fine, ray_idx, img_idx, scale)
    return _rays_result(vector, count, depth_fine is not None)


def compute_depth_error_on_rays(data_dict, output_dict, pred_depth, scaling_factor_for_pred_depth=1.):
    """metrics.py:81-134 under its own signature: (abs_e, rmse) as 0-dim tensors for the one head it is given.  One kernel call and no
    readback: output_dict.idx_img_rendered goes to the kernel as it is where it is a device tensor; a host list is uploaded, unless it
    names every rendered image in order (then the kernel needs no index)."""
    idx = output_dict.idx_img_rendered
    ray_idx = output_dict.ray_idx if 'ray_idx' in output_dict.keys() else None
    depth_gt, valid = data_dict.depth_gt, data_dict.valid_depth_gt
    B = len(idx)
    on_host = not torch.is_tensor(idx) or (idx.device.type == "cpu" and idx.device != depth_gt.device)
    if not _rays_take_kernel(depth_gt, valid, (pred_depth,), ray_idx, None if on_host else idx, scaling_factor_for_pred_depth) or pred_depth.shape[0] != B:
        abs_e, rmse, _ = _rays_head_torch(depth_gt, valid, idx, ray_idx, pred_depth, scaling_factor_for_pred_depth)
        return abs_e, rmse
    if on_host:
        listed = [int(i) for i in idx]
        idx = None if listed == list(range(B)) else torch.tensor(listed, dtype=torch.int64, device=depth_gt.device)
    vector, _ = ops.ray_depth_err(depth_gt, valid, pred_depth, None, ray_idx, idx, scaling_factor_for_pred_depth)
    return vector[0], vector[1]


_rays_installer = Patcher("sparf_amd.metrics.install_depth_error_on_rays", "uninstall_depth_error_on_rays")
RAYS_NAME = "compute_depth_error_on_rays"


def install_depth_error_on_rays(metrics_module, *importing_modules):
    """Opt-in, and independent of install(): put compute_depth_error_on_rays above under that name on `metrics_module`
    (source.training.core.metrics) and on every module given whose own namespace holds the name (nerf_trainer imports it by name),
    until `uninstall_depth_error_on_rays()`.  Nothing in this package calls it."""
    _rays_installer.guard()
    if hasattr(metrics_module, RAYS_NAME):
        _rays_installer.save(RAYS_NAME, getattr(metrics_module, RAYS_NAME))
    _rays_installer.put(metrics_module, RAYS_NAME, compute_depth_error_on_rays)
    for mod in importing_modules:
        if RAYS_NAME in vars(mod):
            _rays_installer.put(mod, RAYS_NAME, compute_depth_error_on_rays)


def uninstall_depth_error_on_rays():
    _rays_installer.restore()


def install(metrics_module, *importing_modules):
    """Opt-in: put compute_metrics, compute_metrics_masked and ssim (as `ssim_loss`) above under those names on `metrics_module`
    (source.training.core.metrics) and on every module given that imported one of them (base, nerf_trainer), until `uninstall()`.
    Nothing in this package calls it."""
    _installer.guard()
    ours = dict(compute_metrics=compute_metrics, compute_metrics_masked=compute_metrics_masked, ssim_loss=ssim)
    for name in NAMES:
        if hasattr(metrics_module, name):
            _installer.save(name, getattr(metrics_module, name))
    for mod in (metrics_module, *importing_modules):
        for name in NAMES:
            if name in vars(mod):
                _installer.put(mod, name, ours[name])


def uninstall():
    _installer.restore()
