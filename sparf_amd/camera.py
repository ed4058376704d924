"""Ray generation: the boundary feeder of the hot path.

Stays in PyTorch on purpose (north_star: pose SE(3) machinery and autograd to the pose
parameters live in PyTorch); mirrors /root/reference/source/utils/camera.py:296-416.
Unlike the reference, rays are built only for the requested pixels instead of all H*W
pixels of every image followed by an index (renderer.py:273-291) -- same values, ~100x
less work.

Pose parameterisations, second half of the file: the parameters, their
optimiser and the autograd graph stay PyTorch's; the BODY of se3_to_SE3, compose_pair_b_at_a
and r6d2mat (+ concatenation, + inversion) is one kernel per direction behind ops.Se3Pose /
ComposePose / D9Pose for dense float32 tensors on the GPU, and a plain torch restatement of
the same formulas for everything else.  `install()` puts them under a trainer's own names.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

from . import ops
from .patcher import Patcher


def to_hom(X):
    return torch.cat([X, torch.ones_like(X[..., :1])], dim=-1)


def invert_pose(pose):
    """[...,3,4] rigid transform -> its inverse (camera.py Pose.invert)."""
    R, t = pose[..., :3], pose[..., 3:]
    R_inv = R.transpose(-1, -2)
    return torch.cat([R_inv, -R_inv @ t], dim=-1)


def _intr_inverse(cam_intr):
    """K^-1 of [...,3,3] intrinsics.  torch.linalg.inv synchronises with the host (LAPACK-style info check) and cannot be
    captured in a hipGraph, so a non-differentiable K is inverted in closed form -- the adjugate over the determinant, in
    float64 like the fused ray-generation kernel (csrc/ray_ops.hip) -- from the tensor's CURRENT values on every call.
    (Round 3 cached the inverse by (data_ptr, _version, shape): a freed and re-allocated intrinsics tensor at the same
    address with other values returned a stale inverse.)"""
    if cam_intr.requires_grad:
        return cam_intr.inverse()
    K = cam_intr.double()
    r0, r1, r2 = K[..., 0, :], K[..., 1, :], K[..., 2, :]
    c0, c1, c2 = torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)
    det = (r0 * c0).sum(-1, keepdim=True)
    return (torch.stack([c0, c1, c2], dim=-1) / det[..., None]).to(cam_intr.dtype)


def img2cam(X, cam_intr):
    return X @ _intr_inverse(cam_intr).transpose(-1, -2)


def cam2world(X_cam, pose_w2c):
    return to_hom(X_cam) @ invert_pose(pose_w2c).transpose(-1, -2)


def get_center_and_ray_at_pixels(pose_w2c, pixels, intr):
    """pixels [N,2] or [B,N,2] (x,y) used as given -- no +0.5 (camera.py:384-416).
    Returns center, ray [B,N,3]; ray = R_c2w K^-1 [x,y,1] is NOT normalised."""
    B = len(pose_w2c)
    xy = pixels.unsqueeze(0).repeat(B, 1, 1) if pixels.dim() == 2 else pixels
    grid_3D = img2cam(to_hom(xy.to(pose_w2c.dtype)), intr)
    center_3D = cam2world(torch.zeros_like(grid_3D), pose_w2c)
    grid_3D = cam2world(grid_3D, pose_w2c)
    return center_3D, grid_3D - center_3D


def pixel_centers(ray_idx, W, dtype):
    """flat pixel index -> (x+0.5, y+0.5), the grid of camera.py:365-368."""
    ray_idx = ray_idx.long()
    x = (ray_idx % W).to(dtype) + 0.5
    y = torch.div(ray_idx, W, rounding_mode="floor").to(dtype) + 0.5
    return torch.stack([x, y], dim=-1)


def get_center_and_ray(pose_w2c, H, W, intr, ray_idx=None):
    """All H*W pixel centres (ray_idx None) or the selected flat indices: [N] shared by
    every image or [B,N] per image (renderer.py:277-291)."""
    B = len(pose_w2c)
    if ray_idx is None:
        ray_idx = torch.arange(H * W, device=pose_w2c.device)
    xy = pixel_centers(ray_idx, W, pose_w2c.dtype)
    if xy.dim() == 3 and xy.shape[0] != B:
        raise ValueError("per-image ray_idx must have one row per pose")
    return get_center_and_ray_at_pixels(pose_w2c, xy, intr)


def get_3D_points_from_depth(center, ray, depth, multi_samples=False):
    """camera.py:418-437 (kept for API completeness; the HIP kernel fuses it)."""
    if multi_samples:
        center, ray = center[:, :, None], ray[:, :, None]
    return center + ray * depth


# ---------------------------------------------------------------------------------------------- pose parameterisations
SERIES_TERMS = 11           # camera.py:180-205 taylor_A / _B / _C, nth = 10
_unfused = 0


@contextlib.contextmanager
def unfused():
    """Inside the block every function below takes its torch restatement, whatever its inputs: for a caller that needs a
    second derivative (the kernels' backward is once-differentiable) and for measuring the kernels against what an unmodified
    trainer runs (tools/pose_optim_bench.py --pose series)."""
    global _unfused
    _unfused += 1
    try:
        yield
    finally:
        _unfused -= 1


def _on_device(*tensors):
    return all(t.dtype == torch.float32 and t.device.type == "cuda" and t.layout == torch.strided for t in tensors)


def _takes_kernel(*tensors):
    """dense float32 tensors on the renderer's device; anything else (CPU, float64, `unfused()`) is torch's"""
    return not _unfused and _on_device(*tensors)


def _series(theta, k):
    """sum_{i=0}^{10} (-1)^i theta^(2i) / (2i + k)!  -- k = 1: sin(x)/x, 2: (1 - cos x)/x^2, 3: (x - sin x)/x^3, each TRUNCATED as
    the reference truncates it and accumulated term by term in its order, so that values at large theta are the polynomial's"""
    ans = torch.zeros_like(theta)
    for i in range(SERIES_TERMS):
        ans = ans + (-1) ** i * theta ** (2 * i) / float(math.factorial(2 * i + k))
    return ans


def skew_symmetric(w):
    w0, w1, w2 = w.unbind(dim=-1)
    O = torch.zeros_like(w0)
    return torch.stack([torch.stack([O, -w2, w1], dim=-1), torch.stack([w2, O, -w0], dim=-1), torch.stack([-w1, w0, O], dim=-1)], dim=-2)


def se3_to_SE3_torch(wu):
    """[...,6] (w, u) -> [...,3,4] = [R | V u] (camera.py:142-157)"""
    w, u = wu.split([3, 3], dim=-1)
    wx = skew_symmetric(w)
    theta = w.norm(dim=-1)[..., None, None]
    I = torch.eye(3, device=wu.device, dtype=wu.dtype)
    A, B, C = _series(theta, 1), _series(theta, 2), _series(theta, 3)
    wx2 = wx @ wx
    R = I + A * wx + B * wx2
    V = I + B * wx + C * wx2
    return torch.cat([R, V @ u[..., None]], dim=-1)


def compose_pair_torch(pose_a, pose_b):
    """pose_b o pose_a (camera.py:108-115)"""
    R_a, t_a = pose_a[..., :3], pose_a[..., 3:]
    R_b, t_b = pose_b[..., :3], pose_b[..., 3:]
    return torch.cat([R_b @ R_a, R_b @ t_a + t_b], dim=-1)


def r6d2mat_torch(d6):
    """[...,6] two first ROWS of a rotation -> [...,3,3] by Gram-Schmidt (two_columns.py:42-62)"""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.linalg.cross(b1, b2, dim=-1)), dim=-2)


def pose_from_d9_torch(d9, invert=False):
    pose = torch.cat([r6d2mat_torch(d9[..., 3:]), d9[..., :3, None]], dim=-1)
    return invert_pose(pose) if invert else pose


def refine_se3(xi, base):
    """camera.pose.compose([camera.lie.se3_to_SE3(xi), base]) folded into one launch per direction: xi [...,6], base [...,3,4]
    (or [1,3,4]) -> [...,3,4]"""
    if not _takes_kernel(xi, base):
        return compose_pair_torch(se3_to_SE3_torch(xi), base)
    lead = torch.broadcast_shapes(xi.shape[:-1], base.shape[:-2])
    pose, _ = ops.Se3Pose.apply(xi.expand(*lead, 6).reshape(-1, 6), base.expand(*lead, 3, 4).reshape(-1, 3, 4), False)
    return pose.reshape(*lead, 3, 4)


def r6d2mat(d6):
    if not _takes_kernel(d6):
        return r6d2mat_torch(d6)
    return ops.D9Pose.apply(F.pad(d6.reshape(-1, 6), (3, 0)), False)[..., :3].reshape(*d6.shape[:-1], 3, 3)


def pose_from_d9(d9, invert=False):
    """d9 [...,9] = (t, r1, r2) in pose_to_d9's order (two_columns.py:23-39) -> [r6d2mat(r1, r2) | t], inverted if asked"""
    if not _takes_kernel(d9):
        return pose_from_d9_torch(d9, invert)
    return ops.D9Pose.apply(d9.reshape(-1, 9), invert).reshape(*d9.shape[:-1], 3, 4)


class Lie:
    """camera.py's Lie, the part a pose optimisation runs every iteration"""

    def se3_to_SE3(self, wu):
        if not _takes_kernel(wu):
            return se3_to_SE3_torch(wu)
        return ops.Se3Pose.apply(wu.reshape(-1, 6), None, False)[0].reshape(*wu.shape[:-1], 3, 4)


class Pose:
    """camera.py's Pose: operations on [...,3,4] = [R | t]"""

    def invert(self, pose):
        return invert_pose(pose)

    def compose(self, pose_list):
        """pose_new(x) = poseN o ... o pose2 o pose1(x)"""
        pose_new = pose_list[0]
        for p in pose_list[1:]:
            pose_new = self.compose_pair_b_at_a(pose_a=pose_new, pose_b=p)
        return pose_new

    def compose_pair_b_at_a(self, pose_a, pose_b):
        if not _takes_kernel(pose_a, pose_b):
            return compose_pair_torch(pose_a, pose_b)
        # a single [1,3,4] operand is expanded to match [B,3,4] (what the trainer hands over at joint_pose_nerf_trainer.py:739)
        lead = torch.broadcast_shapes(pose_a.shape[:-2], pose_b.shape[:-2])
        a, b = (p.expand(*lead, 3, 4).reshape(-1, 3, 4) for p in (pose_a, pose_b))
        return ops.ComposePose.apply(a, b).reshape(*lead, 3, 4)


lie = Lie()
pose = Pose()

_installer = Patcher("sparf_amd.camera.install", "uninstall")


def install(camera_module, two_columns_module=None):
    """Opt-in: put the functions above under a trainer's own names -- `camera_module.lie.se3_to_SE3`,
    `camera_module.pose.compose_pair_b_at_a` (its `compose` goes through it) and, if given, `two_columns_module.r6d2mat` -- until
    `uninstall()`.  Nothing in this package calls it."""
    _installer.guard()
    targets = [(camera_module.lie, "se3_to_SE3", lie.se3_to_SE3), (camera_module.pose, "compose_pair_b_at_a", pose.compose_pair_b_at_a)]
    if two_columns_module is not None:
        targets.append((two_columns_module, "r6d2mat", r6d2mat))
    for obj, name, fn in targets:
        _installer.put(obj, name, fn)        # (a method lives on the class: the instance then goes back to having none of its own)


def uninstall():
    _installer.restore()
