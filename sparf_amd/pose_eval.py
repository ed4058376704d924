"""Pose evaluation: what every joint pose-NeRF trainer of the reference runs to log its pose errors and to bring a test
pose into the optimised frame -- CommonPoseEvaluation.evaluate_any_poses with prealign_w2c_small_camera_systems and
evaluate_camera_alignment (source/training/joint_pose_nerf_trainer.py:160-311) and backtrack_from_aligning_the_trajectory
(source/utils/geometry/align_trajectories.py:94-101) -- as ONE library call each (csrc/pose_eval.hip), and a plain torch restatement of the
same lines, in this file, for everything the kernels do not take: CPU or float64 tensors, `unfused()`, more than 64 poses, fewer than two,
a similarity of type 'align_to_first'.

`evaluate_poses` and `backtrack` return device tensors and read nothing back.  `install()` puts the three methods on a trainer's pose
evaluation class and the backtrack under the reference's name on the modules that imported it.  Nothing in this package calls install();
there is no `opt.hip` key.  Not covered: prealign_w2c_large_camera_systems (Procrustes, B > 10), the ATE path, the align-to-first
backtrack, gradients (the reference runs all of it under no_grad).
"""
import contextlib
import ctypes

import numpy as np
import torch

from . import lib as L
from .camera import invert_pose
from .edict import EasyDict as edict
from .patcher import Patcher

MAX_POSES = L.POSE_EVAL_MAX_POSES        # of one set, in the kernel
MAX_VIEWS = 10                           # joint_pose_nerf_trainer.py:233: the pairs of the first min(B, 10) views
MAX_PAIRS = L.POSE_EVAL_MAX_PAIRS
STATS = ("error_R_before_align", "error_t_before_align", "error_R", "error_t")      # joint_pose_nerf_trainer.py:299-311
_unfused = 0


@contextlib.contextmanager
def unfused():
    """Inside the block everything below takes its torch restatement, whatever its inputs (tools/pose_eval_bench.py --leg series)."""
    global _unfused
    _unfused += 1
    try:
        yield
    finally:
        _unfused -= 1


def n_pairs(B):
    n = min(B, MAX_VIEWS)
    return n * (n - 1)


def pair_of(p, B):
    """candidate p -> (a, b) in the reference's order (:233-236)"""
    n = min(B, MAX_VIEWS)
    a, r = divmod(p, n - 1)
    return a, r + (r >= a)


# ---------------------------------------------------------------------------------------------- the torch restatement
def _pad(p):
    """camera.py:24-29 pad_poses"""
    bottom = torch.broadcast_to(torch.tensor([0, 0, 0, 1.0], device=p.device, dtype=p.dtype), p[..., :1, :4].shape)
    return torch.cat((p[..., :3, :4], bottom), dim=-2)


def _inverse_4x4(mat):
    """camera.py:37-59 pose_inverse_4x4 in its transpose form, [B,4,4] or [4,4]"""
    out = torch.zeros_like(mat)
    out[..., 3, 3] = 1
    R, t = mat[..., :3, :3], mat[..., :3, 3:]
    R_inv = R.transpose(-1, -2)
    out[..., :3, :] = torch.cat([R_inv, -R_inv @ t], dim=-1)
    return out


def rotation_distance_torch(R1, R2, eps=1e-7):
    """camera.py:466-471"""
    R_diff = R1 @ R2.transpose(-2, -1)
    trace = R_diff[..., 0, 0] + R_diff[..., 1, 1] + R_diff[..., 2, 2]
    return ((trace - 1) / 2).clamp(-1 + eps, 1 - eps).acos_()


def camera_alignment_errors_torch(pose_aligned_w2c, pose_GT_w2c):
    """joint_pose_nerf_trainer.py:257-287 evaluate_camera_alignment -> edict(R [B] in radians, t [B]), not averaged"""
    R_a, t_a = invert_pose(pose_aligned_w2c).split([3, 1], dim=-1)
    R_g, t_g = invert_pose(pose_GT_w2c).split([3, 1], dim=-1)
    return edict(R=rotation_distance_torch(R_a, R_g), t=(t_a.reshape(-1, 3) - t_g.reshape(-1, 3)).norm(dim=-1))


def _alignment_function(from_padded, to_padded, idx_a, idx_b):
    """:173-213"""
    from_padded = from_padded.clone()
    dist_from = torch.norm(from_padded[idx_a, :3, 3] - from_padded[idx_b, :3, 3])
    dist_to = torch.norm(to_padded[idx_a, :3, 3] - to_padded[idx_b, :3, 3])
    scale = dist_to / dist_from
    from_padded[:, :3, 3] = from_padded[:, :3, 3] * scale
    transformation = to_padded[idx_a] @ _inverse_4x4(from_padded[idx_a])
    aligned_w2c = _inverse_4x4(transformation[None] @ from_padded)
    sim3 = edict(R=transformation[:3, :3].unsqueeze(0), type='traj_align', t=transformation[:3, 3].reshape(1, 3, 1), s=scale)
    return aligned_w2c[:, :3], sim3


def align_pairwise_torch(pose_w2c, pose_GT_w2c, with_scores=False):
    """:215-254 prealign_w2c_small_camera_systems without its fixed-pose branch: the literal loop over every ordered pair of the first
    min(B, 10) views with its four readbacks per candidate -> (pose_aligned_w2c [B,3,4], ssim_est_gt_c2w); with_scores: also the index
    and the list of (R in degrees, t, their product) per candidate"""
    pose_c2w, pose_GT_c2w = invert_pose(pose_w2c), invert_pose(pose_GT_w2c)
    B = pose_c2w.shape[0]
    aligned_list, sim3_list, scores = [], [], []
    for a in range(min(B, MAX_VIEWS)):
        for b in range(min(B, MAX_VIEWS)):
            if a == b:
                continue
            aligned, sim3 = _alignment_function(_pad(pose_c2w), _pad(pose_GT_c2w), a, b)
            aligned_list.append(aligned)
            sim3_list.append(sim3)
            error = camera_alignment_errors_torch(aligned, pose_GT_w2c)
            scores.append((error.R.mean().item() * 180. / np.pi, error.t.mean().item(), error.t.mean().item() * (error.R.mean().item() * 180. / np.pi)))
    best = int(np.argmin([s[2] for s in scores]))
    if with_scores:
        return aligned_list[best], sim3_list[best], best, scores
    return aligned_list[best], sim3_list[best]


def _identity_sim3(device, dtype=torch.float32):
    """:221-222; the kernel's form: a 0-dim s"""
    return edict(R=torch.eye(3, device=device, dtype=dtype).unsqueeze(0), t=torch.zeros(1, 3, 1, device=device, dtype=dtype), s=1.)


def evaluate_poses_torch(pose_w2c, pose_gt_w2c, align=True):
    """The torch restatement of evaluate_poses: the reference's lines in the reference's order, set by set, in the operands' own dtype
    -> the same edict (stats, errors, aligned, best, scores, sim3 with `packed`)."""
    single = pose_w2c.dim() == 3
    pose = pose_w2c[None] if single else pose_w2c
    gt = pose_gt_w2c[None] if pose_gt_w2c.dim() == 3 else pose_gt_w2c
    S, B = pose.shape[:2]
    dev, dt = pose.device, pose.dtype
    P = n_pairs(B) if align else 0
    out = dict(stats=[], errors=[], aligned=[], best=[], scores=[], packed=[])
    for s in range(S):
        p, g = pose[s].detach(), gt[s if gt.shape[0] > 1 else 0]
        before = camera_alignment_errors_torch(p, g)
        if align:
            aligned, sim3, best, scores = align_pairwise_torch(p, g, with_scores=True)
        else:
            aligned, sim3, best, scores = p, _identity_sim3(dev, dt), -1, []
        after = camera_alignment_errors_torch(aligned, g)
        out["stats"].append(torch.stack([before.R.mean() * 180. / np.pi, before.t.mean(), after.R.mean() * 180. / np.pi, after.t.mean()]))
        out["errors"].append(torch.stack([torch.stack([before.R, before.t], dim=-1), torch.stack([after.R, after.t], dim=-1)]))
        out["aligned"].append(aligned)
        out["best"].append(best)
        out["scores"].append(torch.tensor(scores, device=dev, dtype=dt).reshape(P, 3))
        out["packed"].append(torch.cat([sim3.R.reshape(9), sim3.t.reshape(3), torch.as_tensor(sim3.s, device=dev, dtype=dt).reshape(1)]))
    return _result(torch.stack(out["stats"]), torch.stack(out["errors"]), torch.stack(out["aligned"]),
                   torch.tensor(out["best"], device=dev, dtype=torch.int32), torch.stack(out["scores"]), torch.stack(out["packed"]), single)


def backtrack_torch(pose_GT_w2c, ssim_est_gt_c2w):
    """align_trajectories.py:94-101"""
    pose_GT_c2w = invert_pose(pose_GT_w2c)
    R_aligned = ssim_est_gt_c2w.R.transpose(-2, -1) @ pose_GT_c2w[:, :3, :3]
    t_aligned = ssim_est_gt_c2w.R.transpose(-2, -1) / ssim_est_gt_c2w.s @ (pose_GT_c2w[:, :3, 3:4] - ssim_est_gt_c2w.t)
    return invert_pose(torch.cat([R_aligned, t_aligned.reshape(-1, 3, 1)], dim=-1))


# ---------------------------------------------------------------------------------------------- the public functions
def sim3_of(packed):
    """13 floats (R rows, t, s) [13] or [S,13] -> the reference's ssim_est_gt_c2w (:210-211) as views of them: R [1,3,3], t [1,3,1], s
    0-dim ([S,...] / [S] for sets), type 'traj_align'; `packed` is the vector itself"""
    lead = packed.shape[:-1]
    return edict(R=packed[..., :9].reshape(*lead, 1, 3, 3), t=packed[..., 9:12].reshape(*lead, 1, 3, 1), s=packed[..., 12], type='traj_align',
                 packed=packed)


def _result(stats, errors, aligned, best, scores, packed, single):
    if single:
        stats, errors, aligned, best, scores, packed = stats[0], errors[0], aligned[0], best[0], scores[0], packed[0]
    return edict(stats=stats, errors=errors, aligned=aligned, best=best, scores=scores, sim3=sim3_of(packed))


def _on_device(*tensors):
    return all(t.dtype == torch.float32 and t.device.type == "cuda" and t.layout == torch.strided for t in tensors)


def _takes_kernel(*tensors):
    """float32 tensors on the GPU; anything else (CPU, float64, `unfused()`) is the restatement's"""
    return not _unfused and _on_device(*tensors)


def evaluate_poses(pose_w2c, pose_gt_w2c, align=True):
    """Rotation and camera-centre errors of estimated world-to-camera poses against the ground truth, before and after the similarity
    that the reference's pairwise search finds (evaluate_any_poses, :290-311, for B <= 10; the same search over the first 10 views above
    that): pose_w2c [B,3,4] or [S,B,3,4] for S independent sets, pose_gt_w2c [B,3,4] (shared by the sets) or [S,B,3,4].
    align=False: no search -- the reference's n_first_fixed_poses > 1 branch, or a bare evaluate_camera_alignment.
    -> edict of device tensors ([S,...] in front for sets): stats [4] = error_R_before_align (degrees), error_t_before_align, error_R
    (degrees), error_t; errors [2,B,2] = before / after x (R in radians, t) per pose; aligned [B,3,4]; best int32 (-1 without the
    search); scores [P,3] = (R in degrees, t, product) per candidate, P = n (n - 1), n = min(B, 10); sim3 = edict(R [1,3,3], t [1,3,1],
    s 0-dim, type 'traj_align', packed [13]), views of one vector.  One kernel call, no readback."""
    if pose_w2c.dim() not in (3, 4) or pose_w2c.shape[-2:] != (3, 4) or pose_gt_w2c.shape[-3:] != pose_w2c.shape[-3:]:
        raise ValueError(f"pose evaluation: poses must be [B,3,4] or [S,B,3,4] and the ground truth [B,3,4] of the same B, got {list(pose_w2c.shape)} and "
                         f"{list(pose_gt_w2c.shape)}")
    single = pose_w2c.dim() == 3
    S, B = (1, pose_w2c.shape[0]) if single else pose_w2c.shape[:2]
    gt_sets = 1 if pose_gt_w2c.dim() == 3 else pose_gt_w2c.shape[0]
    if gt_sets not in (1, S):
        raise ValueError(f"pose evaluation: {gt_sets} ground-truth sets for {S} pose sets")
    if not _takes_kernel(pose_w2c, pose_gt_w2c) or B > MAX_POSES or B < (2 if align else 1) or S == 0:
        return evaluate_poses_torch(pose_w2c, pose_gt_w2c, align)
    dev = pose_w2c.device
    L.require_gpu(dev)
    pose, gt = pose_w2c.detach().contiguous(), pose_gt_w2c.detach().contiguous()
    new = lambda *shape, dtype=torch.float32: torch.empty(*shape, device=dev, dtype=dtype)
    stats, errors, aligned, packed, best = new(S, 4), new(S, 2, B, 2), new(S, B, 3, 4), new(S, L.POSE_EVAL_SIM3), new(S, dtype=torch.int32)
    scores = new(S, MAX_PAIRS, 3)
    a = L.PoseEval(pose=pose.data_ptr(), pose_gt=gt.data_ptr(), gt_sets=gt_sets, S=S, B=B, flags=L.POSE_EVAL_ALIGN if align else 0,
                   stats=stats.data_ptr(), errors=errors.data_ptr(), aligned=aligned.data_ptr(), sim3=packed.data_ptr(), best=best.data_ptr(),
                   scores=scores.data_ptr())
    L.call("sparf_pose_eval", dev, ctypes.byref(a))
    return _result(stats, errors, aligned, best, scores[:, :n_pairs(B) if align else 0], packed, single)


def pack_sim3(sim3, device, dtype=torch.float32):
    """ssim_est_gt_c2w -> 13 floats on `device`: its `packed` if it has one, otherwise R, t and s (a tensor or, from the large-system
    path, a Python float)"""
    if sim3.get("packed") is not None and sim3.packed.dim() == 1:
        return sim3.packed.to(device=device, dtype=dtype)        # (as it is where it already lies there: no copy)
    return torch.cat([sim3.R.reshape(9).to(device=device, dtype=dtype), sim3.t.reshape(3).to(device=device, dtype=dtype),
                      torch.as_tensor(sim3.s, device=device, dtype=dtype).reshape(1)])


_installer = Patcher("sparf_amd.pose_eval.install", "uninstall")     # keeps the trainer's own methods and function: what the kernels do not take goes to them


def backtrack(pose_gt_w2c, sim3):
    """backtrack_from_aligning_the_trajectory (align_trajectories.py:94-101): ground-truth world-to-camera poses [N,3,4] into the frame of
    the estimated poses, under the similarity `sim3` that evaluate_poses (or a prealign method) returned -> [N,3,4].  One kernel call."""
    kernel = _takes_kernel(pose_gt_w2c) and pose_gt_w2c.dim() == 3 and pose_gt_w2c.shape[-2:] == (3, 4) and sim3.get("type") != 'align_to_first' and \
        sim3.R.numel() == 9
    if not kernel:
        return _original_method(BACKTRACK, backtrack_torch)(pose_gt_w2c, sim3)
    dev = pose_gt_w2c.device
    L.require_gpu(dev)
    packed = pack_sim3(sim3, dev).detach().contiguous()
    gt = pose_gt_w2c.detach().contiguous()
    out = torch.empty_like(gt)
    L.call("sparf_pose_backtrack", dev, L.ptr(gt), gt.shape[0], L.ptr(packed), 0, L.ptr(out))
    return out


# ---------------------------------------------------------------------------------------------- under the reference's names
def _fixed_first_poses(self):
    return self.settings.camera.n_first_fixed_poses > 1


def evaluate_camera_alignment(self, opt, pose_aligned_w2c, pose_GT_w2c):
    """:257-287 under its own signature -> edict(R [B] in radians, t [B])"""
    if not _takes_kernel(pose_aligned_w2c, pose_GT_w2c) or not 1 <= pose_aligned_w2c.shape[0] <= MAX_POSES:
        return _original_method("evaluate_camera_alignment", lambda self, opt, a, b: camera_alignment_errors_torch(a, b))(self, opt, pose_aligned_w2c, pose_GT_w2c)
    res = evaluate_poses(pose_aligned_w2c, pose_GT_w2c, align=False)
    return edict(R=res.errors[0, :, 0], t=res.errors[0, :, 1])


def prealign_w2c_small_camera_systems(self, opt, pose_w2c, pose_GT_w2c):
    """:160-254 under its own signature -> (pose_aligned_w2c, ssim_est_gt_c2w); the similarity also carries `packed`"""
    if not _takes_kernel(pose_w2c, pose_GT_w2c) or not 2 <= pose_w2c.shape[0] <= MAX_POSES:
        return _original_method("prealign_w2c_small_camera_systems", _prealign_torch)(self, opt, pose_w2c, pose_GT_w2c)
    if _fixed_first_poses(self):
        return pose_w2c, _identity_sim3(self.device)             # (:221-223: no `type`, a Python float s, the poses themselves; no launch)
    res = evaluate_poses(pose_w2c, pose_GT_w2c)
    return res.aligned, res.sim3


def _prealign_torch(self, opt, pose_w2c, pose_GT_w2c):
    if _fixed_first_poses(self):
        return pose_w2c, _identity_sim3(self.device)
    return align_pairwise_torch(pose_w2c, pose_GT_w2c)


def evaluate_any_poses(self, opt, pose_w2c, pose_GT_w2c):
    """:290-311 under its own signature -> dict of four 0-dim tensors.  B <= 10: one launch; above, the original method (its Procrustes
    path is not covered)"""
    B = pose_w2c.shape[0]
    if not _takes_kernel(pose_w2c, pose_GT_w2c) or not 2 <= B <= MAX_VIEWS:
        return _original_method("evaluate_any_poses", _evaluate_any_poses_torch)(self, opt, pose_w2c, pose_GT_w2c)
    res = evaluate_poses(pose_w2c, pose_GT_w2c, align=not _fixed_first_poses(self))
    return {key: res.stats[i] for i, key in enumerate(STATS)}


def _evaluate_any_poses_torch(self, opt, pose_w2c, pose_GT_w2c):
    if pose_w2c.shape[0] > MAX_VIEWS:
        raise RuntimeError("sparf_amd.pose_eval.evaluate_any_poses: more than 10 poses go to the trainer's own method "
                           "(prealign_w2c_large_camera_systems) and there is none (install() saves it)")
    error = camera_alignment_errors_torch(pose_w2c.detach(), pose_GT_w2c)
    stats = {STATS[0]: error.R.mean() * 180. / np.pi, STATS[1]: error.t.mean()}
    aligned, _ = _prealign_torch(self, opt, pose_w2c.detach(), pose_GT_w2c)
    error = camera_alignment_errors_torch(aligned, pose_GT_w2c)
    stats.update({STATS[2]: error.R.mean() * 180. / np.pi, STATS[3]: error.t.mean()})
    return stats


def _original_method(name, restatement):
    """the trainer's own method where install() saved one -- not inside unfused(), which asks for this file's restatement"""
    return restatement if _unfused else _installer.original(name) or restatement


METHODS = ("evaluate_camera_alignment", "prealign_w2c_small_camera_systems", "evaluate_any_poses")
BACKTRACK = "backtrack_from_aligning_the_trajectory"


def install(pose_evaluation_class, *importing_modules):
    """Opt-in: put evaluate_camera_alignment, prealign_w2c_small_camera_systems and evaluate_any_poses above on `pose_evaluation_class`
    (CommonPoseEvaluation of source.training.joint_pose_nerf_trainer; its subclasses inherit them) and `backtrack` under the name
    backtrack_from_aligning_the_trajectory on every module given that has it (align_trajectories itself, and joint_pose_nerf_trainer,
    which imported it by name), until `uninstall()`.  Nothing in this package calls it."""
    _installer.guard()
    ours = dict(evaluate_camera_alignment=evaluate_camera_alignment, prealign_w2c_small_camera_systems=prealign_w2c_small_camera_systems,
                evaluate_any_poses=evaluate_any_poses)
    for name in METHODS:
        if hasattr(pose_evaluation_class, name):
            _installer.save(name, getattr(pose_evaluation_class, name))        # (inherited ones too)
        _installer.put(pose_evaluation_class, name, ours[name])
    for mod in importing_modules:
        if BACKTRACK in vars(mod):
            _installer.save(BACKTRACK, vars(mod)[BACKTRACK])                 # (the first one met stays)
            _installer.put(mod, BACKTRACK, backtrack)


def uninstall():
    _installer.restore()
