"""Generate tests/golden/pose.npz: inputs, upstream gradients and the REFERENCE's own fp32 outputs and autograd gradients (CPU) for
the pose parameterisations (tests/test_pose_cpu.py, tests/test_pose_gpu.py; names and cases: tests/pose_referee.py).

Runs only where the reference is importable (as make_golden.py): the committed file holds arrays only.

  se3_<case>_<n>_{xi,base,g_pose,g_refine}   inputs; cases: xi exactly zero, Gaussian of scale 1e-7 / 0.05 / 1.5, |w| = 3.1
  ..._{refine,pose}                          lie.se3_to_SE3(xi), pose.compose([refine, base])
  ..._d_xi_a                                 d xi of  sum(refine * g_pose)                       (no base)
  ..._{d_xi_b,d_base_b}                      d xi, d base of  sum(pose * g_pose) + sum(refine * g_refine)
  cmp_<n>_{a,b,g,out,d_a,d_b}                pose.compose_pair_b_at_a(a, b)
  d9_<case>_<n>_{d9,g}                       cases: pose_to_d9 of rigid transforms + N(0, 0.1) ("init"), generic r1, r2
  ..._{pose0,pose1,d0,d1}                    [r6d2mat | t] and pose.invert of it; d d9 of sum(pose * g)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat"), "/root/reference"]

import source.utils.camera as camera                                    # noqa: E402  (the reference)
from source.models.poses_models.two_columns import pose_to_d9, r6d2mat   # noqa: E402
from tests.pose_referee import NS, XI_CASES, D9_CASES, FIXTURE          # noqa: E402


def rigid(rs, n):
    q, r = np.linalg.qr(rs.randn(n, 3, 3))
    q = q * np.sign(np.diagonal(r, axis1=-2, axis2=-1))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return torch.from_numpy(np.concatenate([q, rs.randn(n, 3, 1)], -1).astype(np.float32))


def xi_case(rs, case, n):
    if case == "zero":
        return torch.zeros(n, 6)
    if case == "w3.1":
        w = rs.randn(n, 3)
        w *= 3.1 / np.linalg.norm(w, axis=-1, keepdims=True)
        return torch.from_numpy(np.concatenate([w, rs.randn(n, 3)], -1).astype(np.float32))
    return torch.from_numpy((float(case[1:]) * rs.randn(n, 6)).astype(np.float32))


def d9_case(rs, case, n):
    if case == "init":
        return pose_to_d9(rigid(rs, n)) + torch.from_numpy((0.1 * rs.randn(n, 9)).astype(np.float32))
    out = []
    while len(out) < n:                 # |r1| >= 0.1 and at least 10 degrees between r1 and r2: the reference itself is well conditioned
        v = rs.randn(9)
        r1, r2 = v[3:6], v[6:]
        c = abs(r1 @ r2) / (np.linalg.norm(r1) * np.linalg.norm(r2))
        if np.linalg.norm(r1) >= 0.1 and np.linalg.norm(r2) >= 0.1 and c <= np.cos(np.deg2rad(10.0)):
            out.append(v)
    return torch.from_numpy(np.stack(out).astype(np.float32))


def grads(loss, *xs):
    return [g.numpy() for g in torch.autograd.grad(loss, xs)]


def main():
    rs = np.random.RandomState(20260)
    out = {}
    rnd = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    for n in NS:
        for case in XI_CASES:
            k = f"se3_{case}_{n}_"
            xi, base, g_pose, g_refine = xi_case(rs, case, n), rigid(rs, n), rnd(n, 3, 4), rnd(n, 3, 4)
            out.update({k + "xi": xi.numpy(), k + "base": base.numpy(), k + "g_pose": g_pose.numpy(), k + "g_refine": g_refine.numpy()})
            x, b = xi.clone().requires_grad_(), base.clone().requires_grad_()
            refine = camera.lie.se3_to_SE3(x)
            pose = camera.pose.compose([refine, b])
            out[k + "refine"], out[k + "pose"] = refine.detach().numpy(), pose.detach().numpy()
            out[k + "d_xi_a"], = grads((refine * g_pose).sum(), x)
            refine = camera.lie.se3_to_SE3(x)
            pose = camera.pose.compose([refine, b])
            out[k + "d_xi_b"], out[k + "d_base_b"] = grads((pose * g_pose).sum() + (refine * g_refine).sum(), x, b)
        k = f"cmp_{n}_"
        a, b, g = rigid(rs, n).requires_grad_(), rigid(rs, n).requires_grad_(), rnd(n, 3, 4)
        o = camera.pose.compose_pair_b_at_a(a, b)
        out.update({k + "a": a.detach().numpy(), k + "b": b.detach().numpy(), k + "g": g.numpy(), k + "out": o.detach().numpy()})
        out[k + "d_a"], out[k + "d_b"] = grads((o * g).sum(), a, b)
        for case in D9_CASES:
            k = f"d9_{case}_{n}_"
            d9, g = d9_case(rs, case, n), rnd(n, 3, 4)
            out.update({k + "d9": d9.numpy(), k + "g": g.numpy()})
            for inv in (0, 1):
                x = d9.clone().requires_grad_()
                p = torch.cat((r6d2mat(x[:, 3:])[:, :3, :3], x[:, :3, None]), -1)          # two_columns.py:177-178
                if inv:
                    p = camera.pose.invert(p)
                out[k + f"pose{inv}"] = p.detach().numpy()
                out[k + f"d{inv}"], = grads((p * g).sum(), x)
    for key, v in out.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), key
    np.savez_compressed(FIXTURE, **out)
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
