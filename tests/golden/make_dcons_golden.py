"""Generate tests/golden/dcons.npz: inputs and the REFERENCE's own fp32 results (CPU) for the depth-consistency kernels
(tests/test_dcons_cpu.py, tests/test_dcons_gpu.py; names, sizes and cases: tests/dcons_referee.py).

Runs only where the reference is importable (through tests/ref_harness.install_reference()): the committed file holds arrays only.
The projection results come from the reference's unmodified batch_backproject_to_3d and batch_project and the mask lines of
depth_cons_loss.py:252-254, the loss results from BaseLoss.compute_diff_loss in the call order of :293-312, the gradients from autograd
on them.

Scene, as in make_reproj_golden.py: a 378x504 image, the general K (unequal focal lengths, a skew, a shifted principal point) for both
views; a reference pose; the unseen pose = the reference's pose_inverse_4x4 of a blend of two c2w poses (weight 0.37), so its rotation
block is not orthonormal; integer pixels, depths in [0.8, 5], depth_min 1.2; rendered depths = the projected depth + N(0, 0.8)
(differences on both sides of |e| = 1), the fine ones + N(0, 0.6).

Margins are a CONDITION: a point whose float64 projection lies within 0.01 px of one of the four image bounds or whose depth lies
within 1e-4 of depth_min is redrawn (at most 1 % of every size's points), the visibilities keep 7e-4 from the threshold by
construction, and the reference's fp32 mask must equal the float64 one on every case: every size and every mask pattern
(dcons_referee.PATTERNS, rows of the first PATTERN_BASES points rearranged), each of which is a run of the reference of its own.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat")]

from tests import ref_harness                                           # noqa: E402
from tests import dcons_referee as R                                    # noqa: E402
from tests.golden.make_reproj_golden import K_GENERAL, P_SELF, T_REL, H, W, f32      # noqa: E402  (the scene constants; importing it installs the reference)

assert ref_harness.install_reference(), "the reference tree is not importable"
from source.training.core.base_losses import BaseLoss                   # noqa: E402
from source.utils.camera import pose_inverse_4x4                        # noqa: E402
from source.utils.geometry.batched_geometry_utils import batch_backproject_to_3d, batch_project      # noqa: E402

DEPTH_MIN, BLEND = 1.2, 0.37


def draw(rs, n):
    return np.stack([rs.randint(0, W, n), rs.randint(0, H, n)], 1).astype(np.float32), rs.uniform(0.8, 5.0, n).astype(np.float32)


def main():
    rs = np.random.RandomState(20262)
    N = R.NS[-1]
    K = K_GENERAL.astype(np.float32)
    P_ref = torch.tensor(P_SELF)
    c2w_ref, c2w_other = pose_inverse_4x4(P_ref), pose_inverse_4x4(torch.tensor(T_REL @ P_SELF))
    T_c2w = c2w_ref.numpy().astype(np.float32)
    P_unseen = pose_inverse_4x4(BLEND * c2w_ref + (1 - BLEND) * c2w_other).numpy().astype(np.float32)
    fx = dict(K=K, T_c2w=T_c2w, P_unseen=P_unseen, HW=np.array([H, W], dtype=np.int32), depth_min=np.float32(DEPTH_MIN))
    px, d = draw(rs, N)
    redrawn = np.zeros(N, dtype=bool)
    for _ in range(100):
        uv64, z64 = R.project(R.world(px, d, K, T_c2w), P_unseen, K)
        bad = R.near_margin(uv64, z64, H, W, fx["depth_min"])
        if not bad.any():
            break
        redrawn |= bad
        px[bad], d[bad] = draw(rs, int(bad.sum()))
    else:
        raise RuntimeError("margins not met")
    for n in R.NS:
        assert redrawn[:n].sum() <= 0.01 * n, (n, int(redrawn[:n].sum()))
    assert (np.abs(R.vis(N).astype(np.float64) - R.VIS_THRESH) > 1e-4).all()
    mask64 = R.inside(uv64, z64, H, W, fx["depth_min"])

    # the reference's chain in fp32 at every size (a matrix product of another size may round differently), back-projecting form, and
    # its gradient to the depth; the largest run also provides the inputs of the select and loss cases
    guv, gz, dmin = f32(R.g_uv(N)), f32(R.g_z(N)), f32(fx["depth_min"])

    def inside(uv, z):
        return uv[:, 0].ge(0.) & uv[:, 1].ge(0.) & uv[:, 0].le(W - 1) & uv[:, 1].le(H - 1) & z.ge(dmin)
    def reference_run(rows):
        """the reference's unmodified chain on the given rows of the scene -> (uv, z, d depth) as numpy; its mask must be the float64 one"""
        n = len(rows)
        dt = f32(d[rows]).requires_grad_()
        pts = batch_backproject_to_3d(kpi=f32(px[rows]), di=dt, Ki=f32(K), T_itoj=f32(T_c2w))
        uv, z = batch_project(pts, T_itoj=f32(P_unseen), Kj=f32(K), return_depth=True)
        valid = inside(uv, z)
        assert np.array_equal(valid.numpy(), mask64[rows]), "the reference's fp32 mask differs from the float64 one"
        d_d = torch.zeros(n)
        if valid.any():
            d_d, = torch.autograd.grad((uv[valid] * guv[:n][valid]).sum() + (z[valid] * gz[:n][valid]).sum(), dt)
        return uv.detach().numpy(), z.detach().numpy(), d_d.numpy()
    for n in R.NS:
        sfx = "" if n == N else f"_{n}"
        fx["uv" + sfx], fx["z" + sfx], fx["d_d" + sfx] = reference_run(np.arange(n))
    # the mask patterns: the rows of the first `base` points rearranged, each through a run of the reference of its own
    for base in R.PATTERN_BASES:
        counts = {}
        for pattern in R.PATTERNS[1:]:
            rows = R.pattern_rows(mask64[:base], pattern)
            counts[pattern] = int(mask64[rows].sum())
            assert counts[pattern] == dict(all=len(rows), none=0, first=1, last=1, alternating=len(rows) // 2)[pattern] and len(rows) > 0
            fx[f"uv_{pattern}_{base}"], fx[f"z_{pattern}_{base}"], fx[f"d_d_{pattern}_{base}"] = reference_run(rows)
        print("patterns of", base, counts)
    assert int(mask64[:R.PATTERN_BASES[-1]].sum()) > 4096          # `all` of the larger base takes the counts launch
    assert 0.6 < mask64.mean() < 0.95
    z32 = fx["z"]
    dr = (z32 + 0.8 * rs.standard_normal(N)).astype(np.float32)
    drf = (z32 + 0.6 * rs.standard_normal(N)).astype(np.float32)
    fx.update(px=px, d=d, dr=dr, drf=drf, valid=mask64)

    # the points form on the float32 of the referee's world points
    Xw = R.world(px[:R.POINTS_NS[-1]], d[:R.POINTS_NS[-1]], K, T_c2w).astype(np.float32)
    fx["Xw"] = Xw
    for n in R.POINTS_NS:
        Xt = f32(Xw[:n]).requires_grad_()
        uv_p, z_p = batch_project(Xt, T_itoj=f32(P_unseen), Kj=f32(K), return_depth=True)
        valid_p = inside(uv_p, z_p)
        assert np.array_equal(valid_p.numpy(), R.project_want(fx, n, Xw=Xw[:n])["mask"]) and np.array_equal(valid_p.numpy(), mask64[:n])
        d_Xw = torch.zeros(n, 3)
        if valid_p.any():
            d_Xw, = torch.autograd.grad((uv_p[valid_p] * guv[:n][valid_p]).sum() + (z_p[valid_p] * gz[:n][valid_p]).sum(), Xt)
        fx.update({f"uv_p_{n}": uv_p.detach().numpy(), f"z_p_{n}": z_p.detach().numpy(), f"d_Xw_{n}": d_Xw.numpy()})

    # depth_cons_loss.py:293-312 on the first n points
    for n in R.NS:
        for case, (loss_type, fine) in R.LOSS_CASES.items():
            zp, v, dep, op, depf, opf = (f32(a) if a is not None else None for a in R.loss_inputs(fx, n, fine))
            zp.requires_grad_(), dep.requires_grad_()
            vis_ = v[:, None]
            w = vis_ * op[:, None]
            loss = BaseLoss.compute_diff_loss(None, loss_type, diff=zp.view(-1) - dep.view(-1), weights=w.view(-1))
            leaves = [zp, dep]
            if fine:
                depf.requires_grad_()
                w = vis_ * opf[:, None]
                loss = loss + BaseLoss.compute_diff_loss(None, loss_type, diff=zp.view(-1) - depf.view(-1), weights=w.view(-1))
                leaves.append(depf)
            avg = w.sum() / (w.nelement() + 1e-6)
            fx[f"loss_{case}_{n}"] = np.array([loss.item(), avg.item()], dtype=np.float32)
            if n in R.SEED_NS:
                fx[f"seeds_{case}_{n}"] = np.stack([g.numpy() for g in torch.autograd.grad(loss, leaves)])
    for key, v in fx.items():
        assert v.dtype in (np.float32, np.bool_, np.int32) and np.isfinite(v).all(), key
    np.savez_compressed(R.FIXTURE, **fx)
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes,", len(fx), "arrays")
    print("redrawn", int(redrawn.sum()), "of", N, "; valid share", mask64.mean(), "; kept by visibility", (R.vis(N) >= np.float32(R.VIS_THRESH)).mean())
    print("reference fp32 to float64: uv", np.abs(fx["uv"] - uv64).max(), "px, z", np.abs(fx["z"] - z64).max())


if __name__ == "__main__":
    main()
