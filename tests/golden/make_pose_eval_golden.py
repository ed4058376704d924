"""Generate tests/golden/pose_eval.npz: seeded fp32 pose sets and the REFERENCE's own fp32 results (CPU) on them, for the pose-evaluation
kernels (tests/test_pose_eval_cpu.py, tests/test_pose_eval_gpu.py; cases and the float64 referee: tests/pose_eval_referee.py).

Runs only where the reference is importable (through tests/ref_harness.install_reference()): the committed file holds arrays only.
source.training.joint_pose_nerf_trainer does not import without tensorboard, so -- as tests/ref_harness.joint_graph_class does for the
Graph subclass -- the text of `class CommonPoseEvaluation` is taken from the reference file at run time and executed in a namespace
holding what it names; the object is built with __new__ and given `settings.camera.n_first_fixed_poses` and `device`.  The values come
from its UNMODIFIED evaluate_any_poses, prealign_w2c_small_camera_systems and evaluate_camera_alignment and from
backtrack_from_aligning_the_trajectory.  The method keeps its per-candidate triples in local lists, so they are formed here from the
reference's own pad_poses, pose_inverse_4x4 and evaluate_camera_alignment in the method's order (joint_pose_nerf_trainer.py:185-209,
:244-247); that the method's own choice is the first minimum of that list is asserted on its returned scale.

Stored per case: the inputs; the reference's stats, aligned poses, similarity, index, triples and backtracked poses; the reference's
distance from the float64 referee for each of them, in the fp32 spacings of tests/pose_eval_referee.py; `decisive` -- the relative gap
between the referee's two smallest scores is at least 10 x the reference's measured relative distance from float64 on those two scores;
`roundtrip` -- the referee's own figure for backtrack(gt, similarity) against the estimated poses, in spacings.

Asserted here: every case with noise >= 0.05 is decisive (seeds are drawn until it is); in every non-degenerate case the referee's own
relative gap is >= 1e-6; the reference's index equals the referee's wherever decisive; the NaN pattern of the degenerate cases.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat")]

from tests import ref_harness                                           # noqa: E402
from tests import pose_eval_referee as R                                # noqa: E402

assert ref_harness.install_reference(), "the reference tree is not importable"
from easydict import EasyDict as edict                                  # noqa: E402
import source.utils.camera as camera                                    # noqa: E402
import source.utils.geometry.align_trajectories as align_trajectories   # noqa: E402


def pose_evaluation(n_first_fixed_poses):
    import typing
    from oracle.stage_reference import read_text
    src = read_text("source/training/joint_pose_nerf_trainer.py")
    body = src[src.index("class CommonPoseEvaluation"):src.index("class PoseAndNerfTrainerPerScene")]
    ns = dict(camera=camera, torch=torch, np=np, edict=edict, **{k: getattr(typing, k) for k in ("Any", "Dict", "List", "Tuple", "Union", "Optional", "Callable")})
    ns.update({k: v for k, v in vars(align_trajectories).items() if not k.startswith("_")})
    exec(body, ns)
    obj = ns["CommonPoseEvaluation"].__new__(ns["CommonPoseEvaluation"])
    obj.settings = edict(camera=edict(n_first_fixed_poses=n_first_fixed_poses))
    obj.device = torch.device("cpu")
    return obj


# ---- the inputs
def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def w2c_of(R_c2w, c):
    return np.concatenate([np.swapaxes(R_c2w, -1, -2), -(np.swapaxes(R_c2w, -1, -2) @ c[..., None])], axis=-1)


def make_inputs(c, seed):
    rs = np.random.RandomState(seed)
    S, B, G = c["S"], c["B"], c["gt_sets"]
    gt_R = np.stack([[rodrigues(rs.standard_normal(3)) for _ in range(B)] for _ in range(G)])
    gt_c = 2.0 * rs.standard_normal((G, B, 3))
    pose = np.zeros((S, B, 3, 4))
    for s in range(S):
        g = s if G > 1 else 0
        Rs, ts, sc = rodrigues(rs.standard_normal(3)), rs.standard_normal(3), np.exp(rs.uniform(-0.7, 0.7))
        for i in range(B):
            Rn = gt_R[g, i] @ rodrigues(c["noise"] * rs.standard_normal(3))
            cn = gt_c[g, i] + c["noise"] * rs.standard_normal(3)
            if c["kind"] == "pi" and i == 1:
                Rn = Rn @ rodrigues(np.pi * np.array([0.6, 0.0, 0.8]))
            pose[s, i] = w2c_of(Rs.T @ Rn, Rs.T @ (cn - ts) / sc)
        if c["kind"] == "coincident":
            pose[s, 1] = pose[s, 0]
        if c["kind"] == "identity":
            pose[s] = np.eye(3, 4)
    return pose.astype(np.float32), w2c_of(gt_R, gt_c).astype(np.float32)


# ---- the reference
def reference_run(c, pose, gt):
    ev = pose_evaluation(1 if c["align"] else 2)
    out = dict(stats=[], aligned=[], sim3=[], best=[], scores=[], back=[])
    for s in range(pose.shape[0]):
        p, g = torch.from_numpy(pose[s]), torch.from_numpy(gt[s if gt.shape[0] > 1 else 0])
        st = ev.evaluate_any_poses(None, p, g)
        assert list(st) == ["error_R_before_align", "error_t_before_align", "error_R", "error_t"]
        aligned, sim3 = ev.prealign_w2c_small_camera_systems(None, p, g)
        scores = []
        if c["align"]:
            B = p.shape[0]
            assert sim3.type == 'traj_align'
            # the candidates again, through the reference's own functions: what :238-247 appends for each
            for a in range(min(B, 10)):
                for b in range(min(B, 10)):
                    if a == b:
                        continue
                    c2w, gt_c2w = camera.pad_poses(camera.pose.invert(p)).clone(), camera.pad_poses(camera.pose.invert(g))
                    scale = torch.norm(gt_c2w[a, :3, 3] - gt_c2w[b, :3, 3]) / torch.norm(c2w[a, :3, 3] - c2w[b, :3, 3])
                    c2w[:, :3, 3] = c2w[:, :3, 3] * scale
                    T = gt_c2w[a] @ camera.pose_inverse_4x4(c2w[a])
                    err = ev.evaluate_camera_alignment(None, camera.pose_inverse_4x4(T[None] @ c2w)[:, :3], g)
                    scores.append((err.R.mean().item() * 180. / np.pi, err.t.mean().item(), err.t.mean().item() * (err.R.mean().item() * 180. / np.pi)))
            best = int(np.argmin([v[2] for v in scores]))
            a, b = R.pair_of(best, B)
            # the method's own choice is the candidate this list puts first: its similarity and poses, bit for bit (NaN compares by place)
            c2w, gt_c2w = camera.pad_poses(camera.pose.invert(p)).clone(), camera.pad_poses(camera.pose.invert(g))
            scale = torch.norm(gt_c2w[a, :3, 3] - gt_c2w[b, :3, 3]) / torch.norm(c2w[a, :3, 3] - c2w[b, :3, 3])
            assert np.array_equal(np.float32(scale), np.float32(sim3.s), equal_nan=True), (best, scale, sim3.s)
            back = align_trajectories.backtrack_from_aligning_the_trajectory(g, sim3)
        else:
            best = -1
            assert aligned is p and float(sim3.s) == 1.0
            back = align_trajectories.backtrack_from_aligning_the_trajectory(g, edict(R=sim3.R, t=sim3.t, s=sim3.s))
        stats = [float(v) for v in st.values()]
        if p.shape[0] > 10:      # evaluate_any_poses hands more than 10 poses to the Procrustes path (:304-305): the small-system method's own values
            err = ev.evaluate_camera_alignment(None, aligned, g)
            stats[2:] = [float(err.R.mean() * 180. / np.pi), float(err.t.mean())]
        out["stats"].append(np.array(stats, dtype=np.float32))
        out["aligned"].append(aligned.numpy().copy())
        out["sim3"].append(np.concatenate([sim3.R.reshape(9).numpy(), sim3.t.reshape(3).numpy(), [np.float32(sim3.s)]]).astype(np.float32))
        out["best"].append(best)
        out["scores"].append(np.array(scores, dtype=np.float64).reshape(-1, 3))
        out["back"].append(back.numpy().copy())
    return {k: np.stack(v) for k, v in out.items()}


def relative_gap(scores):
    """of the two smallest products"""
    v = np.sort(scores[:, 2])
    return (v[1] - v[0]) / v[1]


def measure(name, c, pose, gt):
    """-> (arrays to store, decisive [S], referee gaps [S])"""
    ref = reference_run(c, pose, gt)
    w = R.want(pose, gt, c["align"])
    S, B = pose.shape[:2]
    fx, decisive, gaps = {}, [], []
    dist = {k: [] for k in ("stats", "aligned", "sim3", "scores")}
    round_trip = []
    for s in range(S):
        ws = R.set_of(w, s)
        got = dict(stats=ref["stats"][s], errors=ws["errors"], aligned=ref["aligned"][s], sim3=ref["sim3"][s], scores=ref["scores"][s])
        for k in ("stats", "aligned", "sim3", "scores"):
            assert R.same_pattern(got[k], ws[k]), (name, s, k, got[k], ws[k])
        d = R.distances(got, ws)
        for k in dist:
            dist[k].append(d[k])
        if c["align"] and name not in R.DEGENERATE:
            order = np.argsort(ws["scores"][:, 2], kind="stable")[:2]
            gap = relative_gap(ws["scores"])
            rel = np.abs(ref["scores"][s][order, 2] - ws["scores"][order, 2]) / ws["scores"][order, 2]
            decisive.append(bool(gap >= 10 * rel.max()))
            gaps.append(gap)
            if decisive[-1]:
                assert ref["best"][s] == ws["best"], (name, s, ref["best"][s], ws["best"])
        else:
            decisive.append(name in R.DEGENERATE or not c["align"])        # NaN first / no search: nothing to decide
            gaps.append(np.inf)
            assert ref["best"][s] == ws["best"], (name, s, ref["best"][s], ws["best"])
        # the referee's own round trip: backtrack of the ground truth under ITS similarity as the kernel stores it (fp32) against the estimated poses
        sim32 = ws["sim3"].astype(np.float32)
        g = gt[s if gt.shape[0] > 1 else 0]
        if np.isfinite(sim32).all():
            rt = R.spacings(R.backtrack(g, sim32), pose[s].astype(np.float64), R.pose_floor(B, ws["floor"]))
            round_trip.append(np.nanmax(rt))
        else:
            round_trip.append(np.nan)
    for k, v in ref.items():
        fx[f"ref_{k}_{name}"] = v
    for k, v in dist.items():
        fx[f"refdist_{k}_{name}"] = np.stack(v)
    fx[f"decisive_{name}"] = np.array(decisive)
    fx[f"roundtrip_{name}"] = np.array(round_trip)
    return fx, decisive, gaps


def main():
    fx = {}
    for k, (name, c) in enumerate(R.CASES.items()):
        for attempt in range(200):
            seed = 1000 * (k + 1) + attempt
            pose, gt = make_inputs(c, seed)
            arrays, decisive, gaps = measure(name, c, pose, gt)
            if min(gaps) >= 1e-6 and (c["noise"] < 0.05 or c["kind"] != "noisy" or all(decisive)):
                break
        else:
            raise AssertionError(f"{name}: no seed gives a decisive case")
        fx[f"pose_{name}"], fx[f"gt_{name}"], fx[f"seed_{name}"] = pose, gt, np.array(seed)
        fx.update(arrays)
        worst = {q: float(np.nanmax(arrays[f"refdist_{q}_{name}"])) if np.isfinite(arrays[f"refdist_{q}_{name}"]).any() else float("nan")
                 for q in ("stats", "aligned", "sim3", "scores")}
        print(f"{name:16s} seed {seed} best {arrays[f'ref_best_{name}']} decisive {decisive} gap {min(gaps):.2e} round trip {arrays[f'roundtrip_{name}']} "
              f"reference to float64 (spacings): {worst}")
    if "coincident_b3" in R.CASES:
        sc = fx["ref_scores_coincident_b3"][0][:, 2]
        assert np.isnan(sc[[0, 2]]).all() and np.isfinite(sc[[1, 3, 4, 5]]).all() and fx["ref_best_coincident_b3"][0] == 0 and np.isnan(fx["ref_aligned_coincident_b3"]).all()
        assert np.isnan(fx["ref_scores_identity_b3"]).all() and np.isfinite(fx["ref_stats_identity_b3"][0, :2]).all() and np.isnan(fx["ref_stats_identity_b3"][0, 2:]).all()
    np.savez_compressed(R.FIXTURE, **fx)
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes,", len(fx), "arrays,", len(R.CASES), "cases")


if __name__ == "__main__":
    main()
