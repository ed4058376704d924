"""The float64 referee of the pose-evaluation kernels (csrc/pose_eval.h): numpy float64 on the stored fp32 operands,
following joint_pose_nerf_trainer.py:160-311 and align_trajectories.py:94-101 line by line -- padded 4 x 4 products with their zero
terms, the double inversion of evaluate_camera_alignment, np.argmin's choice -- with ONE thing taken from the reference's fp32 world: the
clamp bound of rotation_distance as its fp32 tensor holds it, float32(1 - 1e-7).  Also the case table shared by the generator
(tests/golden/make_pose_eval_golden.py), the CPU tests and the GPU tests, and the comparison in fp32 spacings.

The bound (BOUND = 1 spacing): the kernel's arithmetic is double on the same operands, so it differs from this file by operation order
only (~1e-16 relative, times the conditioning of acos at the clamp, ~2e3); a stored value is then rounded once (half a spacing) and the
comparison rounds the referee's value to the fp32 grid to take its spacing (the other half).  The spacing is taken at max(|value|,
floor): 1 for the entries of a rotation matrix, the set's largest camera-centre norm for translations and distances (each is a sum of
terms of that size), nothing for angles, the scale and the product of the angle and the distance: each of those is within a spacing
taken at its own value."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "pose_eval.npz")
BOUND = 1.0
MAX_VIEWS, MAX_PAIRS = 10, 90
CLAMP = float(np.float32(1.0 - 1e-7))
NOISES = (1e-3, 0.05, 0.3)


def _cases():
    C = {}

    def add(name, B, **kw):
        C[name] = dict(dict(B=B, S=1, gt_sets=1, noise=0.05, kind="noisy", align=True), **kw)
    for noise in NOISES:
        for B in (2, 3, 9, 10, 12):        # P = 2; a typical system; P = 72 crosses a wave; P = 90; candidates capped, errors over 12
            add(f"b{B}_n{noise:g}", B, noise=noise)
        add(f"s3_gt1_n{noise:g}", 4, S=3, noise=noise)
        add(f"s3_gt3_n{noise:g}", 4, S=3, gt_sets=3, noise=noise)
    add("exact_b3", 3, noise=0.0)                              # every pose on the clamp floor
    add("exact_b9", 9, noise=0.0)
    add("pi_b3", 3, noise=0.0, kind="pi")                      # one rotation by pi: the lower clamp
    add("coincident_b3", 3, kind="coincident")                 # two coincident estimated centres: candidates 0 and 2 NaN, NaN first
    add("identity_b3", 3, kind="identity")                     # identity initialisation: all NaN after alignment, finite before
    add("noalign_b3", 3, align=False)
    add("noalign_b1", 1, align=False)
    add("noalign_s3", 4, S=3, gt_sets=3, align=False)
    return C


CASES = _cases()
DEGENERATE = ("coincident_b3", "identity_b3")


@functools.lru_cache(maxsize=1)
def fixture():
    return dict(np.load(FIXTURE))


def inputs(name, fx=None):
    """-> (pose [S,B,3,4], pose_gt [gt_sets,B,3,4]) float32, as stored"""
    fx = fixture() if fx is None else fx
    return fx[f"pose_{name}"], fx[f"gt_{name}"]


# ---- float64 arithmetic on [...,3,4] poses
def invert(p):
    R, t = p[..., :3], p[..., 3:]
    Rt = np.swapaxes(R, -1, -2)
    return np.concatenate([Rt, ((-Rt)[..., :, :, None] * t[..., None, :, :]).sum(-2)], axis=-1)


def pad(p):
    bottom = np.broadcast_to(np.array([0, 0, 0, 1.0]), p[..., :1, :].shape)
    return np.concatenate([p, bottom], axis=-2)


def matmul(a, b):
    """padded product with every term written out: 0 * inf is NaN, as in the reference's 4 x 4 matmul"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (pad(a)[..., :, :, None] * pad(b)[..., None, :, :]).sum(-2)[..., :3, :]


def rotation_distance(R1, R2):
    with np.errstate(invalid="ignore"):
        x = ((R1 * R2).sum((-1, -2)) - 1.0) / 2.0
        x = np.where(x < -CLAMP, -CLAMP, np.where(x > CLAMP, CLAMP, x))
        return np.arccos(x)


def alignment_errors(c2w, gt_c2w):
    with np.errstate(invalid="ignore", over="ignore"):
        d = c2w[..., 3] - gt_c2w[..., 3]
        return rotation_distance(c2w[..., :3], gt_c2w[..., :3]), np.sqrt((d * d).sum(-1))


def pair_of(p, B):
    n = min(B, MAX_VIEWS)
    a, r = divmod(p, n - 1)
    return a, r + (r >= a)


def similarity(c2w, gt_c2w, a, b):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        f, t = c2w[a, :, 3] - c2w[b, :, 3], gt_c2w[a, :, 3] - gt_c2w[b, :, 3]
        scale = np.sqrt((t * t).sum()) / np.sqrt((f * f).sum())
        sa = c2w[a].copy()
        sa[:, 3] = sa[:, 3] * scale
        return matmul(gt_c2w[a], invert(sa)), scale


def align(T, scale, c2w):
    with np.errstate(invalid="ignore", over="ignore"):
        sc = c2w.copy()
        sc[..., 3] = sc[..., 3] * scale
        return invert(matmul(T, sc))


def want_set(pose, gt, do_align):
    """one set, float32 [B,3,4] each -> float64 dict"""
    with np.errstate(invalid="ignore", over="ignore"):
        B = pose.shape[0]
        c2w, gt_c2w = invert(pose.astype(np.float64)), invert(gt.astype(np.float64))
        eR0, et0 = alignment_errors(c2w, gt_c2w)
        before = (eR0.sum() / B * 180. / np.pi, et0.sum() / B)
        P = min(B, MAX_VIEWS) * (min(B, MAX_VIEWS) - 1) if do_align else 0
        scores = np.zeros((P, 3))
        for p in range(P):
            T, scale = similarity(c2w, gt_c2w, *pair_of(p, B))
            eR, et = alignment_errors(invert(align(T, scale, c2w)), gt_c2w)
            scores[p, 0], scores[p, 1] = eR.sum() / B * 180. / np.pi, et.sum() / B
            scores[p, 2] = scores[p, 1] * scores[p, 0]
        if P:
            best = int(np.argmin(scores[:, 2]))
            T, scale = similarity(c2w, gt_c2w, *pair_of(best, B))
            aligned = align(T, scale, c2w)
            eR1, et1 = alignment_errors(invert(aligned), gt_c2w)
            after = (scores[best, 0], scores[best, 1])
        else:
            best, T, scale, aligned, eR1, et1, after = -1, np.eye(3, 4), 1.0, pose.astype(np.float64), eR0, et0, before
        # the floor of the translations' spacing: the largest camera-centre norm in the set (finite ones)
        norms = np.concatenate([np.linalg.norm(m[..., 3], axis=-1).reshape(-1) for m in (c2w, gt_c2w, invert(aligned))])
        return dict(stats=np.array([*before, *after]), errors=np.stack([np.stack([eR0, et0], -1), np.stack([eR1, et1], -1)]), aligned=aligned,
                    sim3=np.concatenate([T[:, :3].reshape(9), T[:, 3], [scale]]), best=best, scores=scores, floor=float(np.max(norms[np.isfinite(norms)])))


def want(pose, gt, do_align=True):
    """[S,B,3,4] and [gt_sets,B,3,4] float32 -> float64 dict with a leading set axis"""
    sets = [want_set(pose[s], gt[s if gt.shape[0] > 1 else 0], do_align) for s in range(pose.shape[0])]
    return {k: np.stack([np.asarray(w[k]) for w in sets]) for k in sets[0]}


def backtrack(gt_w2c, sim):
    """align_trajectories.py:94-101 in float64: gt_w2c [N,3,4], sim [13]"""
    c = invert(gt_w2c.astype(np.float64))
    sim = sim.astype(np.float64)
    R, t, s = sim[:9].reshape(3, 3), sim[9:12], sim[12]
    al = np.concatenate([R.T @ c[:, :, :3], ((R.T / s) @ (c[:, :, 3:] - t.reshape(1, 3, 1)))], axis=-1)
    return invert(al)


# ---- the comparison
def spacings(got, want64, floor=0.0, at=None):
    """|got - want| in fp32 spacings at max(|at|, floor), elementwise (at: the referee's value where `want64` is another's, by default
    want64 itself); NaN where either is not finite"""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    at = want64 if at is None else np.asarray(at, dtype=np.float64)
    fin = np.isfinite(want64) & np.isfinite(at)
    at = np.maximum(np.abs(np.where(fin, at, 1.0)), floor)
    sp = np.spacing(at.astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(fin, np.abs(got - want64) / sp, np.nan)


def same_pattern(got, want64):
    """NaN and +-inf in the same places"""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    return np.array_equal(np.isnan(got), np.isnan(want64)) and np.array_equal(np.where(np.isinf(got), np.sign(got), 0), np.where(np.isinf(want64), np.sign(want64), 0))


def pose_floor(B, floor):
    """[B,3,4] floors of a pose array: 1 for the rotation, `floor` for the translation column"""
    f = np.ones((B, 3, 4))
    f[..., 3] = floor
    return f


def distances(got, w, against=None):
    """got / w: dicts of one SET (stats [4], errors [2,B,2], aligned [B,3,4], sim3 [13], scores [P,3]), w the referee's -> {output:
    spacings array} of got from w -- or from `against` (a dict of some of the outputs, the reference's values), still in the spacings
    of the referee's values"""
    fl = w["floor"]
    B, P = w["aligned"].shape[0], len(w["scores"])
    floors = dict(stats=np.array([0, fl, 0, fl]), errors=np.broadcast_to(np.array([0, fl]), (2, B, 2)), aligned=pose_floor(B, fl),
                  sim3=np.concatenate([np.ones(9), np.full(3, fl), [0.0]]),
                  scores=np.broadcast_to(np.array([0, fl, 0]), (P, 3)))
    target = w if against is None else against
    return {k: spacings(got[k], target[k], floors[k], at=w[k]) for k in floors if k in target and k in got}


def worst(d):
    vals = [np.nanmax(v) for v in d.values() if v.size and np.isfinite(v).any()]
    return max(vals) if vals else 0.0


def set_of(res, s):
    """set s of a result with a leading set axis (a dict of numpy arrays) -> one set's dict"""
    return {k: v[s] for k, v in res.items()}


def result_arrays(res):
    """an evaluate_poses result (torch, with or without a set axis) -> dict of numpy arrays with a leading set axis"""
    single = res.stats.dim() == 1
    out = {k: res[k].detach().cpu().numpy() for k in ("stats", "errors", "aligned", "best", "scores")}
    out["sim3"] = res.sim3.packed.detach().cpu().numpy()
    return {k: v[None] for k, v in out.items()} if single else out
