"""The cases of the depth-consistency front end and the ray sampler and a float64 referee of the pose outputs.
Nothing here imports torch or the package; tests/test_pick_cpu.py and tests/test_pick_gpu.py hold the package to it,
tests/golden/make_pick_golden.py records what the reference's own functions did on these cases (tests/golden/pick.npz).

Pixel cases: sample_rays (patch None) and sample_rays_for_patch on images of 7 x 9 and 12 x 10 -- not square, so that x and y cannot be
swapped -- with nbr 1, 5 and 300 (one workgroup of the kernel plus 44 rows; the pools of the two images are smaller, so a third image of
19 x 21 holds the 300 rows without a patch, and the patches of 2 and 3 give 396 and 720 rows on 12 x 10), a centre fraction of 0 and
0.4, and nbr None (nothing is drawn).  Strategy cases: RaySamplingStrategy.__call__ with the mask fraction 0 on the same two images.
Pose cases: 1, 2, 3, 6 and 70 cameras (70: more cameras than the lanes of the one wave), one set as [B,3,4].

The referee: float64 arithmetic on the stored float32 operands, and a bound per entry derived from the roundings a float32 evaluation
makes (u = 2^-24):
  * a copied entry (a rotation entry of an inverse, all of pose_w2c_ref) has none: bound 0;
  * a translation entry -(r0 t0 + r1 t1 + r2 t2) of exact operands, fused or not, in any order: gamma_3 sum |r_i||t_i|,
    gamma_3 = 3u / (1 - 3u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1);
  * a blended entry fl(fl(w a) + fl(v b)): u|wa| + u|vb| for the products and u|wa + vb| <= u(|wa| + |vb|) for the sum, together
    2u (|wa| + |vb|), plus |w| da + |v| db for operands that carry errors da, db themselves;
  * the translation entry of the inverse of the blend: gamma_3 sum |R_k||t_k| on the blended values plus sum (dR_k |t_k| + |R_k| dt_k).
Products of two errors are O(u^2) relative; a factor 1 + 2^-10 on every bound covers them."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pick.npz")
BLOCK = 256                      # csrc/pick.h PICK_BLOCK
IMAGES = ((7, 9), (12, 10))      # (H, W)
BIG_IMAGE = (19, 21)             # its pool of 18 x 20 pixels holds BLOCK + 44 picks
NBRS = (1, 5, BLOCK + 44)
FRACTIONS = (0.0, 0.4)
PATCHES = (None, 1, 2, 3)        # None: sample_rays; a number: sample_rays_for_patch
PRECROP = 0.5
U = 2.0 ** -24
GAMMA3 = 3 * U / (1 - 3 * U)
SLACK = 1 + 2.0 ** -10
MIN_GAP = 1e-6                   # rad: between the smallest and the second-smallest angular distance of every stored pose set


def pixel_cases():
    """name -> dict(H, W, nbr, fraction, patch, seed)"""
    cases, seed = {}, 100
    for H, W in IMAGES:
        for nbr in NBRS:
            for f in FRACTIONS:
                for p in PATCHES:
                    seed += 1
                    cases[f"px_{H}x{W}_n{nbr}_f{f}_p{p}"] = dict(H=H, W=W, nbr=nbr, fraction=f, patch=p, seed=seed)
    for f in FRACTIONS:
        seed += 1
        H, W = BIG_IMAGE
        cases[f"px_{H}x{W}_n{NBRS[-1]}_f{f}_pNone"] = dict(H=H, W=W, nbr=NBRS[-1], fraction=f, patch=None, seed=seed)
    for f in FRACTIONS:
        for p in (None, 2):
            seed += 1
            cases[f"px_7x9_nNone_f{f}_p{p}"] = dict(H=7, W=9, nbr=None, fraction=f, patch=p, seed=seed)
    return cases


def pool_of(case):
    """the pool A of a pixel case as (a_w, a_h)"""
    border = 1 if case["patch"] is None else case["patch"] - 1
    return case["W"] - border, case["H"] - border


def centre_box(H, W, precrop=PRECROP):
    dH, dW = int(H // 2 * precrop), int(W // 2 * precrop)
    return W // 2 - dW, H // 2 - dH, 2 * dW, 2 * dH


def counts_of(case):
    """(picks of the pool, picks of the centre box) of a pixel case with a number of pixels"""
    n_center = int(case["nbr"] * case["fraction"]) if case["fraction"] > 0 else 0
    return case["nbr"] - n_center, n_center


def strategy_cases():
    """name -> dict(H, W, B, nbr_pixels, fraction, patch (None: loss_weight.depth_patch None), in_center, idx_imgs, seed)"""
    cases, seed = {}, 500
    for H, W in IMAGES:
        for f in FRACTIONS:
            for p in (None, 2, 3):
                for in_center in (False, True):
                    seed += 1
                    nbr = 600 if (H, W) == IMAGES[1] and not in_center else 37
                    cases[f"st_{H}x{W}_f{f}_p{p}_c{int(in_center)}"] = dict(H=H, W=W, B=2, nbr_pixels=nbr, fraction=f, patch=p, in_center=in_center,
                                                                          idx_imgs=None, seed=seed)
    cases["st_12x10_idx"] = dict(H=12, W=10, B=3, nbr_pixels=23, fraction=0.4, patch=None, in_center=False, idx_imgs=[1], seed=seed + 1)
    return cases


def strategy_pool(case):
    p = case["patch"]
    return (case["W"], case["H"]) if p is None else (case["W"] - p - 1, case["H"] - p - 1)


# ---- poses
POSE_CASES = {
    # name -> (B, id_self, [B,3,4] form, seed)
    "pose_b1": (1, 0, False, 11), "pose_b2": (2, 1, False, 12), "pose_b3_3x4": (3, 0, True, 13), "pose_b6": (6, 4, False, 14),
    "pose_b6_first": (6, 0, False, 15), "pose_b70": (70, 37, False, 16),
}


def poses_of(B, seed, three_by_four=False):
    """B world-to-camera poses float32: random rotations, camera centres 2 to 5 away from the scene centre"""
    rs = np.random.RandomState(seed)
    out = np.zeros((B, 4, 4), dtype=np.float64)
    for b in range(B):
        q, r = np.linalg.qr(rs.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        c = rs.standard_normal(3)
        c = c / np.linalg.norm(c) * rs.uniform(2.0, 5.0)
        out[b, :3, :3], out[b, :3, 3], out[b, 3, 3] = q, -q @ c, 1.0
    out = out.astype(np.float32)
    return np.ascontiguousarray(out[:, :3]) if three_by_four else out


def inverse64(m):
    """the transpose inverse of [..,3+,4] in float64, and the bound of its float32 evaluation from exact operands"""
    m = np.asarray(m, dtype=np.float64)
    R, t = m[:3, :3], m[:3, 3]
    out, bound = np.zeros((4, 4)), np.zeros((4, 4))
    out[:3, :3], out[:3, 3], out[3, 3] = R.T, -(R.T @ t), 1.0
    bound[:3, 3] = GAMMA3 * (np.abs(R.T) @ np.abs(t))
    return out, bound


def centres32(poses_w2c):
    """the camera centres -R^T t of float32 poses, evaluated in float32 (no fused multiply-add, left to right)"""
    p = np.asarray(poses_w2c, dtype=np.float32)
    R, t = p[:, :3, :3], p[:, :3, 3]
    prod = R * t[:, :, None]                                # prod[b, k, r] = R[b, k, r] t[b, k]
    return -((prod[:, 0] + prod[:, 1]) + prod[:, 2])


def angular_dists(centres, id_self):
    """data_utils.py:248-252, :304-306 in float64 on the given centres; the self entry is 1e3"""
    v = np.asarray(centres, dtype=np.float64)
    unit = v / (np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None] + 1e-6)
    p = unit[id_self][None] * unit
    d = np.arccos(np.clip((p[:, 0] + p[:, 1]) + p[:, 2], -1.0, 1.0))
    d[id_self] = 1e3
    return d


def gap(centres, id_self):
    """the distance between the smallest and the second-smallest angular distance (inf with fewer than two other cameras)"""
    d = np.sort(np.delete(angular_dists(centres, id_self), id_self))
    return float(d[1] - d[0]) if len(d) >= 2 else float("inf")


def referee_pose(poses_w2c, id_self, w, id_other):
    """-> {name: (value float64 [4,4], bound [4,4])} of the four matrices for the given other camera"""
    p = np.asarray(poses_w2c, dtype=np.float32)
    w32, v32 = float(np.float32(w)), float(np.float32(1.0 - float(w)))
    ref = np.zeros((4, 4))
    ref[:p.shape[1]] = p[id_self].astype(np.float64)
    if p.shape[1] == 3:
        ref[3, 3] = 1.0
    a, da = inverse64(p[id_self])
    b, db = inverse64(p[id_other])
    blend = w32 * a + v32 * b
    dblend = 2 * U * (np.abs(w32 * a) + np.abs(v32 * b)) + abs(w32) * da + abs(v32) * db
    R, t, dR, dt = blend[:3, :3], blend[:3, 3], dblend[:3, :3], dblend[:3, 3]
    unseen, dunseen = np.zeros((4, 4)), np.zeros((4, 4))
    unseen[:3, :3], unseen[:3, 3], unseen[3, 3] = R.T, -(R.T @ t), 1.0
    dunseen[:3, :3] = dR.T
    dunseen[:3, 3] = GAMMA3 * (np.abs(R.T) @ np.abs(t)) + dR.T @ np.abs(t) + np.abs(R.T) @ dt
    return {"pose_w2c_ref": (ref, np.zeros((4, 4))), "pose_c2w_ref": (a, da * SLACK), "pose_c2w_other": (b, db * SLACK),
            "pose_w2c_at_unseen": (unseen, dunseen * SLACK)}


POSE_OUTS = ("pose_w2c_ref", "pose_c2w_ref", "pose_c2w_other", "pose_w2c_at_unseen")


def within(got, want, bound):
    """every entry of got within its bound of the referee; -> (ok, worst |error| / bound over the entries with a bound)"""
    got, err = np.asarray(got, dtype=np.float64), None
    err = np.abs(got - want)
    ok = bool(np.all(err <= bound))
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    return ok, ratio


def fixture():
    return np.load(FIXTURE)
