"""Float64 referee of the depth-consistency kernels (tests/test_dcons_cpu.py, tests/test_dcons_gpu.py, tests/golden/make_dcons_golden.py):
the formulas as include/sparf_hip.h states them, in float64 on the fp32 operands cast to double.  The forward chain is numpy, written
element by element in the operation order of batched_geometry_utils.py:244-247 and :262-265 (no BLAS call: the same bits on every
machine); the gradients come from torch.float64 autograd on the same order, so the hand-derived gathers and seeds of csrc/dcons.hip are
checked against a derivation they do not share.

Bounds (the issue's, from the arithmetic contract: double arithmetic on the fp32 operands, double sums, one rounding per stored value):
every stored forward element (pixels, pseudo depth), the loss and avg_vis_weight within ONE fp32 spacing of the float64 value; every
gradient tensor relative L2 <= 2^-22; dst / src / count and the masks EQUAL (the fixture keeps every point 0.01 px away from the four
image bounds, 1e-4 from depth_min and 1e-4 from the visibility threshold).  The torch restatement (sparf_amd.losses.*_torch) runs in
fp32 like the reference and is held to 4x the reference's own distance from this referee.

Fixture (tests/golden/dcons.npz): ONE scene of NS[-1] points; size n is its first n points (every per-point value is independent of n;
the loss and its seeds, which are not, are stored per size).
  K, T_c2w, P_unseen, HW, depth_min       the general K (both views), the reference view's c2w [4,4], the unseen w2c [4,4]
  px, d, dr, drf                          integer pixels [N,2] and depth of the reference view; rendered depths (coarse, fine)
  uv, z, d_d (and uv_<n>, z_<n>, d_d_<n>) the REFERENCE's fp32 projection of all (of the first n) points and d (sum uv g_uv + z g_z over
                                          valid) / d d, from a run of its own per size: a matrix product of another size may round differently
  valid                                   the mask, equal in fp32 and float64
  uv_<pattern>_<base>, z_.., d_d_..       the same three of the REFERENCE on pattern_rows(valid[:base], pattern), for base in PATTERN_BASES
  Xw, uv_p_<n>, z_p_<n>, d_Xw_<n>         world points (float32 of the referee's) of the first POINTS_NS[-1] points; for n in POINTS_NS the
                                          reference's projection of the first n of THOSE and the gradient to them
  loss_<case>_<n> (loss, avg_vis_weight)  the reference's compute_diff_loss lines on the first n points, for every n
  seeds_<case>_<n>                        [3 or 2, n]: d z_pseudo, d depth(, d depth_fine) for n in SEED_NS
Upstream gradients, visibilities and opacities are exact dyadic functions of the point index (g_uv, g_z, vis, opacity below).
"""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dcons.npz")
# 63 / 64 / 65: a wave; 255 / 256 / 257: a tile of the compaction; 4096 / 4097: the last size one workgroup handles in one launch and
# the first that takes the counts launch; 8200: two full chunks and a partial third
NS = (1, 63, 64, 65, 255, 256, 257, 4096, 4097, 8200)
POINTS_NS = (1, 65, 257, 4097)
SEED_NS = (1, 63, 64, 65, 255, 256, 257, 4097)
LOSS_CASES = {"huber": ("huber", 0), "l1": ("l1", 0), "mse": ("mse", 0), "huber_fine": ("huber", 1), "l1_fine": ("l1", 1), "mse_fine": ("mse", 1)}
PATTERNS = ("drawn", "all", "none", "first", "last", "alternating")
# the first points whose rows the patterns rearrange: one workgroup; and enough that `all` (four in five are valid) takes the counts launch
PATTERN_BASES = (257, 5400)
VIS_THRESH = 0.2
GRAD_BOUND = 2.0 ** -22


def fixture():
    return dict(np.load(FIXTURE))


# ---- exact functions of the point index k (dyadic rationals: the same fp32 bits wherever they are computed)
def g_uv(n):
    k = np.arange(n, dtype=np.int64)
    return np.stack([((k * 37) % 101 - 50) / 64.0, ((k * 53) % 89 - 44) / 64.0], 1).astype(np.float32)


def g_z(n):
    k = np.arange(n, dtype=np.int64)
    return (((k * 29) % 97 - 48) / 32.0).astype(np.float32)


def vis(n):
    """in (0, 1): j / 128 + 1 / 256, so never within 7e-4 of the 0.2 threshold; about four in five are kept"""
    k = np.arange(n, dtype=np.int64)
    return (((k * 45) % 128) / 128.0 + 1.0 / 256.0).astype(np.float32)


def opacity(n, fine=False):
    k = np.arange(n, dtype=np.int64)
    return ((((k * (61 if fine else 43)) % 97) + 159) / 256.0).astype(np.float32)


# ---- the forward chain, element by element
def inverse3(K):
    """adj(K) / det(K)"""
    K = np.asarray(K, dtype=np.float64)
    c00, c01, c02 = K[1, 1] * K[2, 2] - K[1, 2] * K[2, 1], K[1, 2] * K[2, 0] - K[1, 0] * K[2, 2], K[1, 0] * K[2, 1] - K[1, 1] * K[2, 0]
    det = K[0, 0] * c00 + K[0, 1] * c01 + K[0, 2] * c02
    return np.array([[c00, K[0, 2] * K[2, 1] - K[0, 1] * K[2, 2], K[0, 1] * K[1, 2] - K[0, 2] * K[1, 1]],
                     [c01, K[0, 0] * K[2, 2] - K[0, 2] * K[2, 0], K[0, 2] * K[1, 0] - K[0, 0] * K[1, 2]],
                     [c02, K[0, 1] * K[2, 0] - K[0, 0] * K[2, 1], K[0, 0] * K[1, 1] - K[0, 1] * K[1, 0]]]) / det


def pose44(P):
    P = np.asarray(P, dtype=np.float64)
    return P if P.shape[0] == 4 else np.concatenate([P, [[0.0, 0.0, 0.0, 1.0]]], 0)


def world(px, d, K_ref, T_c2w):
    """x = K^-1 [p, 1] d;  h = T [x, 1];  X_w = h[0:3] / (h[3] + 1e-6)   -> [n,3] float64"""
    px, d, Ki, T = np.asarray(px, dtype=np.float64), np.asarray(d, dtype=np.float64), inverse3(K_ref), pose44(T_c2w)
    x = [(Ki[r, 0] * px[:, 0] + Ki[r, 1] * px[:, 1] + Ki[r, 2]) * d for r in range(3)]
    h = [T[r, 0] * x[0] + T[r, 1] * x[1] + T[r, 2] * x[2] + T[r, 3] for r in range(4)]
    s = h[3] + 1e-6
    return np.stack([h[0] / s, h[1] / s, h[2] / s], 1)


def project(Xw, P_unseen, K_unseen):
    """g = P [X_w, 1];  X = g[0:3] / (g[3] + 1e-6);  y = K X;  uv = y[0:2] / (y[2] + 1e-6);  z = X[2]   -> ([n,2], [n]) float64"""
    Xw, P, K = np.asarray(Xw, dtype=np.float64), pose44(P_unseen), np.asarray(K_unseen, dtype=np.float64)
    g = [P[r, 0] * Xw[:, 0] + P[r, 1] * Xw[:, 1] + P[r, 2] * Xw[:, 2] + P[r, 3] for r in range(4)]
    s = g[3] + 1e-6
    X = [g[0] / s, g[1] / s, g[2] / s]
    y = [K[r, 0] * X[0] + K[r, 1] * X[1] + K[r, 2] * X[2] for r in range(3)]
    sy = y[2] + 1e-6
    return np.stack([y[0] / sy, y[1] / sy], 1), X[2]


def inside(uv, z, H, W, depth_min):
    """depth_cons_loss.py:252-254 on the values as stored: rounded to fp32, compared in fp32"""
    uv, z = np.asarray(uv).astype(np.float32), np.asarray(z).astype(np.float32)
    return ((uv[:, 0] >= np.float32(0)) & (uv[:, 1] >= np.float32(0)) & (uv[:, 0] <= np.float32(W - 1)) & (uv[:, 1] <= np.float32(H - 1)) &
            (z >= np.float32(depth_min)))


def near_margin(uv, z, H, W, depth_min, pix_margin=0.01, depth_margin=1e-4):
    uv, z = np.asarray(uv, dtype=np.float64), np.asarray(z, dtype=np.float64)
    return ((np.abs(uv[:, 0]) < pix_margin) | (np.abs(uv[:, 1]) < pix_margin) | (np.abs(uv[:, 0] - (W - 1)) < pix_margin) |
            (np.abs(uv[:, 1] - (H - 1)) < pix_margin) | (np.abs(z - float(np.float32(depth_min))) < depth_margin))


def compaction(mask):
    """-> (dst [n] int32: output row or -1, src [count] int32, count) of an ordered compaction"""
    mask = np.asarray(mask, dtype=bool)
    src = np.nonzero(mask)[0].astype(np.int32)
    dst = np.full(mask.shape[0], -1, dtype=np.int32)
    dst[src] = np.arange(src.shape[0], dtype=np.int32)
    return dst, src, int(src.shape[0])


# ---- the same order in torch.float64, for the gradients
def f64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).clone()


def _hom(x):
    return torch.cat([x, torch.ones_like(x[:, :1])], 1)


def world_t(px, d, K_ref, T_c2w):
    x = (_hom(px) @ torch.linalg.inv(K_ref).T) * d[:, None]
    h = _hom(x) @ T_c2w.T
    return h[:, :3] / (h[:, 3:] + 1e-6)


def project_t(Xw, P, K):
    g = _hom(Xw) @ P.T
    X = g[:, :3] / (g[:, 3:] + 1e-6)
    y = X @ K.T
    return y[:, :2] / (y[:, 2:] + 1e-6), X[:, 2]


def project_want(fx, n, Xw=None, px=None, d=None, guv=None, gz=None):
    """the float64 values of a project case on the given points (default: the first n of the fixture, back-projecting form):
    dict(uv [c,2], z [c], mask, dst, src, count, d_in: d (sum uv g_uv + z g_z) / d (d or Xw), Xw)"""
    H, W = (int(v) for v in fx["HW"])
    K, T, P = fx["K"], fx["T_c2w"], fx["P_unseen"]
    if Xw is None:
        px = fx["px"][:n] if px is None else px
        d = fx["d"][:n] if d is None else d
        leaf = f64(d).requires_grad_()
        Xw_t = world_t(f64(px), leaf, f64(K), f64(pose44(T)))
        Xw64 = world(px, d, K, T)
    else:
        leaf = f64(Xw).requires_grad_()
        Xw_t, Xw64 = leaf, np.asarray(Xw, dtype=np.float64)
    uv, z = project(Xw64, P, K)
    mask = inside(uv, z, H, W, fx["depth_min"])
    dst, src, count = compaction(mask)
    out = dict(uv=uv[mask], z=z[mask], mask=mask, dst=dst, src=src, count=count, Xw=Xw64)
    if guv is not None:
        uv_t, z_t = project_t(Xw_t, f64(pose44(P)), f64(K))
        m = torch.from_numpy(mask)
        out["d_in"] = np.zeros(tuple(leaf.shape))
        if count:
            out["d_in"] = torch.autograd.grad((uv_t[m] * f64(guv)).sum() + (z_t[m] * f64(gz)).sum(), leaf)[0].numpy()
    return out


def loss_want(zp, v, depth, op, depth_fine, op_fine, loss_type):
    """the float64 values of a loss case: dict(loss, avg, d_zp, d_depth[, d_depth_fine])"""
    t = [f64(a).requires_grad_(i in (0, 2, 4)) if a is not None else None for i, a in enumerate((zp, v, depth, op, depth_fine, op_fine))]
    m = t[0].shape[0]

    def term(dep, opa):
        w = t[1] * opa
        e = t[0] - dep
        a = e.abs()
        l = torch.where(a <= 1.0, 0.5 * e * e, a - 0.5) if loss_type == "huber" else a if loss_type == "l1" else e * e
        return (l * w).sum() / (m + 1e-6), w.sum() / (m + 1e-6)
    loss, avg = term(t[2], t[3])
    if depth_fine is not None:
        l2, avg = term(t[4], t[5])
        loss = loss + l2
    leaves = [x for i, x in enumerate(t) if i in (0, 2, 4) and x is not None]
    gs = torch.autograd.grad(loss, leaves)
    return dict(loss=loss.item(), avg=avg.item(), **{k: g.numpy() for k, g in zip(("d_zp", "d_depth", "d_depth_fine"), gs)})


def ref_of(fx, name, n, pattern="drawn"):
    """the reference's own fp32 result `name` of the run on the first n points (on the rows of a mask pattern of the first n points)"""
    if pattern != "drawn":
        return fx[f"{name}_{pattern}_{n}"]
    return fx[name] if n == NS[-1] and name in fx else fx[f"{name}_{n}"]


def loss_inputs(fx, n, fine):
    """(z_pseudo, vis, depth, opacity, depth_fine, opacity_fine) as float32 numpy: the reference's projected depth of the first n points
    against the stored rendered depths (differences on both sides of |e| = 1)"""
    return (fx["z"][:n], vis(n), fx["dr"][:n], opacity(n), fx["drf"][:n] if fine else None, opacity(n, True) if fine else None)


def pattern_rows(mask, pattern):
    """row indices into the fixture's points that give the mask pattern: as drawn, all valid, none valid, only the first valid, only
    the last valid, alternating"""
    good, bad = np.nonzero(mask)[0], np.nonzero(~mask)[0]
    if pattern == "drawn":
        return np.arange(mask.shape[0])
    if pattern == "all":
        return good
    if pattern == "none":
        return bad
    if pattern == "first":
        return np.concatenate([good[:1], bad])
    if pattern == "last":
        return np.concatenate([bad, good[:1]])
    k = min(good.shape[0], bad.shape[0])
    return np.stack([good[:k], bad[:k]], 1).reshape(-1)


def to_np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def fwd_excess(got, want64):
    """max over elements of |got - want| / spacing(fp32(|want|)): <= 1 passes"""
    got, want64 = to_np(got).astype(np.float64), np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape, (got.shape, want64.shape)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want64) / np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)))


def l2(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


def rel_l2(got, want64):
    got, want64 = to_np(got).astype(np.float64), np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape, (got.shape, want64.shape)
    den = l2(want64)
    return l2(got - want64) / den if den > 0 else l2(got - want64)
