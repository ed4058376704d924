"""Float64 referee of the photometric / mask / depth-patch kernel (tests/test_photo_cpu.py, tests/test_photo_gpu.py,
tests/golden/make_photo_golden.py): the formulas as include/sparf_hip.h states them, in float64 on the fp32 operands cast to double.  The
forward values are numpy, written element by element (no BLAS call: the same bits on every machine); the gradients come from
torch.float64 autograd on the same formulas, so the hand-derived seeds of csrc/photo.hip are checked against a derivation they do not share.

Bounds (the issue's, from the arithmetic contract: double arithmetic on the fp32 operands, double sums, one rounding per stored value;
the ones tests/dcons_referee.py uses): out[0..4] within ONE fp32 spacing of the float64 value; every seed tensor relative L2 <= 2^-22;
seeds of constant patches exactly 0.  (c is 0.001 here, as the formula has it; the kernel is handed a float, (double)0.001f, 4.7e-8 away in
relative terms: that distance is inside the bound and shows on a case that is one constant patch, whose value is all c.)  The torch restatement (sparf_amd.losses.*_torch) runs in fp32 like the reference and is held to
4x the reference's own distance from this referee.

Fixture (tests/golden/photo_regu.npz, arrays only): ONE 24 x 40 image set with B = 3
  image [3,3,24,40], fg_mask [3,1,24,40]   colours in [0, 1]; a mask that is about 40 % foreground
  pool_check                               a few values of the row pools below, so that a test sees a generator that drifted
  ref_<case> [5]                           the REFERENCE's own fp32 (render, fg_mask, depth_patch, mse, mse_fine) on the CPU: its
                                           unmodified BasePhotoandReguLoss.compute_loss and compute_mse_on_rays (0 for what is off)
  seed_<case>_<tensor>                     its autograd gradient of each term to its own tensor, for the cases that list seeds
The per-row inputs are NOT stored: pools() draws them from np.random.RandomState(SEED) (Mersenne twister and the legacy normal: the same
stream on every machine and numpy version) for POOL rows; a case of `rows` rows uses the first `rows` entries.
  pred = target + e, e uniform in (-0.9, 0.9): both sides of the Huber kink at 0.5; an element whose |e| lies within 1e-3 of 0.5 is
  redrawn (a condition, at most 1 % of any case, asserted by the generator together with: the side of the kink agrees between the fp32
  difference and the float64 one on every case); opacities in [0.02, 0.98], so fg - opacity is never 0; depths per patch = a base in
  [1.2, 5] + N(0, 0.05), every 7th patch exactly constant (all its r = 0: its value is M^2 c, its gradient exactly 0).
Upstream scalars are dyadic (UPSTREAM).
"""
import functools
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photo_regu.npz")
SEED = 20268
H, W, B_SET = 24, 40, 3
HW = H * W
POOL = 8200
# rows per image with B = 1: a wave; a tile; the last one-launch size and the first two-launch size; two chunks and a partial third
NS = (1, 63, 64, 65, 255, 256, 257, 4096, 4097, 8200)
SEED_NS = (1, 63, 64, 65, 255, 256, 257, 4097)
KINDS = ("mse", "huber")
DELTA, CHARBONNIER, KINK_MARGIN = 0.5, 0.001, 1e-3
CHUNK = 4096                     # csrc/photo.h PHOTO_CHUNK
GRAD_BOUND = 2.0 ** -22
UPSTREAM = dict(render=0.75, fg_mask=1.5, depth_patch=0.625)
OUT_KEYS = ("render", "fg_mask", "depth_patch", "mse", "mse_fine")
TENSORS = ("rgb", "rgb_fine", "opacity", "opacity_fine", "depth", "depth_fine")
TERM_OF = dict(rgb="render", rgb_fine="render", opacity="fg_mask", opacity_fine="fg_mask", depth="depth_patch", depth_fine="depth_patch")
COLOUR_SEEDS, PATCH_SEEDS = ("rgb", "rgb_fine", "opacity", "opacity_fine"), ("depth", "depth_fine")


def _cases():
    C = {}

    def add(name, **kw):
        C[name] = dict(dict(B=1, form="shared", fine=True, mask=True, patch=0, views=(0,), seeds=()), **kw)
    for kind in KINDS:
        for n in NS:
            add(f"n{n}_{kind}", N=n, kind=kind, seeds=COLOUR_SEEDS if n in SEED_NS else ())
        # the index forms at B = 3: one list for all images; one per image, with repeated indices; none (full images: 2880 rows in one
        # launch, and 5 views of the same set for 4800 rows in two)
        for n in (64, 1368):
            for form in ("shared", "per_image"):
                add(f"{form}{n}_{kind}", B=3, N=n, form=form, patch=2, kind=kind, views=(0, 1, 2), seeds=TENSORS if n == 64 else ())
        add(f"full3_{kind}", B=3, N=HW, form="none", patch=2, kind=kind, views=(0, 1, 2))
        add(f"full5_{kind}", B=5, N=HW, form="none", patch=2, kind=kind, views=(0, 1, 2, 0, 1))
        # the terms
        add(f"colour_{kind}", N=257, kind=kind, fine=False, mask=False, seeds=("rgb",))
        add(f"fine_{kind}", N=257, kind=kind, mask=False, seeds=("rgb", "rgb_fine"))
        add(f"mask_{kind}", N=257, kind=kind, fine=False, seeds=("rgb", "opacity"))
        add(f"all256_{kind}", N=256, kind=kind, patch=2, seeds=TENSORS)
        add(f"all4100_{kind}", N=4100, kind=kind, patch=2)
    # the depth patch: P = 2 (the default); P = 3 (9 rows: patches straddle waves, and 4104 rows: one straddles the chunk); P = 8 (a patch
    # is a whole wave)
    for P, ns, stored in ((2, (64, 256, 4096, 4100), (64, 256, 4100)), (3, (9, 63, 576, 4104), (9, 63, 576, 4104)), (8, (64, 4096, 4160), (64, 4160))):
        for n in ns:
            add(f"p{P}_{n}", N=n, kind="mse", mask=False, patch=P, seeds=PATCH_SEEDS if n in stored else ())
    return C


CASES = _cases()


def fixture():
    return dict(np.load(FIXTURE))


# ---- the inputs
def make_images(rs):
    """-> (image [3,3,H,W] float32 in [0, 1], fg_mask [3,1,H,W] bool, about 40 % foreground: a disc and noise)"""
    image = rs.random_sample((B_SET, 3, H, W)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    disc = ((yy - 11.5) ** 2 + (xx - 19.5) ** 2 < 110.0)[None, None]
    mask = np.where(rs.random_sample((B_SET, 1, H, W)) < 0.15, ~disc, disc)
    return image, mask


@functools.lru_cache(maxsize=1)
def pools():
    """the per-row inputs of every case (see the module docstring); -> dict of arrays with POOL rows, and `redrawn` [2,POOL,3]"""
    rs = np.random.RandomState(SEED)
    p = dict(idx=rs.randint(0, HW, POOL).astype(np.int64), idx_per_image=rs.randint(0, HW, POOL).astype(np.int64))
    p["idx_per_image"][1::5] = p["idx_per_image"][0::5][:len(p["idx_per_image"][1::5])]        # repeated indices, whatever the draw
    e = rs.uniform(-0.9, 0.9, (2, POOL, 3))
    redrawn = np.zeros(e.shape, dtype=bool)
    for _ in range(100):
        # (1e-6 on top: pred - target of a case differs from e by the rounding of the sum, at most 2^-23)
        bad = np.abs(np.abs(e.astype(np.float32).astype(np.float64)) - DELTA) < KINK_MARGIN + 1e-6
        if not bad.any():
            break
        redrawn |= bad
        e[bad] = rs.uniform(-0.9, 0.9, int(bad.sum()))
    else:
        raise RuntimeError("kink margin not met")
    p.update(e=e.astype(np.float32), redrawn=redrawn)
    p["opacity"] = rs.uniform(0.02, 0.98, (2, POOL)).astype(np.float32)
    p["base"] = rs.uniform(1.2, 5.0, POOL).astype(np.float32)
    p["noise"] = (0.05 * rs.standard_normal((2, POOL))).astype(np.float32)
    return p


def pool_check():
    p = pools()
    return np.concatenate([p["idx"][:4].astype(np.float64), p["idx_per_image"][-4:].astype(np.float64), p["e"][1, -2].astype(np.float64),
                           p["opacity"][:, -1].astype(np.float64), p["base"][-2:].astype(np.float64), p["noise"][1, -3:].astype(np.float64),
                           [p["e"].astype(np.float64).sum(), p["noise"].astype(np.float64).sum()]]).astype(np.float32)


def depths(rows, P, head):
    """[rows] float32: per patch of P^2 rows a base + noise; every 7th patch exactly constant"""
    p, M = pools(), P * P
    patch = np.arange(rows) // M
    base = p["base"][patch]
    return np.where(patch % 7 == 0, base, base + p["noise"][head, :rows]).astype(np.float32)


def gather(per_pixel, ray_idx):
    """per_pixel [B,C,HW] -> [B,N,C] by ray_idx [N], [B,N] or None"""
    B = per_pixel.shape[0]
    if ray_idx is None:
        return np.transpose(per_pixel, (0, 2, 1))
    if ray_idx.ndim == 1:
        return np.transpose(per_pixel[:, :, ray_idx], (0, 2, 1))
    return np.stack([per_pixel[b][:, ray_idx[b]].T for b in range(B)])


def inputs(fx, name):
    """the float32 / bool / int64 numpy inputs of a case: dict(image [B,3,H,W], fg_mask [B,1,H,W] | None, ray_idx, rgb [B,N,3], rgb_fine,
    opacity [B,N,1], opacity_fine, depth [B,N,1], depth_fine, kind, patch, B, N)"""
    c, p = CASES[name], pools()
    B, N = c["B"], c["N"]
    rows = B * N
    views = list(c["views"])
    image, mask = fx["image"][views], fx["fg_mask"][views]
    ray_idx = dict(shared=p["idx"][:N], per_image=p["idx_per_image"][:rows].reshape(B, N), none=None)[c["form"]]
    target = gather(image.reshape(B, 3, HW), ray_idx)
    x = dict(image=image, fg_mask=mask if c["mask"] else None, ray_idx=ray_idx, kind=c["kind"], patch=c["patch"], B=B, N=N)
    x["rgb"] = (target + p["e"][0, :rows].reshape(B, N, 3)).astype(np.float32)
    x["rgb_fine"] = (target + p["e"][1, :rows].reshape(B, N, 3)).astype(np.float32) if c["fine"] else None
    for head, sfx in ((0, ""), (1, "_fine")):
        on = head == 0 or c["fine"]
        x["opacity" + sfx] = p["opacity"][head, :rows].reshape(B, N, 1) if c["mask"] and on else None
        x["depth" + sfx] = depths(rows, c["patch"], head).reshape(B, N, 1) if c["patch"] and on else None
    return x


# ---- the float64 values
def f64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).clone()


def colour_np(e, kind):
    a = np.abs(e)
    return e * e if kind == "mse" else np.where(a <= DELTA, 0.5 * e * e, DELTA * (a - 0.5 * DELTA))


def patch_np(d, P, c=CHARBONNIER):
    """sum over patches and all ordered pairs of sqrt((d_i - d_j)^2 + c^2), pair by pair"""
    M = P * P
    d = np.asarray(d, dtype=np.float64).reshape(-1, M)
    total = 0.0
    for i in range(M):
        for j in range(M):
            r = d[:, i] - d[:, j]
            total += float(np.sqrt(r * r + c * c).sum())
    return total


def want(x):
    """-> dict(out=[5] float64, seeds={tensor: float64 array: d (its own out[k]) / d tensor})"""
    B, N, kind, P = x["B"], x["N"], x["kind"], x["patch"]
    rows, hw = B * N, x["image"][0, 0].size
    target = gather(x["image"].reshape(B, 3, hw).astype(np.float64), x["ray_idx"])
    out = np.zeros(5)
    for head, key in enumerate(("rgb", "rgb_fine")):
        if x[key] is None:
            continue
        e = x[key].astype(np.float64) - target
        s = float(colour_np(e, kind).sum())
        out[0] += s / (3.0 * rows + 1e-6) if kind == "mse" else 2.0 * s / (3.0 * rows)
        out[3 + head] = float((e * e).sum()) / (3.0 * rows)
    if x["fg_mask"] is not None:
        fg = gather(x["fg_mask"].reshape(B, 1, hw).astype(np.float64), x["ray_idx"])
        for key in ("opacity", "opacity_fine"):
            if x[key] is not None:
                out[1] += 0.5 * float(np.abs(fg - x[key].astype(np.float64)).sum()) / rows
    if P:
        for key in ("depth", "depth_fine"):
            if x[key] is not None:
                out[2] += 0.02 * patch_np(x[key], P) / (rows * P * P)
    # the gradients: torch.float64 autograd on the same formulas
    seeds = {}
    tt = f64(target)
    for key in ("rgb", "rgb_fine"):
        if x[key] is None:
            continue
        t = f64(x[key]).requires_grad_()
        e = t - tt
        l = (e * e).sum() / (3.0 * rows + 1e-6) if kind == "mse" else 2.0 * torch.where(e.abs() <= DELTA, 0.5 * e * e, DELTA * (e.abs() - 0.5 * DELTA)).sum() / (3.0 * rows)
        seeds[key] = torch.autograd.grad(l, t)[0].numpy()
    if x["fg_mask"] is not None:
        fgt = f64(fg)
        for key in ("opacity", "opacity_fine"):
            if x[key] is not None:
                t = f64(x[key]).requires_grad_()
                seeds[key] = torch.autograd.grad(0.5 * (fgt - t).abs().sum() / rows, t)[0].numpy()
    if P:
        for key in ("depth", "depth_fine"):
            if x[key] is not None:
                t = f64(x[key]).requires_grad_()
                d = t.reshape(-1, P * P)
                r = d[:, :, None] - d[:, None, :]
                seeds[key] = torch.autograd.grad(0.02 * torch.sqrt(r * r + CHARBONNIER ** 2).sum() / (rows * P * P), t)[0].numpy()
    return dict(out=out, seeds=seeds)


def constant_rows(x):
    """the rows (flat) of the exactly constant patches of a case"""
    M = x["patch"] ** 2
    return (np.arange(x["B"] * x["N"]) // M) % 7 == 0


def kink_sides(x):
    """-> (side of the kink of every colour element in fp32, the same in float64, |e| in float64) over the heads that are there"""
    B = x["B"]
    t32 = gather(x["image"].reshape(B, 3, HW), x["ray_idx"])
    s32, s64, ab = [], [], []
    for key in ("rgb", "rgb_fine"):
        if x[key] is not None:
            e32 = x[key] - t32
            e64 = x[key].astype(np.float64) - t32.astype(np.float64)
            s32.append(np.abs(e32) <= np.float32(DELTA))
            s64.append(np.abs(e64) <= DELTA)
            ab.append(np.abs(e64))
    return np.stack(s32), np.stack(s64), np.stack(ab)


# ---- measures
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
