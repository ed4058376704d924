"""numpy / float64 referee of the DS-NeRF sparse depth loss (base_losses.py:326-402): the case recipes, the selection
(integer and copy work: bit for bit), the loss in float64 and its closed-form gradient seeds.  Nothing here imports torch or the
package; tests/test_colmap_cpu.py and tests/test_colmap_gpu.py hold the package to it, tests/golden/make_colmap_golden.py records
what the reference's own method did on the same cases (tests/golden/colmap.npz)."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colmap.npz")
B, RAND_RAYS = 4, 128
QUOTA = RAND_RAYS // B
SHAPES = ((65, 67), (16, 16), (64, 64))          # two chunks with a 259-pixel tail; one tile; exactly 4096, the last one-launch size
SEEDS = (11, 12)
# 65 x 67, from the recipes below: image 0 draws, image 1 sits exactly at the quota (no draw), image 2 is skipped, image 3 holds values
# between the two thresholds, a negative one, and the first and the last pixel
VALID_65x67, POSITIVE_65x67 = (1452, 32, 0, 2), (1452, 32, 0, 2178)
PERC_65x67 = 3662 / 17420


def case_name(H, W):
    return f"{H}x{W}"


def maps_of(H, W):
    """-> (colmap_depth [B,1,H,W] float32, colmap_conf [B,1,H,W] float32) of the recipes, on the H W pixels p = h W + w"""
    n = H * W
    p = np.arange(n)
    depth = np.zeros((B, n), dtype=np.float64)
    depth[0] = np.where(p % 3 == 0, 2 + 0.001 * (p % 97), 0.0)
    depth[1] = np.where(p % 137 == 1, 3 + 0.002 * (p % 53), 0.0)
    depth[3] = np.where(p % 2 == 0, 5e-7, 0.0)
    depth[3, 0], depth[3, n - 1], depth[3, 7] = 1.5, 2.5, -1.0
    conf = np.tile(0.25 + 0.5 * ((7 * p + 3) % 11) / 11, (B, 1))
    return depth.astype(np.float32).reshape(B, 1, H, W), conf.astype(np.float32).reshape(B, 1, H, W)


def select_np(depth, conf, rand_rays, perms=None):
    """base_losses.py:363-386: perms[b] = the permutation image b draws (read where its count is ABOVE the quota).
    -> dict(rays: list of int64 arrays, target, weight: packed float32, valid, positive, rows: lists of ints, perc)"""
    nb = depth.shape[0]
    d, c = depth.reshape(nb, -1), conf.reshape(nb, -1)
    quota = rand_rays // nb
    rays, valid, positive = [], [], []
    for b in range(nb):
        idx = np.nonzero(d[b] > np.float32(1e-6))[0].astype(np.int64)
        valid.append(len(idx))
        positive.append(int((d[b] > 0).sum()))
        if len(idx) > quota:
            idx = idx[np.asarray(perms[b])[:quota]]
        rays.append(idx)
    return dict(rays=rays, target=np.concatenate([d[b][r] for b, r in enumerate(rays)]), weight=np.concatenate([c[b][r] for b, r in enumerate(rays)]),
                valid=valid, positive=positive, rows=[len(r) for r in rays], perc=sum(positive) / d.size)


def rendered_np(b, rays, fine=False):
    """the stand-in render of tests/colmap_fake.DepthNet: multiples of 1/128, exact in float32"""
    return (2.0 + 0.25 * b + ((np.asarray(rays) * 37) % 101) / 128.0 + (0.0625 if fine else 0.0)).astype(np.float32)


def loss_np(target, weight, rows, depth, depth_fine=None, batch_size=None):
    """base_losses.py:391-400 in float64 on the packed float32 rows -> (loss, d loss / d depth, d loss / d depth_fine or None), float64"""
    nb = len(rows) if batch_size is None else batch_size
    t, w, p = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (target, weight, depth))
    pf = np.asarray(depth_fine, dtype=np.float64).reshape(-1) if depth_fine is not None else None
    k = np.repeat(np.asarray(rows, dtype=np.float64), rows)
    total = 0.0
    off = 0
    for r in rows:
        if r:
            s = slice(off, off + r)
            total += float(np.sum(w[s] * (t[s] - p[s]) ** 2)) / r
            if pf is not None:
                total += float(np.sum(w[s] * (t[s] - pf[s]) ** 2)) / r
        off += r
    seed = lambda q: (0.1 / nb) * (2.0 / k) * w * (q - t)
    return 0.1 * total / nb, seed(p), seed(pf) if pf is not None else None


def spacing(x):
    """the fp32 spacing at |x| (of the smallest normal below it)"""
    return float(np.spacing(np.float32(max(abs(float(x)), float(np.finfo(np.float32).tiny)))))


def within_spacings(got, want, n):
    """every |got - want| <= n fp32 spacings at |want|"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    tol = n * np.array([spacing(x) for x in want]) if want.size else np.zeros(0)
    return bool(np.all(np.abs(got - want) <= tol))


def fixture():
    return np.load(FIXTURE)
