"""numpy / float64 referee of the depth errors on rendered rays (metrics.py:81-134) and the case builder.  The
referee is csrc/depth_err.h in numpy: exact on the stored float32 operands, e = gt - pred s in float64 with s = float32(scale), the sums
by math.fsum (exactly rounded), one division and one square root.  Nothing here imports torch or the package;
tests/test_depth_err_cpu.py and tests/test_depth_err_gpu.py hold the package to it, tests/golden/make_depth_err_golden.py records what the
reference's own function did on the fixture cases (tests/golden/depth_err.npz)."""
import math
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_err.npz")
B_MAPS, H, W = 3, 16, 20
HW = H * W
N = 37
SCALES = (1.0, 1.7)
# name -> (idx_img_rendered, kind of ray_idx)
FIXTURE_CASES = {
    "list": ([0, 1, 2], "list"),             # one list of N = 37 rays with repeats for all images
    "per_image": ([0, 1, 2], "per_image"),   # [B,N]
    "full": ([0, 1, 2], None),               # no ray_idx: full images
    "subset": ([2, 0], "list"),              # idx_img_rendered = [2, 0]
    "hole": ([0, 1, 2], "hole"),             # [B,N]; the rays of image 1 meet no valid pixel of map 1
    "empty": ([1], "hole1"),                 # map 1 alone under those rays: no valid pixel at all
}
# full images with B = 1 around the one-launch limit of 4096 rows, and B = 2 over three chunks with a partial last one
EDGE_SHAPES = ((1, 64, 64), (1, 17, 241), (2, 65, 67))


def case_names():
    return [f"{name}/s{scale}" for name in FIXTURE_CASES for scale in SCALES]


def maps_of(b_maps=B_MAPS, h=H, w=W):
    """-> (depth_gt [b_maps,1,h,w] float32, valid [b_maps,1,h,w] bool): map 1 is invalid on every pixel p with p % 5 < 2"""
    n = h * w
    p = np.arange(n)
    depth = np.stack([1.5 + 0.37 * m + 0.003 * ((p * 7 + 3 * m) % 211) + 0.11 * np.sin(0.05 * p + m) for m in range(b_maps)])
    valid = np.stack([(p * 11 + m) % 7 != 0 for m in range(b_maps)])
    if b_maps > 1:
        valid[1] &= p % 5 >= 2
    return depth.astype(np.float32).reshape(b_maps, 1, h, w), valid.reshape(b_maps, 1, h, w)


def rays_of(kind, B, n=N, hw=HW):
    """-> ray_idx int64 [n] ('list', with repeats), [B,n] ('per_image'; 'hole': row 1 on invalid pixels of map 1; 'hole1': that row alone) or None"""
    if kind is None:
        return None
    j = np.arange(n, dtype=np.int64)
    if kind == "list":
        r = (j * 53 + 7) % hw
        r[5], r[20], r[36] = r[4], r[4], r[0]
        return r
    per = np.stack([(j * (41 + 6 * b) + 13 * b) % hw for b in range(max(B, 2))])
    if kind == "per_image":
        return per[:B]
    invalid = 5 * ((j * 9) % (hw // 5)) + (j % 2)            # p % 5 < 2
    if kind == "hole1":
        return invalid[None]
    per[1] = invalid
    return per[:B]


def rendered_of(B, n, fine=False):
    """the rendered depth [B,n,1] float32 of a head: near the maps' range, no exact float32 pattern"""
    r = np.arange(B * n, dtype=np.float64)
    d = 1.7 + 0.45 * np.cos(0.37 * r) + 0.002 * (r % 89) + (0.031 * np.sin(0.11 * r) + 0.02 if fine else 0.0)
    return d.astype(np.float32).reshape(B, n, 1)


def build(name):
    """-> dict(depth_gt, valid, idx, ray_idx (or None), depth, depth_fine) of a fixture case"""
    idx, kind = FIXTURE_CASES[name]
    depth_gt, valid = maps_of()
    ray_idx = rays_of(kind, len(idx))
    n = HW if ray_idx is None else ray_idx.shape[-1]
    return dict(depth_gt=depth_gt, valid=valid, idx=np.array(idx, dtype=np.int64), ray_idx=ray_idx, depth=rendered_of(len(idx), n),
                depth_fine=rendered_of(len(idx), n, fine=True))


def build_edge(B, h, w):
    """full images (no ray_idx, no index: the first B of B + 1 maps) of h x w pixels"""
    depth_gt, valid = maps_of(B + 1, h, w)
    return dict(depth_gt=depth_gt, valid=valid, idx=None, ray_idx=None, depth=rendered_of(B, h * w), depth_fine=rendered_of(B, h * w, fine=True))


def gathered(depth_gt, valid, idx, ray_idx, B, n):
    """section 1 of the issue, the source position of every row -> (gt [B,n] float32, kept [B,n] bool); indices are clamped"""
    b_maps = depth_gt.shape[0]
    gt, va = depth_gt.reshape(b_maps, -1), (valid.reshape(b_maps, -1) if valid is not None else np.ones((b_maps, depth_gt[0].size), dtype=bool))
    hw = gt.shape[1]
    m = np.clip(np.arange(B) if idx is None else np.asarray(idx), 0, b_maps - 1)
    if ray_idx is None:
        p = np.tile(np.arange(n), (B, 1))
    else:
        p = np.asarray(ray_idx) if np.ndim(ray_idx) == 2 else np.tile(np.asarray(ray_idx), (B, 1))
    p = np.clip(p, 0, hw - 1)
    return gt[m[:, None], p], va[m[:, None], p] != 0


def errors(gt, kept, pred, scale):
    """-> (abs_e, rmse, K) in float64 for one head: pred [B,n(,1)] float32"""
    s = np.float64(np.float32(scale))
    e = (gt.astype(np.float64) - pred.reshape(gt.shape).astype(np.float64) * s)[kept]
    K = int(kept.sum())
    abs_e = math.fsum(np.abs(e)) / (K + 1e-6)
    rmse = math.sqrt(math.fsum(e * e) / K) if K else float("nan")
    return abs_e, rmse, K


def referee(case, scale, fine=True):
    """-> (vector [4] float64: abs_e, rmse, abs_e_fine, rmse_fine (0 without a fine head), K)"""
    B, n = case["depth"].shape[:2]
    gt, kept = gathered(case["depth_gt"], case["valid"], case["idx"], case["ray_idx"], B, n)
    a, r, K = errors(gt, kept, case["depth"], scale)
    af, rf = errors(gt, kept, case["depth_fine"], scale)[:2] if fine else (0.0, 0.0)
    return np.array([a, r, af, rf], dtype=np.float64), K


def spacing(x):
    """the fp32 spacing at |x| (of the smallest normal below it)"""
    return float(np.spacing(np.float32(max(abs(float(x)), float(np.finfo(np.float32).tiny)))))


def distance(got, want):
    """|got - want| in fp32 spacings at |want|; 0 where both are NaN, inf where one is"""
    got, want = float(got), float(want)
    if math.isnan(got) or math.isnan(want):
        return 0.0 if math.isnan(got) and math.isnan(want) else float("inf")
    return abs(got - want) / spacing(want)


def fixture():
    return np.load(FIXTURE)
