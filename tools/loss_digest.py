"""SHA-256 digests of every output tensor of the six loss units that share csrc/ordered.h (reproj, dcons, photo, matches, colmap,
depth_err), at the sizes either side of each unit's one-launch limit, for the seeded inputs of the referee modules in tests/ -- run it under two
$SPARF_LIB builds to show that a change to the ordered compaction or the fixed-order sums is bit-neutral.

    python tools/loss_digest.py ;  SPARF_LIB=sparf_amd/libsparf_hip_base.so python tools/loss_digest.py
One line per entry point and size: `unit entry size  name:digest ...`.  The calls are those of the GPU tests (their run helpers)."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat")]
from sparf_amd import losses, ops                                                    # noqa: E402
from tests import colmap_referee, dcons_referee, depth_err_referee, matches_referee, photo_referee, reproj_referee   # noqa: E402
from tests import test_colmap_gpu, test_dcons_gpu, test_depth_err_gpu, test_matches_gpu, test_photo_gpu, test_reproj_gpu      # noqa: E402


def digest(t):
    a = t.detach().contiguous().cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()[:16]


def line(unit, entry, size, items):
    print(unit, entry, size, " " + " ".join(f"{k}:{digest(v)}" for k, v in items), flush=True)


def reproj():
    R, T = reproj_referee, test_reproj_gpu
    fx = R.fixture()
    case = R.PAIR_CASES[-1]
    for n in (4096, 4097):
        line("reproj", "term", n, sorted(T.run_term(*R.term_case(fx, n, case)).items()))
        # the pair fixture ends at 1025 matches: its rows repeated up to n (the poses and intrinsics stay)
        inp, opts = R.pair_case(fx, 1025, 1, case)
        inp = {k: np.resize(v, (n,) + v.shape[1:]) if v.shape[0] == 1025 else v for k, v in inp.items()}
        line("reproj", "pair_fine", n, sorted(T.run_pair(inp, opts).items()))


def dcons():
    R, T = dcons_referee, test_dcons_gpu
    fx = R.fixture()
    for n in (257, 4096, 4097, 8200):
        line("dcons", "project", n, sorted(T.run_project(fx, px=fx["px"][:n], d=fx["d"][:n]).items()))
        out = losses.visibility_select(T.D(R.vis(n)), T.D(fx["uv"][:n], True), T.D(fx["z"][:n], True))
        line("dcons", "select", n, list(zip(("uv", "z", "vis", "index"), out)) + [("dst", out[0].grad_fn.saved_tensors[0])])
        line("dcons", "loss", n, sorted(T.run_loss(R.loss_inputs(fx, n, 1), "huber").items()))


def photo():
    R, T = photo_referee, test_photo_gpu
    fx = R.fixture()
    for name in ("all256_huber", "all4100_huber", "p3_4104"):
        out, seeds, _ = T.run(R.inputs(fx, name))
        line("photo", "loss", name, [("out", out)] + sorted(seeds.items()))


def matches():
    R, T = matches_referee, test_matches_gpu
    for H, W in ((64, 65), (96, 128)):
        corres, conf = R.maps_of(H, W)
        win = R.window_of(H, W, "precrop")
        for pattern in R.PATTERNS:
            mask = R.mask_of(H, W, pattern)
            perm = R.perm_of(int(R.window_mask(mask, win).sum()))
            index, count, _ = ops.match_compact(T.D(mask), win, want_perc=False)
            out = losses.select_matches(T.D(mask), T.D(corres), T.D(conf), R.MAX_MATCHES, window=win, perm=T.D(perm))
            items = [("index", index[:int(count.item())]), ("count", count)] + list(zip(T.RESULTS, out[:5])) + [("perc", out[6])]
            line("matches", "compact+gather", f"{H}x{W}_{pattern}", items)


def colmap():
    R, T = colmap_referee, test_colmap_gpu
    H, W = 65, 67
    depth, conf = R.maps_of(H, W)
    valid = R.select_np(depth, conf, R.RAND_RAYS, [np.arange(H * W)] * R.B)["valid"]
    g = np.random.RandomState(W)
    perms = [g.permutation(v) for v in valid]
    d, c = T.D(depth), T.D(conf)
    index, count = ops.colmap_compact(d)
    rays, target, weight, _, _ = losses.sparse_depth_select(d, c, R.RAND_RAYS, perms=[T.D(p) for p in perms])
    items = [(f"index{b}", index[b, :valid[b]]) for b in range(R.B)] + [("count", count)] + [(f"rays{b}", r) for b, r in enumerate(rays)]
    line("colmap", "compact+gather", f"{H}x{W}", items + [("target", target), ("weight", weight)])
    rows = [1500, 1499, 1101]
    t, w, p, pf, _ = T._loss_case(rows, True, 7 + len(rows), False)
    loss = losses.sparse_depth_loss(t, w, rows, p, pf)
    grads = torch.autograd.grad(loss, p + pf)
    line("colmap", "loss_fine", "+".join(map(str, rows)), [("loss", loss)] + [(f"seed{i}", x) for i, x in enumerate(grads)])


def depth_err():
    R, T = depth_err_referee, test_depth_err_gpu
    cases = [("per_image", R.build("per_image"))] + [("x".join(map(str, shape)), R.build_edge(*shape)) for shape in R.EDGE_SHAPES]      # 4096, 4097, 8710 rows
    for size, case in cases:
        for scale in R.SCALES:
            for fine in (True, False):
                vector, count, _ = T.run(case, scale, fine)
                line("depth_err", "fine" if fine else "coarse", f"{size}_s{scale}", [("vector", vector), ("count", count)])


if __name__ == "__main__":
    print("library:", os.environ.get("SPARF_LIB", "default"), flush=True)
    for unit in (reproj, dcons, photo, matches, colmap, depth_err):
        unit()
    torch.cuda.synchronize()
