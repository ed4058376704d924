"""The correspondence loss of one view pair, timed three ways.

    python tools/corres_loss_bench.py [--out profiles/reproj_loss_bench.json] [--legs series term pair] [--blocks 5] [--iters 20] [--warmup 5]
                                      [--rows alone iteration] [--count-launches]

Legs.  `series`: the torch restatement of sparf_amd.losses under `losses.unfused()` -- the composition of the relative pose and the four
re-projection terms as the chain of small torch ops an unmodified trainer runs; the baseline, never the code under test.  `term`: the
composition in torch, then four `losses.reprojection_loss` calls (one launch each).  `pair`: one `losses.correspondence_pair_loss` call.
Rows.  `alone_<n>`: the loss forward + backward on fixed inputs, n = 1024 and 2048 matches (rand_rays // 2 of the 2048 / 4096 settings),
gradients to the four depth tensors and both poses.  `iteration_2048`: two 2048-pixel renders at 64 + 128 samples through ONE
`render_batch` in bf16x3, the loss on their depths (huber, both checks on), backward to both poses and both networks.
The legs of a row run in the alternating blocks of tools/paired_bench.py, of `--iters` iterations; per leg ms per iteration as median
and min ... max over the blocks, and `pair` over `series` with whether their blocks overlap.
`--count-launches` (a run of its own) traces ONE loss-alone iteration of each leg after the warm-up (paired_bench's profiler pass) and
reports the kernels, copies and memsets it launched; it times nothing.
One JSON document on stdout and, with --out, in that file."""
import os
import sys

import torch

import paired_bench as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_workloads import SHAPES, cameras, config_opt      # noqa: E402
from sparf_amd import losses                                  # noqa: E402
from sparf_amd.renderer import Graph                          # noqa: E402

LEGS = ("series", "term", "pair")
OPTS = dict(loss_type="huber", pixel_thresh=10.0, depth_thresh=0.1)


def pair_loss(leg, ps, po, d, K, Ps, Po, conf):
    """d = (depth_self, depth_other, depth_fine_self, depth_fine_other)"""
    if leg == "series":
        with losses.unfused():
            return losses.correspondence_pair_loss(ps, po, d[0], d[1], K[0], K[1], Ps, Po, conf, d[2], d[3], **OPTS)[0]
    if leg == "pair":
        return losses.correspondence_pair_loss(ps, po, d[0], d[1], K[0], K[1], Ps, Po, conf, d[2], d[3], **OPTS)[0]
    T = losses._to_4x4(Po) @ losses.pose_inverse_4x4_torch(losses._to_4x4(Ps))
    Ti = losses.pose_inverse_4x4_torch(T)
    loss = 0
    for a, b in ((d[0], d[1]), (d[2], d[3])):
        loss = loss + losses.reprojection_loss(ps, a, K[0], po, b, K[1], T, conf, **OPTS)[0]
        loss = loss + losses.reprojection_loss(po, b, K[1], ps, a, K[0], Ti, conf, **OPTS)[0]
    return loss / 4.0


def matches(n, H, W, f, device, seed):
    """n matches of a two-view scene: integer pixels in self, depths in [1.5, 5], the projection in other plus noise (0.3 px for half,
    6 px for the rest), depth_other = the projected depth x (1 + 0.08 N), fine depths 2 % off the coarse ones; poses 0.2 rad / 0.4 apart"""
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=torch.float64)
    c, s = torch.cos(torch.tensor(0.2, dtype=torch.float64)), torch.sin(torch.tensor(0.2, dtype=torch.float64))
    Ps = torch.eye(4, dtype=torch.float64)[:3]
    Po = torch.tensor([[c, 0, -s, 0.4], [0, 1, 0, -0.05], [s, 0, c, 0.1]], dtype=torch.float64)
    ps = torch.stack([torch.randint(0, W, (n,), generator=g), torch.randint(0, H, (n,), generator=g)], 1).double()
    ds = torch.rand(n, generator=g, dtype=torch.float64) * 3.5 + 1.5
    X = (torch.cat([ps, torch.ones(n, 1, dtype=torch.float64)], 1) @ torch.linalg.inv(K).T) * ds[:, None]
    Xo = X @ Po[:, :3].T + Po[:, 3]
    y = Xo @ K.T
    sigma = torch.where(torch.rand(n, 1, generator=g) < 0.5, 0.3, 6.0)
    po = y[:, :2] / y[:, 2:] + torch.randn(n, 2, generator=g, dtype=torch.float64) * sigma
    do = Xo[:, 2] * (1 + 0.08 * torch.randn(n, generator=g, dtype=torch.float64))
    fine = [x * (1 + 0.02 * torch.randn(n, generator=g, dtype=torch.float64)) for x in (ds, do)]
    t = lambda x: x.float().to(device)
    return dict(ps=t(ps).long(), po=t(po), d=[t(ds), t(do), t(fine[0]), t(fine[1])], K=(t(K), t(K)), Ps=t(Ps), Po=t(Po),
                conf=t(torch.rand(n, 1, generator=g) * 0.5 + 0.5))


class Alone:
    """the loss forward + backward on fixed inputs"""

    def __init__(self, leg, n, device):
        self.leg = leg
        m = matches(n, 378, 504, 500.0, device, seed=n)
        self.m = m
        self.leaves = [x.requires_grad_() for x in m["d"]] + [m["Ps"].requires_grad_(), m["Po"].requires_grad_()]

    def iteration(self):
        for x in self.leaves:
            x.grad = None
        m = self.m
        loss = pair_loss(self.leg, m["ps"], m["po"], m["d"], m["K"], m["Ps"], m["Po"], m["conf"])
        loss.backward()
        return loss


class Iteration:
    """two pixel-list renders through one render_batch, the loss on their depths, backward to both poses and both networks"""

    def __init__(self, leg, n, device, precision="bf16x3"):
        self.leg, s = leg, SHAPES[2]
        self.opt = config_opt(2, precision, rays=2 * n)
        torch.manual_seed(0)
        self.graph = Graph(self.opt, device)
        self.graph.train()
        for net in (self.graph.nerf, self.graph.nerf_fine):
            net.progress.data.fill_(1.0)
        self.H, self.W, self.rng = s["H"], s["W"], list(s["rng"])
        pose, intr = cameras(2, device)
        rel = matches(1, self.H, self.W, s["f"], device, seed=0)["Po"]             # the second view: 0.2 rad / 0.4 units from the first
        other = torch.cat([rel[:, :3] @ pose[0, :, :3], rel[:, :3] @ pose[0, :, 3:] + rel[:, 3:]], dim=-1)
        self.pose = torch.stack([pose[0], other]).requires_grad_()
        self.intr = intr[:2]
        g = torch.Generator().manual_seed(1)
        self.ps = torch.stack([torch.randint(0, self.W, (n,), generator=g), torch.randint(0, self.H, (n,), generator=g)], 1).to(device)
        self.po = (self.ps.float() + torch.randn(n, 2, generator=g).to(device) * 3).clamp_min(0)
        self.conf = (torch.rand(n, 1, generator=g) * 0.5 + 0.5).to(device)

    def iteration(self):
        self.graph.zero_grad(set_to_none=True)
        self.pose.grad = None
        reqs = [dict(pose=self.pose[i:i + 1], H=self.H, W=self.W, intr=self.intr[i:i + 1], pixels=px, depth_range=self.rng, mode="train")
                for i, px in enumerate((self.ps.float(), self.po))]
        a, b = self.graph.render_batch(self.opt, reqs, iter=0)
        loss = pair_loss(self.leg, self.ps, self.po, (a.depth, b.depth, a.depth_fine, b.depth_fine), (self.intr[0], self.intr[1]), self.pose[0],
                         self.pose[1], self.conf)
        loss.backward()
        return loss


def measure(works, blocks, iters, warmup):
    ms = pb.device_ms(works, blocks, iters, warmup)
    out = {k: pb.flat(t) for k, t in ms.items()}
    out["loss"] = {k: float(w.iteration().detach()) for k, w in works.items()}
    if "series" in ms and "pair" in ms:
        ratio, less, overlap = pb.versus(ms["series"], ms["pair"])
        out.update(pair_over_series=ratio, pair_and_series_blocks_overlap=overlap, series_minus_pair_ms=less)
    return out


def count_launches(device, legs, n, warmup):
    """-> per leg the device activities of ONE loss-alone iteration (forward + backward) after the warm-up (paired_bench.traced):
    kernels, memory copies and memsets, with the kernels' names"""
    works = {leg: Alone(leg, n, device) for leg in legs}
    for w in works.values():
        pb.device_block(w, warmup)
    out = {}
    for leg, w in works.items():
        t = pb.traced(w.iteration)
        out[leg] = dict(kernels=len(t.kernels), copies_and_memsets=len(t.copies), by_name=t.by_name)
    return out


def main():
    ap = pb.parser(__doc__)
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=LEGS)
    ap.add_argument("--rows", nargs="+", default=["alone", "iteration"], choices=["alone", "iteration"])
    ap.add_argument("--count-launches", action="store_true")
    a = ap.parse_args()
    device = pb.gpu_or_exit("tools/corres_loss_bench.py")
    if a.count_launches:
        doc = dict(tool="tools/corres_loss_bench.py --count-launches", device=torch.cuda.get_device_name(0), matches=1024,
                   launches_per_iteration=count_launches(device, a.legs, 1024, a.warmup))
        return pb.emit(doc, a.out)
    rows = {}
    if "alone" in a.rows:
        for n in (1024, 2048):
            rows[f"alone_{n}"] = measure({leg: Alone(leg, n, device) for leg in a.legs}, a.blocks, a.iters, a.warmup)
    if "iteration" in a.rows:
        rows["iteration_2048"] = measure({leg: Iteration(leg, 2048, device) for leg in a.legs}, a.blocks, a.iters, a.warmup)
    doc = dict(tool="tools/corres_loss_bench.py", label=a.label, device=torch.cuda.get_device_name(0),
               workload="correspondence loss of one view pair, huber with both checks, four terms; alone_<n>: loss forward + backward on fixed "
                        "inputs; iteration_2048: two 2048-pixel renders x (64 + 128) through render_batch in bf16x3, loss, backward",
               blocks=a.blocks, iters_per_block=a.iters, warmup_iters=a.warmup, legs=a.legs, rows=rows)
    pb.emit(doc, a.out)


if __name__ == "__main__":
    main()
