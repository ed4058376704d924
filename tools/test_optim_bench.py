"""Test-time photometric pose optimisation, timed: the full route against ray-gradient-only passes (opt.hip.test_optim_rays_only).

    python tools/test_optim_bench.py [--out profiles/rays_only_test_optim.json] [--precisions bf16x3 fp32] [--blocks 5] [--iters 20] [--warmup 5]

The loop is the reference's (joint_pose_nerf_trainer.py:381-406): per test view, Adam on a zero-initialised 6-vector composed with the
view's initial pose, 4096 random rays x (64 + 128) samples of a DTU-shaped 300 x 400 view per iteration, render in mode "test-optim",
photometric loss on both networks' colours, backward, Adam step.  The networks stay trainable, as in the unmodified loop; the option
alone selects the route, so BOTH routes run in ONE process, in the alternating blocks of tools/paired_bench.py, of `--iters` iterations.
Per route and precision: ms per iteration (render + backward + Adam step) as median and spread (min ... max) over the blocks, and the
peak allocated bytes of the route's blocks.
On a tree without the option (an older commit) only the full route runs: the same numbers, comparable between commits.
One JSON document on stdout and, with --out, in that file."""
import os
import sys

import torch

import paired_bench as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_workloads import SHAPES, analytic_images, cameras, compose, config_opt, se3_exp      # noqa: E402
from sparf_amd import lib as L                                                                   # noqa: E402
from sparf_amd.renderer import Graph                                                             # noqa: E402

HAS_ROUTE = hasattr(L, "SAVE_MASKS")


class View:
    """one test view: a trained-scene stand-in (seeded networks), the view's target image and the loop state of one route"""

    def __init__(self, precision, rays_only, device, rays=4096, seed=0):
        self.opt = config_opt(2, precision, rays=rays)                 # joint_pose_nerf_training/dtu/barf.py: 64 + 128 samples, BARF c2f
        self.opt.hip.test_optim_rays_only = bool(rays_only)
        torch.manual_seed(seed)
        self.graph = Graph(self.opt, device)
        for net in (self.graph.nerf, self.graph.nerf_fine):
            net.progress.data.fill_(1.0)                               # after training: every band open
        s = SHAPES[2]
        self.H, self.W = s["H"], s["W"]
        pose, intr = cameras(2, device)
        self.pose0, self.intr = pose[:1], intr[:1]
        self.image = analytic_images(self.pose0, self.intr, self.H, self.W).flatten(2).permute(0, 2, 1).contiguous()      # [1, H*W, 3]
        self.depth_range = list(s["rng"])
        self.rays = rays
        self.gen = torch.Generator(device="cpu").manual_seed(seed + 1)
        self.reset()

    def reset(self):
        self.xi = torch.zeros(1, 6, device=self.pose0.device, requires_grad=True)
        self.optim = torch.optim.Adam([self.xi], lr=1e-3)

    def iteration(self):
        idx = torch.randperm(self.H * self.W, generator=self.gen)[:self.rays].to(self.pose0.device)
        self.optim.zero_grad()
        pose = compose(se3_exp(self.xi), self.pose0)
        ret = self.graph.render(self.opt, pose, H=self.H, W=self.W, intr=self.intr, ray_idx=idx, depth_range=self.depth_range, iter=None, mode="test-optim")
        tgt = self.image[:, idx]
        loss = ((ret.rgb - tgt) ** 2).mean() + ((ret.rgb_fine - tgt) ** 2).mean()
        loss.backward()
        self.optim.step()
        return loss


def block_with_peak(view, iters):
    """paired_bench.device_block -> (ms per iteration, peak allocated bytes) of `iters` iterations"""
    torch.cuda.reset_peak_memory_stats()
    ms, _ = pb.device_block(view, iters)
    return ms, torch.cuda.max_memory_allocated()


def measure(precision, device, blocks, iters, warmup):
    routes = {"full": View(precision, False, device)}
    if HAS_ROUTE:
        routes["rays_only"] = View(precision, True, device)
    timed = pb.alternate(routes, blocks, iters, warmup, block=block_with_peak)
    ms = {k: [t for t, _ in v] for k, v in timed.items()}
    out = {}
    for k in routes:
        out[k] = dict(pb.flat(ms[k]), peak_allocated_bytes=max(p for _, p in timed[k]),
                      network_grads_populated=all(p.grad is not None for p in routes[k].graph.nerf.hip_params()))
    if HAS_ROUTE:
        out["rays_only_over_full"] = pb.versus(ms["full"], ms["rays_only"])[0]
    return out


def main():
    ap = pb.parser(__doc__)
    ap.add_argument("--precisions", nargs="+", default=["bf16x3", "fp32"])
    a = ap.parse_args()
    device = pb.gpu_or_exit("tools/test_optim_bench.py")
    doc = dict(tool="tools/test_optim_bench.py", label=a.label, device=torch.cuda.get_device_name(0), workload="one DTU-shaped test view, 4096 rays x (64 + 128), "
               "Adam on a 6-vector, mode test-optim", blocks=a.blocks, iters_per_block=a.iters, warmup_iters=a.warmup, has_rays_only_route=HAS_ROUTE,
               precisions={p: measure(p, device, a.blocks, a.iters, a.warmup) for p in a.precisions})
    pb.emit(doc, a.out)


if __name__ == "__main__":
    main()
