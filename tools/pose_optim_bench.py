"""Test-time photometric pose optimisation, timed with the pose chain three ways.

    python tools/pose_optim_bench.py [--pose closed series fused] [--out profiles/pose_fused_test_optim.json] [--precisions bf16x3 fp32]
                                     [--blocks 5] [--iters 20] [--warmup 5]

The loop, the view and the two routes (`full`, `rays_only` = opt.hip.test_optim_rays_only) are those of tools/test_optim_bench.py, whose
`View` this tool subclasses; what changes is how the 6-vector becomes the pose.  `closed`: the closed-form twist exponential of
bench_workloads.se3_exp, i.e. exactly what tools/test_optim_bench.py runs.  `series`: the reference's own chain, camera.lie.se3_to_SE3
(truncated series) then camera.pose.compose, as the torch restatement of sparf_amd.camera -- what an unmodified trainer runs.  `fused`:
sparf_amd.camera.refine_se3, one launch each way.  Every (route, pose) pair runs in the alternating blocks of tools/paired_bench.py, of
`--iters` iterations, keyed "<route>" for closed and "<route>+<pose>" otherwise; per pair ms per iteration as median and
min ... max over the blocks, and per route `fused` over `series` with whether their blocks overlap.
One JSON document on stdout and, with --out, in that file."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import paired_bench as pb                                     # noqa: E402
from bench_workloads import compose, se3_exp                  # noqa: E402
from sparf_amd import camera                                  # noqa: E402
from test_optim_bench import HAS_ROUTE, View                  # noqa: E402

POSES = ("closed", "series", "fused")


class PoseView(View):
    def __init__(self, precision, rays_only, device, pose_mode):
        self.pose_mode = pose_mode
        super().__init__(precision, rays_only, device)

    def pose(self):
        if self.pose_mode == "fused":
            return camera.refine_se3(self.xi, self.pose0)
        if self.pose_mode == "series":
            with camera.unfused():
                return camera.pose.compose([camera.lie.se3_to_SE3(self.xi), self.pose0])
        return compose(se3_exp(self.xi), self.pose0)

    def iteration(self):                                       # View.iteration with the pose from self.pose()
        idx = torch.randperm(self.H * self.W, generator=self.gen)[:self.rays].to(self.pose0.device)
        self.optim.zero_grad()
        ret = self.graph.render(self.opt, self.pose(), H=self.H, W=self.W, intr=self.intr, ray_idx=idx, depth_range=self.depth_range, iter=None,
                                mode="test-optim")
        tgt = self.image[:, idx]
        loss = ((ret.rgb - tgt) ** 2).mean() + ((ret.rgb_fine - tgt) ** 2).mean()
        loss.backward()
        self.optim.step()
        return loss


def measure(precision, device, blocks, iters, warmup, poses):
    views = {}
    for route, rays_only in (("full", False),) + ((("rays_only", True),) if HAS_ROUTE else ()):
        for pm in poses:
            views[route if pm == "closed" else route + "+" + pm] = PoseView(precision, rays_only, device, pm)
    ms = pb.device_ms(views, blocks, iters, warmup)
    out = {k: pb.flat(t) for k, t in ms.items()}
    for route in ("full", "rays_only"):
        if route + "+series" in ms and route + "+fused" in ms:
            out[route + "_fused_over_series"], _, out[route + "_fused_and_series_blocks_overlap"] = pb.versus(ms[route + "+series"], ms[route + "+fused"])
    return out


def main():
    ap = pb.parser(__doc__)
    ap.add_argument("--pose", nargs="+", default=list(POSES), choices=POSES)
    ap.add_argument("--precisions", nargs="+", default=["bf16x3", "fp32"])
    a = ap.parse_args()
    device = pb.gpu_or_exit("tools/pose_optim_bench.py")
    doc = dict(tool="tools/pose_optim_bench.py", label=a.label, device=torch.cuda.get_device_name(0), workload="one DTU-shaped test view, 4096 rays x (64 + 128), "
               "Adam on a 6-vector, mode test-optim", blocks=a.blocks, iters_per_block=a.iters, warmup_iters=a.warmup, pose=a.pose,
               precisions={p: measure(p, device, a.blocks, a.iters, a.warmup, tuple(a.pose)) for p in a.precisions})
    pb.emit(doc, a.out)


if __name__ == "__main__":
    main()
