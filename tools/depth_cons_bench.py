"""The depth-consistency loss, timed as torch ops and as the three library calls.

    python tools/depth_cons_bench.py [--out profiles/dcons_loss_bench.json] [--blocks 5] [--iters 20] [--warmup 5] [--rows chain whole]
                                     [--count-launches]

Legs.  `series`: everything under `losses.unfused()` -- the torch restatement of depth_cons_loss.py:209, :247-259, :277-283 and :293-312,
the chain of small torch ops with its two boolean-index selections that an unmodified trainer runs; the baseline, never the code under
test.  `fused`: `losses.depth_consistency_project` (back-projecting form), `visibility_select`, `depth_consistency_loss`.
Rows.  `chain_<n>`: the three ops and their backward at n = 1024 and 2048 pixels, with synthetic visibility and rendered depths (fixed
per source pixel, gathered through the ops' index; the rendered depth also depends weakly on the pixel, so the backward reaches the
projection as it does behind a render), gradient to depth_ref.  `whole_2048`: a 2048-pixel render of the reference view at 64 + 128
samples in bf16x3, project, `render_to_max` under no_grad, select, the render at the kept pixels, the loss, backward to both networks.
Both legs of a row run in the alternating blocks of tools/paired_bench.py, of `--iters` iterations; per leg ms per iteration as median
and min ... max over the blocks, `fused` over `series`, and whether their blocks overlap.
After the timed blocks each leg runs one more iteration from the same generator seed; its loss and point counts are reported.
In a chain row the time left in `fused` is mostly the row's own stand-ins for the renders (the gathers through the ops' index and the
synthetic depths), which both legs run: read the row as the difference of its legs, not `fused` as the cost of the three calls.
`--count-launches` (a run of its own) traces ONE chain-alone iteration of each leg after the warm-up (paired_bench's profiler pass) and
reports the kernels, copies and memsets it launched; it times nothing.
One JSON document on stdout and, with --out, in that file."""
import contextlib
import os
import sys

import torch

import paired_bench as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_workloads import SHAPES, cameras, config_opt      # noqa: E402
from sparf_amd import losses                                  # noqa: E402
from sparf_amd.edict import EasyDict as edict                 # noqa: E402
from sparf_amd.renderer import Graph                          # noqa: E402

LEGS = ("series", "fused")
THRESH = 0.2


def leg_context(leg):
    return losses.unfused() if leg == "series" else contextlib.nullcontext()


def unseen_pose(pose_a, pose_b, w=0.37):
    """depth_cons_loss.py:58-62: the reference's pose_inverse_4x4 of a blend of two c2w poses; [3,4] w2c in, [4,4] w2c and the first c2w out"""
    c2w = [losses.pose_inverse_4x4_torch(losses._to_4x4(p)) for p in (pose_a, pose_b)]
    return losses.pose_inverse_4x4_torch(w * c2w[0] + (1 - w) * c2w[1]), c2w[0]


class Chain:
    """project -> select -> loss and their backward on fixed inputs"""

    def __init__(self, leg, n, device):
        self.leg = leg
        H, W, f = 378, 504, 500.0
        g = torch.Generator().manual_seed(n)
        t = lambda x: x.float().to(device)
        self.H, self.W = H, W
        self.K = t(torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]))
        c, s = torch.cos(torch.tensor(0.2)), torch.sin(torch.tensor(0.2))
        Pa = torch.eye(4)[:3]
        Pb = torch.tensor([[c, 0, -s, 0.4], [0, 1, 0, -0.05], [s, 0, c, 0.1]])
        self.P, self.c2w = (t(x) for x in unseen_pose(Pa, Pb))
        self.px = t(torch.stack([torch.randint(0, W, (n,), generator=g), torch.randint(0, H, (n,), generator=g)], 1))
        self.depth_ref = t(torch.rand(n, generator=g) * 4.2 + 0.8).requires_grad_()
        self.depth_min = t(torch.tensor(1.2))
        self.vis = t(torch.rand(n, generator=g))
        self.noise = [t(torch.randn(n, generator=g) * s) for s in (0.8, 0.6)]
        self.opacity = [t(torch.rand(n, generator=g) * 0.4 + 0.6) for _ in range(2)]
        self.counts = None

    def iteration(self):
        self.depth_ref.grad = None
        with leg_context(self.leg):
            uv, z, i1 = losses.depth_consistency_project(None, self.P, self.K, self.H, self.W, self.depth_min, pixels_ref=self.px, depth_ref=self.depth_ref,
                                                         intr_ref=self.K, pose_c2w_ref=self.c2w)
            uv2, z2, v, i2 = losses.visibility_select(self.vis[i1], uv, z, THRESH)
            src = i1[i2]
            pix = 1e-3 * uv2.sum(-1)
            depth = [z2.detach() + x[src] + pix for x in self.noise]
            loss, avg = losses.depth_consistency_loss(z2, v, depth[0], self.opacity[0][src], depth[1], self.opacity[1][src])
        loss.backward()
        self.counts = (uv.shape[0], uv2.shape[0])
        return loss


class Whole:
    """reference render -> project -> render_to_max -> select -> render -> loss -> backward"""

    def __init__(self, leg, n, device, precision="bf16x3"):
        self.leg, s = leg, SHAPES[2]
        self.opt = config_opt(2, precision, rays=n)
        torch.manual_seed(0)
        self.graph = Graph(self.opt, device)
        self.graph.train()
        for net in (self.graph.nerf, self.graph.nerf_fine):
            net.progress.data.fill_(1.0)
        self.H, self.W = s["H"], s["W"]
        pose, intr = cameras(2, device)
        self.pose_ref, self.intr = pose[0], intr[0]
        c, sn = torch.cos(torch.tensor(0.2)), torch.sin(torch.tensor(0.2))
        rel = torch.tensor([[c, 0, -sn, 0.4], [0, 1, 0, -0.05], [sn, 0, c, 0.1]], device=device)      # the other view: 0.2 rad / 0.4 units from the first
        other = torch.cat([rel[:, :3] @ pose[0, :, :3], rel[:, :3] @ pose[0, :, 3:] + rel[:, 3:]], dim=-1)
        self.P, self.c2w = unseen_pose(pose[0], other)
        self.data = edict(depth_range=torch.tensor([list(s["rng"])] * pose.shape[0], dtype=torch.float32, device=device), iter=0)
        g = torch.Generator().manual_seed(1)
        self.px = torch.stack([torch.randint(0, self.W, (n,), generator=g), torch.randint(0, self.H, (n,), generator=g)], 1).to(device)
        self.counts = None

    def iteration(self):
        G, opt, data, H, W = self.graph, self.opt, self.data, self.H, self.W
        G.zero_grad(set_to_none=True)
        ref = G.render_image_at_specific_pose_and_rays(opt, data, self.pose_ref, self.intr, H, W, iter=0, pixels=self.px, mode="train")
        with leg_context(self.leg):
            uv, z, _ = losses.depth_consistency_project(None, self.P, self.intr, H, W, data.depth_range[0][0], pixels_ref=self.px,
                                                        depth_ref=ref.depth_fine, intr_ref=self.intr, pose_c2w_ref=self.c2w)
        with torch.no_grad():
            far = G.render_up_to_maxdepth_at_specific_pose_and_rays(opt, data, self.P[:3], self.intr, H, W, depth_max=z, pixels=uv, mode="train", iter=0)
        with leg_context(self.leg):
            uv2, z2, v, _ = losses.visibility_select(far["all_cumulated_fine"].squeeze(0), uv, z, THRESH)
        ret = G.render_image_at_specific_pose_and_rays(opt, data, self.P[:3], self.intr, H, W, pixels=uv2, mode="train", iter=0)
        with leg_context(self.leg):
            loss, avg = losses.depth_consistency_loss(z2, v, ret.depth, ret.opacity, ret.depth_fine, ret.opacity_fine)
        loss.backward()
        self.counts = (uv.shape[0], uv2.shape[0])
        return loss


def measure(works, blocks, iters, warmup):
    ms = pb.device_ms(works, blocks, iters, warmup)
    out = {k: pb.flat(t) for k, t in ms.items()}
    out["loss"] = {}
    for k, w in works.items():                                 # the reported iteration: every leg from the same generator state, so the
        torch.manual_seed(0)                                   # renders' stratified draws (and with them depth_ref) are the same in both
        out["loss"][k] = float(w.iteration().detach())
    out["points_after_mask_and_visibility"] = {k: w.counts for k, w in works.items()}
    ratio, less, overlap = pb.versus(ms["series"], ms["fused"])
    out.update(fused_over_series=ratio, fused_and_series_blocks_overlap=overlap, series_minus_fused_ms=less)
    return out


def count_launches(device, n, warmup):
    """-> per leg the device activities of ONE chain-alone iteration (forward + backward) after the warm-up (paired_bench.traced):
    kernels, memory copies and memsets, with the kernels' names"""
    works = {leg: Chain(leg, n, device) for leg in LEGS}
    for w in works.values():
        pb.device_block(w, warmup)
    out = {}
    for leg, w in works.items():
        t = pb.traced(w.iteration)
        out[leg] = dict(kernels=len(t.kernels), copies_and_memsets=len(t.copies), by_name=t.by_name)
    return out


def main():
    ap = pb.parser(__doc__)
    ap.add_argument("--rows", nargs="+", default=["chain", "whole"], choices=["chain", "whole"])
    ap.add_argument("--count-launches", action="store_true")
    a = ap.parse_args()
    device = pb.gpu_or_exit("tools/depth_cons_bench.py")
    if a.count_launches:
        doc = dict(tool="tools/depth_cons_bench.py --count-launches", device=torch.cuda.get_device_name(0), pixels=1024,
                   launches_per_iteration=count_launches(device, 1024, a.warmup))
    else:
        rows = {}
        if "chain" in a.rows:
            for n in (1024, 2048):
                rows[f"chain_{n}"] = measure({leg: Chain(leg, n, device) for leg in LEGS}, a.blocks, a.iters, a.warmup)
        if "whole" in a.rows:
            rows["whole_2048"] = measure({leg: Whole(leg, 2048, device) for leg in LEGS}, a.blocks, a.iters, a.warmup)
        doc = dict(tool="tools/depth_cons_bench.py", label=a.label, device=torch.cuda.get_device_name(0),
                   workload="depth-consistency loss, huber with the fine term, visibility threshold 0.2; chain_<n>: project, select, loss and "
                            "their backward on fixed inputs; whole_2048: reference render, project, render_to_max, select, render, loss, backward "
                            "at 2048 pixels x (64 + 128) in bf16x3",
                   blocks=a.blocks, iters_per_block=a.iters, warmup_iters=a.warmup, legs=list(LEGS), rows=rows)
    pb.emit(doc, a.out)


if __name__ == "__main__":
    main()
