"""The photometric / mask / depth-patch loss module, timed three ways.

    python tools/photo_loss_bench.py [--out profiles/photo_loss_bench.json] [--blocks 5] [--iters 20] [--warmup 5] [--rows alone render]

Legs.  `trainer` (a): the module as an unmodified trainer runs it -- the torch restatement of base_losses.py:274-319 and :180-194
(index build, permuted view, advanced-index gather, the colour, mask and patch terms) followed by compute_mse_on_rays (metrics.py:33-75,
which gathers again) for the logged PSNR; the baseline, never the code under test.  `today` (b): ops.photometric_loss on a torch-gathered
target plus the torch mask and patch terms and the same compute_mse_on_rays.  `fused` (c): losses.photo_and_regu_loss, one call that
also leaves the two MSEs.
Rows, all at 4 x 1024 rays (B = 4 images of 300 x 400, one shared list of 1024 ray indices), Huber: `alone_all` / `alone_colour`: the
module and its backward on fixed render outputs, with every term on (mask and P = 2) or the colour term only; `render_all` /
`render_colour`: the same behind a 4096-ray render at 64 + 128 samples in bf16x3, backward to both networks.
The legs of a row run in the alternating blocks of tools/paired_bench.py, of `--iters` iterations.  Per leg: device ms per iteration
and host ms per iteration (the host clock around the enqueue of the same block), each as median and min ... max over the blocks; after
the timed blocks, the kernels and copies of ONE iteration of the module alone (paired_bench's profiler pass).  The comparison is `fused` against `trainer` of the
same row.  One JSON document on stdout and, with --out, in that file."""
import os
import sys

import torch

import paired_bench as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_workloads import SHAPES, analytic_images, cameras, config_opt      # noqa: E402
from sparf_amd import losses, ops                                              # noqa: E402
from sparf_amd.edict import EasyDict as edict                                  # noqa: E402
from sparf_amd.renderer import Graph                                           # noqa: E402

LEGS = ("trainer", "today", "fused")
CONFIG, RAYS, PATCH = 1, 1024, 2
WEIGHTS = dict(render=1.0, fg_mask=0.5, depth_patch=0.25)


def module(leg, data, out, all_terms):
    """the loss module of one iteration on render outputs `out` -> (dict of terms, (mse, mse_fine))"""
    B = len(data.idx)
    kw = dict(huber=True)
    if all_terms:
        kw.update(fg_mask=data.fg_mask, opacity=out.opacity, opacity_fine=out.opacity_fine, depth=out.depth, depth_fine=out.depth_fine, patch_size=PATCH)
    if leg == "fused":
        terms, mse = losses.photo_and_regu_loss(data.image, out.ray_idx, out.rgb, out.rgb_fine, **kw)
        return terms, (mse["mse"], mse["mse_fine"])
    image = data.image.reshape(B, 3, -1).permute(0, 2, 1)
    target = losses.gather_rays_torch(image, out.ray_idx)
    if leg == "trainer":
        terms = dict(render=losses.colour_loss_torch(out.rgb.reshape(B, -1, 3), target, True) + losses.colour_loss_torch(out.rgb_fine.reshape(B, -1, 3), target, True))
    else:
        terms = dict(render=ops.photometric_loss(out.rgb.reshape(B, -1, 3), target.contiguous(), out.rgb_fine.reshape(B, -1, 3), huber=True))
    if all_terms:
        fg = losses.gather_rays_torch(data.fg_mask.float().view(B, -1, 1), out.ray_idx)
        terms["fg_mask"] = losses.fg_mask_loss_torch(fg, out.opacity.reshape(B, -1, 1)) + losses.fg_mask_loss_torch(fg, out.opacity_fine.reshape(B, -1, 1))
        terms["depth_patch"] = losses.depth_patch_loss_torch(out.depth.reshape(B, -1), PATCH) + losses.depth_patch_loss_torch(out.depth_fine.reshape(B, -1), PATCH)
    return terms, losses.mse_on_rays_torch(data, out)


def scene(device):
    s = SHAPES[CONFIG]
    pose, intr = cameras(CONFIG, device)
    image = analytic_images(pose, intr, s["H"], s["W"])
    g = torch.Generator().manual_seed(4)
    fg_mask = (torch.rand(s["B"], 1, s["H"], s["W"], generator=g) < 0.4).to(device)
    data = edict(idx=torch.arange(s["B"]), image=image, fg_mask=fg_mask, intr=intr, pose=pose,
                 depth_range=torch.tensor([list(s["rng"])] * s["B"], dtype=torch.float32, device=device))
    ray_idx = torch.randperm(s["H"] * s["W"], generator=g)[:RAYS].to(device)
    return s, data, ray_idx


class Alone:
    """the module and its backward on fixed render outputs"""

    def __init__(self, leg, all_terms, device):
        self.leg, self.all_terms = leg, all_terms
        s, self.data, ray_idx = scene(device)
        B = s["B"]
        g = torch.Generator().manual_seed(5)
        r = lambda *shape: torch.rand(*shape, generator=g).to(device).requires_grad_()
        self.out = edict(ray_idx=ray_idx, idx_img_rendered=torch.arange(B, device=device), rgb=r(B, RAYS, 3), rgb_fine=r(B, RAYS, 3), opacity=r(B, RAYS, 1),
                         opacity_fine=r(B, RAYS, 1), depth=r(B, RAYS, 1), depth_fine=r(B, RAYS, 1))
        self.leaves = [self.out[k] for k in ("rgb", "rgb_fine", "opacity", "opacity_fine", "depth", "depth_fine")]
        self.mse = None

    def iteration(self):
        for t in self.leaves:
            t.grad = None
        terms, self.mse = module(self.leg, self.data, self.out, self.all_terms)
        loss = sum(WEIGHTS[k] * v for k, v in terms.items())
        loss.backward()
        return loss


class BehindRender:
    """a 4 x 1024-ray render at 64 + 128 samples in bf16x3, the module, backward to both networks"""

    def __init__(self, leg, all_terms, device, precision="bf16x3"):
        self.leg, self.all_terms = leg, all_terms
        s, self.data, self.ray_idx = scene(device)
        self.opt = config_opt(CONFIG, precision, rays=s["B"] * RAYS)
        torch.manual_seed(0)
        self.graph = Graph(self.opt, device)
        self.graph.train()
        self.B, self.device, self.mse = s["B"], device, None

    def iteration(self):
        G = self.graph
        G.zero_grad(set_to_none=True)
        out = G.render_image_at_specific_rays(self.opt, self.data, iter=0, ray_idx=self.ray_idx, mode="train")
        out.ray_idx = self.ray_idx
        out.idx_img_rendered = torch.arange(self.B, device=self.device)
        terms, self.mse = module(self.leg, self.data, out, self.all_terms)
        loss = sum(WEIGHTS[k] * v for k, v in terms.items())
        loss.backward()
        return loss


def measure(works, blocks, iters, warmup, count):
    timed = pb.alternate(works, blocks, iters, warmup)
    dev, host = ({k: [v[i] for v in t] for k, t in timed.items()} for i in (0, 1))
    out = {k: dict(device_ms_per_iter=pb.summary(dev[k]), host_ms_per_iter=pb.summary(host[k])) for k in works}
    for k, w in works.items():
        torch.manual_seed(0)
        out[k]["loss"] = float(w.iteration().detach())
        out[k]["mse"] = [float(m) for m in w.mse]
        if count:                                              # the kernels and copies of ONE iteration (paired_bench.traced)
            t = pb.traced(w.iteration)
            out[k]["launches_per_iteration"] = dict(kernels=len(t.kernels), copies_and_memsets=len(t.copies))
    ratio, less, overlap = pb.versus(dev["trainer"], dev["fused"])
    out.update(fused_over_trainer_device=ratio, fused_over_trainer_host=pb.versus(host["trainer"], host["fused"])[0],
               trainer_minus_fused_device_ms=less, fused_and_trainer_blocks_overlap=overlap)
    return out


def main():
    ap = pb.parser(__doc__)
    ap.add_argument("--rows", nargs="+", default=["alone", "render"], choices=["alone", "render"])
    a = ap.parse_args()
    device = pb.gpu_or_exit("tools/photo_loss_bench.py")
    rows = {}
    for terms, all_terms in (("all", True), ("colour", False)):
        if "alone" in a.rows:
            rows[f"alone_{terms}"] = measure({leg: Alone(leg, all_terms, device) for leg in LEGS}, a.blocks, a.iters, a.warmup, count=True)
        if "render" in a.rows:
            rows[f"render_{terms}"] = measure({leg: BehindRender(leg, all_terms, device) for leg in LEGS}, a.blocks, a.iters, a.warmup, count=False)
    doc = dict(tool="tools/photo_loss_bench.py", label=a.label, device=torch.cuda.get_device_name(0),
               workload="BasePhotoandReguLoss.compute_loss + compute_mse_on_rays at 4 x 1024 rays of 4 images of 300 x 400, Huber; all: mask and "
                        "depth patch P = 2 on; alone: the module and its backward on fixed render outputs; render: behind a 4096-ray render at "
                        "64 + 128 samples in bf16x3, backward to both networks",
               blocks=a.blocks, iters_per_block=a.iters, warmup_iters=a.warmup, legs=dict(trainer="(a) torch restatement + compute_mse_on_rays",
                                                                                          today="(b) ops.photometric_loss on a torch-gathered target + torch mask / patch terms + compute_mse_on_rays",
                                                                                          fused="(c) losses.photo_and_regu_loss"), rows=rows)
    pb.emit(doc, a.out)


if __name__ == "__main__":
    main()
