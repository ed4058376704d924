"""The evaluation metrics of one view, timed two ways.

    python tools/image_metrics_bench.py [--out profiles/image_metrics_bench.json] [--blocks 5] [--iters 20] [--render-iters 3] [--warmup 3]
    python tools/image_metrics_bench.py --trace-only --out profiles/image_metrics_bench.json      (a run of its own: adds the counts)

Legs.  `series`: the torch restatement exactly as a trainer issues it (nerf_trainer.py:387-405) -- metrics.compute_metrics under
metrics.unfused() for the coarse head, then for the fine head, with a trivial lpips_loss (a constant host tensor; the x 2 - 1 inputs the
reference forms for it are part of the leg) --; the baseline, never the code under test.  It reads back once per call where the
reference's own functions read back 5 to 14 times per head.  `fused`: one two-head metrics.image_metrics call plus the readback of its
vector.
Rows: one view (B = 1) of 300 x 400 and of 378 x 504; `plain` (PSNR and SSIM only) and `all` (foreground mask and depth errors at a scale
of 1.37 as well); `alone` on fixed render outputs and `render` behind a full-image render at 64 + 128 samples in bf16x3 under no_grad.
The legs of a row run in the alternating blocks of tools/paired_bench.py.  Per leg: device ms per iteration as median and min ... max
over the blocks, and whether the legs' ranges overlap.  --trace-only, in a run of its own: the kernels, copies and readbacks
(device-to-host copies, by label) of ONE iteration of each `alone` row (paired_bench's profiler pass), merged into the document of --out.  One JSON document on stdout and, with --out, in that file."""
import os
import sys

import torch

import paired_bench as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat")]
from bench_workloads import analytic_images, cameras                           # noqa: E402
from sparf_amd import metrics                                                  # noqa: E402
from sparf_amd.config import baseline_opt                                      # noqa: E402
from sparf_amd.edict import EasyDict as edict                                  # noqa: E402
from sparf_amd.renderer import Graph                                           # noqa: E402

LEGS = ("series", "fused")
SIZES = ((300, 400), (378, 504))
SCALE = 1.37
DEPTH_RANGE = [1.2, 5.2]
_LPIPS = torch.tensor(0.25)


def lpips_stub(a, b):
    return _LPIPS


def scene(H, W, device):
    pose, intr = cameras(1, device)                       # config 1: views on a ring, 300 x 400
    pose, intr = pose[:1], intr[:1].clone()
    intr[:, 0] *= W / 400
    intr[:, 1] *= H / 300
    image = analytic_images(pose, intr, H, W)
    g = torch.Generator().manual_seed(4)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    fg = (((yy - H / 2) / (0.35 * H)) ** 2 + ((xx - W / 2) / (0.35 * W)) ** 2 < 1.0).reshape(1, 1, H, W).to(device)
    data = edict(idx=torch.arange(1, device=device), image=image, fg_mask=fg, depth_gt=(1.5 + 3 * torch.rand(1, 1, H, W, generator=g)).to(device),
                 valid_depth_gt=(torch.rand(1, 1, H, W, generator=g) < 0.6).to(device))
    return pose, intr, data


def evaluate(leg, data, out, H, W, all_terms):
    """the metrics of one view on render outputs `out`, read back -> list / dict of Python floats"""
    as_image = lambda rgb: rgb.view(-1, H, W, 3).permute(0, 3, 1, 2)
    if leg == "fused":
        kw = dict(fg_mask=data.fg_mask, depth=out.depth, depth_fine=out.depth_fine, depth_gt=data.depth_gt, valid_depth_gt=data.valid_depth_gt,
                  depth_scale=SCALE) if all_terms else {}
        return metrics.image_metrics(as_image(out.rgb), data.image, pred_fine=as_image(out.rgb_fine), **kw).vector.tolist()
    d = data if all_terms else edict(idx=data.idx, image=data.image)
    with metrics.unfused():
        res = metrics.compute_metrics(d, out, as_image(out.rgb), out.depth, data.image, lpips_stub, SCALE, suffix="_c")
        res.update(metrics.compute_metrics(d, out, as_image(out.rgb_fine), out.depth_fine, data.image, lpips_stub, SCALE, suffix="_f"))
    return res


class Alone:
    """the metrics on fixed render outputs"""

    def __init__(self, leg, H, W, all_terms, device):
        self.leg, self.H, self.W, self.all_terms = leg, H, W, all_terms
        _, _, self.data = scene(H, W, device)
        g = torch.Generator().manual_seed(5)
        target = self.data.image.reshape(1, 3, H * W).permute(0, 2, 1)
        noisy = lambda s: (target + s * torch.randn(1, H * W, 3, generator=g).to(device)).clamp(0, 1).contiguous()
        depth = lambda: (self.data.depth_gt.reshape(1, H * W, 1) / 1.3 + 0.1 * torch.randn(1, H * W, 1, generator=g).to(device)).contiguous()
        self.out = edict(idx_img_rendered=torch.arange(1, device=device), rgb=noisy(0.1), rgb_fine=noisy(0.03), depth=depth(), depth_fine=depth())

    def iteration(self):
        return evaluate(self.leg, self.data, self.out, self.H, self.W, self.all_terms)


class BehindRender:
    """a full-image render at 64 + 128 samples in bf16x3 under no_grad, then the metrics"""

    def __init__(self, leg, H, W, all_terms, device, precision="bf16x3"):
        self.leg, self.H, self.W, self.all_terms = leg, H, W, all_terms
        self.pose, self.intr, self.data = scene(H, W, device)
        self.opt = baseline_opt(1, hip=dict(precision=precision))
        torch.manual_seed(0)
        self.graph = Graph(self.opt, device)
        self.device = device

    @torch.no_grad()
    def iteration(self):
        ret = self.graph.render_by_slices(self.opt, self.pose, H=self.H, W=self.W, intr=self.intr, depth_range=DEPTH_RANGE, iter=None, mode="val")
        out = edict(idx_img_rendered=torch.arange(1, device=self.device), rgb=ret.rgb, rgb_fine=ret.rgb_fine, depth=ret.depth, depth_fine=ret.depth_fine)
        return evaluate(self.leg, self.data, out, self.H, self.W, self.all_terms)


def launches(work):
    """the device activities of ONE iteration (paired_bench.traced) -> dict(kernels, copies_and_memsets, readbacks by label)"""
    work.iteration()
    t = pb.traced(work.iteration)
    return dict(kernels=len(t.kernels), copies_and_memsets=len(t.copies), readbacks=t.readbacks_by_label)


def measure(works, blocks, iters, warmup):
    dev = pb.device_ms(works, blocks, iters, warmup)
    out = {k: dict(device_ms_per_iter=pb.summary(dev[k])) for k in works}
    out["fused_over_series_device"], out["series_minus_fused_device_ms"], out["blocks_overlap"] = pb.versus(dev["series"], dev["fused"])
    return out


def agreement(works):
    """the two legs' values of one iteration side by side (the series is fp32 torch: they agree to its rounding, not bit for bit)"""
    res, vec = works["series"].iteration(), works["fused"].iteration()
    return dict(series=dict(psnr_c=res.psnr_c, ssim_c=res.ssim_c, psnr_f=res.psnr_f, ssim_f=res.ssim_f), fused=dict(psnr_c=vec[0][1], ssim_c=vec[0][2], psnr_f=vec[1][1], ssim_f=vec[1][2]))


def main():
    ap = pb.parser(__doc__, warmup=3)
    ap.add_argument("--rows", nargs="+", default=["alone", "render"], choices=["alone", "render"])
    ap.add_argument("--render-iters", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true", help="only the launch counts of the `alone` rows, merged into the document of --out")
    a = ap.parse_args()
    device = pb.gpu_or_exit("tools/image_metrics_bench.py")
    if a.trace_only:
        doc = pb.existing(a.out, dict(tool="tools/image_metrics_bench.py", rows={}))
        for H, W in SIZES:
            for terms, all_terms in (("plain", False), ("all", True)):
                row = doc["rows"].setdefault(f"alone_{H}x{W}_{terms}", {})
                row["launches_per_iteration"] = {leg: launches(Alone(leg, H, W, all_terms, device)) for leg in LEGS}
    else:
        rows = {}
        for H, W in SIZES:
            for terms, all_terms in (("plain", False), ("all", True)):
                if "alone" in a.rows:
                    works = {leg: Alone(leg, H, W, all_terms, device) for leg in LEGS}
                    rows[f"alone_{H}x{W}_{terms}"] = dict(measure(works, a.blocks, a.iters, a.warmup), values=agreement(works))
                if "render" in a.rows:
                    works = {leg: BehindRender(leg, H, W, all_terms, device) for leg in LEGS}
                    rows[f"render_{H}x{W}_{terms}"] = measure(works, a.blocks, a.render_iters, 1)
        doc = dict(tool="tools/image_metrics_bench.py", label=a.label, device=torch.cuda.get_device_name(0),
                   workload="the evaluation metrics of one view (B = 1), both heads: PSNR and SSIM (plain), with the foreground-masked variants and the "
                            "depth errors at scale 1.37 (all); alone: on fixed render outputs; render: behind a full-image render at 64 + 128 samples "
                            "in bf16x3 under no_grad",
                   blocks=a.blocks, iters_per_block=a.iters, render_iters_per_block=a.render_iters, warmup_iters=a.warmup,
                   legs=dict(series="metrics.compute_metrics under metrics.unfused(), coarse head then fine head, trivial lpips_loss",
                             fused="one two-head metrics.image_metrics call + the readback of its vector"), rows=rows)
    pb.emit(doc, a.out)


if __name__ == "__main__":
    main()
