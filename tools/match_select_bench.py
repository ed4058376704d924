"""The correspondence sampler, timed as the torch series and as the two library calls.

    python tools/match_select_bench.py [--out profiles/match_select_bench.json] [--blocks 5] [--iters 20] [--warmup 5]
                                       [--rows sampler whole] [--count-launches]

Legs.  `series`: everything under `losses.unfused()` -- the torch restatement of base_corres_loss.py:260-269, :323-328, :365-369 and
corres_loss.py:139-155 (the centre mask, the rounded index map of the whole image, mask.sum(), five boolean selections, randperm, five
gathers) and, in a `whole` row, of the loss body: what an unmodified trainer runs; the baseline, never the code under test.
`fused`: `losses.select_matches` (compact, one readback, randperm, gather) and, in a `whole` row, the loss kernel.  A `whole` row has a
third leg, `body`: the loss kernel on and ONLY the sampler restated (`losses.unfused_sampler()`), so that `body` - `fused` is the sampler's
own share of the row and `series` - `body` the loss body's, which an earlier change measured.
Rows, at 300 x 400 with max_matches = 512 and at 378 x 504 with max_matches = 1024 (rand_rays // 2 of the reference's default
configurations for 360-degree and forward-facing data), in the pre-crop phase (window of precrop_frac 0.5) on a mask that keeps about
40 % of the pixels: `sampler_<H>x<W>`: select_matches alone; `whole_<H>x<W>`: losses.compute_loss_on_image_pair on a stand-in around a
real Graph -- the sampler, two renders of max_matches pixels at 64 + 128 samples in bf16x3, the loss, backward to poses and networks.
The legs of a row run in the alternating blocks of tools/paired_bench.py, of `--iters` iterations (ten times as many in a sampler row);
per leg ms per iteration as median and min ... max over the blocks, `fused` over `series`, and whether their blocks overlap.  After the timed blocks each leg
runs one more iteration from the same seed; the count, the selected ray indices' checksum and, in a whole row, the loss are reported.
`--count-launches` (a run of its own) traces ONE sampler-alone iteration of each leg after the warm-up (paired_bench's profiler pass) and
reports the kernels, copies and memsets it launched and the host waits; it times nothing.
One JSON document on stdout and, with --out, in that file."""
import contextlib
import os
import sys
import types

import torch

import paired_bench as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_workloads import SHAPES, cameras, config_opt      # noqa: E402
from sparf_amd import losses                                  # noqa: E402
from sparf_amd.edict import EasyDict as edict                 # noqa: E402
from sparf_amd.renderer import Graph                          # noqa: E402

LEGS = ("series", "fused")
WHOLE_LEGS = ("series", "body", "fused")                      # body: the loss kernel of an earlier change on, the sampler still torch's
SIZES = {(300, 400): (512, 2), (378, 504): (1024, 3)}          # H, W -> max_matches, bench_workloads config of that image size
PRECROP_FRAC = 0.5
SAMPLER_ITERS = 10                                             # a sampler-alone block runs this many times --iters: it is short work


def leg_context(leg):
    return losses.unfused() if leg == "series" else losses.unfused_sampler() if leg == "body" else contextlib.nullcontext()


def maps(H, W, device):
    """what CorrespondenceBasedLoss stores for 3 pairs ([3,1,H,W] bool, [3,2,H,W], [3,1,H,W]); pair 1 as sample_valid_image_pair hands it
    over.  Correspondences: the pixel grid moved by a smooth field, inside the image; valid where a smooth confidence is high (~40 %)."""
    g = torch.Generator().manual_seed(H * W)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    cx = (xs + 9.3 * torch.sin(ys / 37.0) + torch.rand(H, W, generator=g)).clamp(0, W - 1)
    cy = (ys + 7.1 * torch.cos(xs / 53.0) + torch.rand(H, W, generator=g)).clamp(0, H - 1)
    conf = 0.5 + 0.5 * torch.sin(xs / 23.0) * torch.cos(ys / 31.0) + 0.05 * torch.rand(H, W, generator=g)
    corres = torch.stack([cx, cy]).expand(3, 2, H, W).contiguous().to(device)
    conf = conf.expand(3, 1, H, W).contiguous().to(device)
    mask = conf.ge(0.6)
    return mask[1].permute(1, 2, 0), corres[1].permute(1, 2, 0)[:, :, :2], conf[1].permute(1, 2, 0)


def precrop_window(H, W):
    dH, dW = int(H // 2 * PRECROP_FRAC), int(W // 2 * PRECROP_FRAC)
    return (H // 2 - dH, H // 2 + dH - 1, W // 2 - dW, W // 2 + dW - 1)


class Sampler:
    """select_matches alone"""

    def __init__(self, leg, H, W, device):
        self.leg, self.max_matches = leg, SIZES[(H, W)][0]
        self.mask, self.corres, self.conf = maps(H, W, device)
        self.window = precrop_window(H, W)
        self.report = None

    def iteration(self):
        with leg_context(self.leg):
            out = losses.select_matches(self.mask, self.corres, self.conf, self.max_matches, window=self.window)
        self.report = dict(count=out[5], rows=out[1].shape[0], ray_self_sum=out[1], ray_other_sum=out[3])
        return out

    def result(self):
        return dict(self.report, ray_self_sum=int(self.report["ray_self_sum"].sum()), ray_other_sum=int(self.report["ray_other_sum"].sum()))


class Whole:
    """compute_loss_on_image_pair around a real Graph, and its backward"""

    def __init__(self, leg, H, W, device, precision="bf16x3"):
        self.leg = leg
        max_matches, config = SIZES[(H, W)]
        s = SHAPES[config]
        assert (s["H"], s["W"]) == (H, W)
        self.opt = config_opt(config, precision, rays=2 * max_matches)
        torch.manual_seed(0)
        self.graph = Graph(self.opt, device)
        self.graph.train()
        for net in (self.graph.nerf, self.graph.nerf_fine):
            net.progress.data.fill_(1.0)
        pose, intr = cameras(config, device)
        self.poses = pose[:2].clone().requires_grad_()
        self.intrs = intr[:2]
        self.images = torch.zeros(2, H, W, 3, device=device)
        self.mask, self.corres, self.conf = maps(H, W, device)
        self.window = precrop_window(H, W)
        self.data = edict(depth_range=torch.tensor([list(s["rng"])] * pose.shape[0], dtype=torch.float32, device=device), iter=0)
        self.obj = types.SimpleNamespace(net=self.graph, device=device, opt=edict(self.opt))
        self.obj.opt.update(min_nbr_matches=500, compute_photo_on_matches=False, diff_loss_type="huber", use_gt_correspondences=False,
                            renderrepro_do_pixel_reprojection_check=False, renderrepro_do_depth_reprojection_check=False,
                            renderrepro_pixel_reprojection_thresh=10.0, renderrepro_depth_reprojection_thresh=0.1)
        self.report = None

    def iteration(self):
        self.graph.zero_grad(set_to_none=True)
        self.poses.grad = None
        stats = {}
        with leg_context(self.leg):
            loss_dict, stats, _ = losses.compute_loss_on_image_pair(
                self.obj, self.data, self.images, self.poses, self.intrs, 0, 1, self.corres, None, self.conf, self.mask.squeeze(-1),
                losses._to_4x4(self.poses[0]), losses._to_4x4(self.poses[1]), self.intrs[0], self.intrs[1],
                {"corres": torch.zeros((), device=self.poses.device)}, stats, {}, window=self.window)
        loss_dict["corres"].backward()
        self.report = dict(loss=loss_dict["corres"].detach(), perc_valid_corr_mask=stats["perc_valid_corr_mask"])
        return loss_dict["corres"]

    def result(self):
        return {k: float(v) for k, v in self.report.items()}


def measure(works, blocks, iters, warmup):
    ms = pb.device_ms(works, blocks, iters, warmup)
    out = {k: pb.flat(t) for k, t in ms.items()}
    out["result"] = {}
    for k, w in works.items():                                 # the reported iteration: every leg from the same generator state
        torch.manual_seed(0)
        w.iteration()
        out["result"][k] = w.result()
    ratio, less, overlap = pb.versus(ms["series"], ms["fused"])
    out.update(fused_over_series=ratio, fused_and_series_blocks_overlap=overlap, series_minus_fused_ms=less)
    if "body" in ms:
        _, less, overlap = pb.versus(ms["body"], ms["fused"])
        out.update(body_minus_fused_ms=less, fused_and_body_blocks_overlap=overlap)
    return out


def count_launches(device, H, W, warmup):
    """-> per leg the device activities of ONE sampler-alone iteration after the warm-up (paired_bench.traced): kernels, memory copies
    and memsets with the kernels' names, and the host waits"""
    works = {leg: Sampler(leg, H, W, device) for leg in LEGS}
    for w in works.values():
        pb.device_block(w, warmup)
    out = {}
    for leg, w in works.items():
        t = pb.traced(w.iteration, host=True)
        out[leg] = dict(kernels=len(t.kernels), copies_and_memsets=len(t.copies), copies_by_name=sorted(t.copies), host_waits=len(t.host_waits),
                        host_waits_by_name=t.host_waits, by_name=t.by_name)
    return out


def main():
    ap = pb.parser(__doc__)
    ap.add_argument("--rows", nargs="+", default=["sampler", "whole"], choices=["sampler", "whole"])
    ap.add_argument("--count-launches", action="store_true")
    a = ap.parse_args()
    device = pb.gpu_or_exit("tools/match_select_bench.py")
    if a.count_launches:
        doc = dict(tool="tools/match_select_bench.py --count-launches", device=torch.cuda.get_device_name(0),
                   launches_per_iteration={f"{H}x{W}": count_launches(device, H, W, a.warmup) for H, W in SIZES})
    else:
        rows = {}
        for (H, W) in SIZES:
            if "sampler" in a.rows:
                rows[f"sampler_{H}x{W}"] = measure({leg: Sampler(leg, H, W, device) for leg in LEGS}, a.blocks, SAMPLER_ITERS * a.iters, a.warmup)
            if "whole" in a.rows:
                rows[f"whole_{H}x{W}"] = measure({leg: Whole(leg, H, W, device) for leg in WHOLE_LEGS}, a.blocks, a.iters, a.warmup)
        doc = dict(tool="tools/match_select_bench.py", label=a.label, device=torch.cuda.get_device_name(0),
                   workload="correspondence sampler in the pre-crop phase on a mask of ~40 % valid pixels; sampler_<HxW>: select_matches alone; "
                            "whole_<HxW>: compute_loss_on_image_pair (sampler, two renders of max_matches pixels x (64 + 128) in bf16x3, huber "
                            "loss with the fine term) and its backward",
                   max_matches={f"{H}x{W}": m for (H, W), (m, _) in SIZES.items()},
                   blocks=a.blocks, iters_per_block=a.iters, sampler_iters_per_block=SAMPLER_ITERS * a.iters, warmup_iters=a.warmup, legs=list(LEGS), whole_legs=list(WHOLE_LEGS), rows=rows)
    pb.emit(doc, a.out)


if __name__ == "__main__":
    main()
