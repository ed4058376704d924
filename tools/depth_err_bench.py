"""The depth errors on rendered rays of a training iteration's result dict, timed three ways.

    python tools/depth_err_bench.py [--out profiles/depth_err_bench.json] [--blocks 5] [--iters 20] [--warmup 5]
                                    [--rows alone render] [--batches 3 6 9] [--trace-only]

Legs.  `series`: metrics.compute_depth_error_on_rays under `metrics.unfused()`, once per head -- the torch restatement of
metrics.py:103-134 in the reference's order (per head two indexed copies of every map, the index build, two gathers, two boolean
selections with their readbacks, eight small reductions): what an unmodified trainer runs; the baseline, never the code under test.
`fused`: metrics.depth_error_on_rays, ONE call for both heads.  `installed`: metrics.compute_depth_error_on_rays as
install_depth_error_on_rays() puts it under the reference's name, once per head (two calls).  All under torch.no_grad(), as the
trainer's make_result_dict runs them, with idx_img_rendered a device arange.
Rows, for B in {3, 6, 9} maps of 300 x 400 with 2048 rays as ray_idx [B, 2048 // B]: `alone_B<B>`: on fixed render outputs;
`render_B<B>`: behind a real render step of those rays at 64 + 128 samples in bf16x3 with a backward to both networks.  The legs of
a row run in the alternating blocks of tools/paired_bench.py, of `--iters` iterations (ten times as many in an `alone` row); per leg
ms per iteration as median and min ... max over the blocks, each leg over `series`, and whether their blocks overlap.
`--trace-only` (a run of its own: tracing slows the host) times nothing: it traces ONE iteration of the depth errors of each leg of
every `alone` row after the warm-up (paired_bench's profiler pass) and reports the kernels, the copies under the profiler's labels,
the readbacks where they are asked for and the host waits (a blocking copy is a readback or the upload of a host index), without any
device synchronise, under `traced_iteration`.  One JSON document on stdout and, with --out, in that file
(a --trace-only run adds its key to the document already there)."""
import contextlib
import os
import sys

import torch

import paired_bench as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_workloads import SHAPES, cameras, config_opt      # noqa: E402
from sparf_amd import metrics                                 # noqa: E402
from sparf_amd.edict import EasyDict as edict                 # noqa: E402
from sparf_amd.renderer import Graph                          # noqa: E402

LEGS = ("series", "fused", "installed")
H, W, RAYS, CONFIG, SCALE = 300, 400, 2048, 1, 1.7
ALONE_ITERS = 10                                               # an alone block runs this many times --iters: it is short work


def maps(B, device):
    """depth_gt [B,1,H,W] inside the scene's range and valid_depth_gt [B,1,H,W], true at about 80 % of the pixels"""
    g = torch.Generator().manual_seed(B)
    lo, hi = SHAPES[CONFIG]["rng"]
    depth = lo + 0.2 + (hi - lo - 0.4) * torch.rand(B, 1, H, W, generator=g)
    valid = torch.rand(B, 1, H, W, generator=g) < 0.8
    return depth.to(device), valid.to(device)


def poses(B, device):
    pose, intr = cameras(CONFIG, device)
    n = pose.shape[0]
    idx = [b % n for b in range(B)]
    return pose[idx].contiguous(), intr[idx].contiguous()


def depth_errors(leg, data, out):
    """the depth errors of both heads as the leg computes them -> tensors on the device"""
    with torch.no_grad():
        if leg == "fused":
            res = metrics.depth_error_on_rays(data.depth_gt, data.valid_depth_gt, out.depth, out.depth_fine, ray_idx=out.ray_idx,
                                              img_idx=out.idx_img_rendered, scale=SCALE)
            return [res.abs_e, res.rmse, res.abs_e_fine, res.rmse_fine]
        with metrics.unfused() if leg == "series" else contextlib.nullcontext():
            return [*metrics.compute_depth_error_on_rays(data, out, out.depth, SCALE), *metrics.compute_depth_error_on_rays(data, out, out.depth_fine, SCALE)]


class Work:
    def __init__(self, leg, B, device, render):
        self.leg, self.B, self.render = leg, B, render
        n = RAYS // B
        depth_gt, valid = maps(B, device)
        pose, intr = poses(B, device)
        g = torch.Generator().manual_seed(7 + B)
        self.ray_idx = torch.stack([torch.randperm(H * W, generator=g)[:n] for _ in range(B)]).to(device)
        self.data = edict(idx=torch.arange(B), image=torch.zeros(B, 3, H, W, device=device), intr=intr, pose=pose, depth_gt=depth_gt, valid_depth_gt=valid,
                          depth_range=torch.tensor([list(SHAPES[CONFIG]["rng"])] * B, dtype=torch.float32, device=device))
        self.img_idx = torch.arange(B, device=device)
        if render:
            self.opt = config_opt(CONFIG, "bf16x3", rays=B * n)
            torch.manual_seed(0)
            self.graph = Graph(self.opt, device)
            self.graph.train()
        else:
            lo, hi = SHAPES[CONFIG]["rng"]
            r = lambda: (lo + (hi - lo) * torch.rand(B, n, 1, generator=g)).to(device)
            self.out = edict(ray_idx=self.ray_idx, idx_img_rendered=self.img_idx, depth=r(), depth_fine=r())
        self.values = None

    def step(self):
        """the render step in front of the result dict -> its outputs"""
        if not self.render:
            return self.out
        G = self.graph
        G.zero_grad(set_to_none=True)
        out = G.render_image_at_specific_rays(self.opt, self.data, iter=0, ray_idx=self.ray_idx, mode="train")
        out.ray_idx, out.idx_img_rendered = self.ray_idx, self.img_idx
        ((out.rgb - 0.5).square().mean() + (out.rgb_fine - 0.5).square().mean()).backward()
        return out

    def iteration(self):
        self.values = depth_errors(self.leg, self.data, self.step())

    def result(self):
        return [float(v) for v in self.values]


def traced(work):
    """-> the device activities of the depth errors of ONE iteration (paired_bench.traced): kernels, copies and memsets, the readbacks
    where they are asked for and the runtime calls that make the host wait, without every device synchronise (the profiler's own too)"""
    out = work.step()
    t = pb.traced(lambda: depth_errors(work.leg, work.data, out), host=True, every_device_sync=True)
    return dict(kernels=len(t.kernels), copies_and_memsets=len(t.copies), copies_by_label=t.copies_by_label, readbacks=t.readbacks_asked,
                host_waits=len(t.host_waits), host_waits_by_name={x: t.host_waits.count(x) for x in sorted(set(t.host_waits))})


def measure(works, blocks, iters, warmup):
    ms = pb.device_ms(works, blocks, iters, warmup)
    out = {k: pb.flat(t) for k, t in ms.items()}
    out["result"] = {k: w.result() for k, w in works.items()}
    for k in LEGS[1:]:
        ratio, less, overlap = pb.versus(ms["series"], ms[k])
        out.update({f"{k}_over_series": ratio, f"{k}_and_series_blocks_overlap": overlap, f"series_minus_{k}_ms": less})
    return out


def main():
    ap = pb.parser(__doc__)
    ap.add_argument("--rows", nargs="+", default=["alone", "render"], choices=["alone", "render"])
    ap.add_argument("--batches", nargs="+", type=int, default=[3, 6, 9])
    ap.add_argument("--trace-only", action="store_true", help="trace one iteration of each leg with the profiler; time nothing")
    a = ap.parse_args()
    device = pb.gpu_or_exit("tools/depth_err_bench.py")
    rows = {}
    for B in a.batches:
        for kind in (["alone"] if a.trace_only else a.rows):
            works = {leg: Work(leg, B, device, kind == "render") for leg in LEGS}
            if a.trace_only:
                for w in works.values():
                    pb.device_block(w, a.warmup)
                rows[f"{kind}_B{B}"] = {leg: traced(w) for leg, w in works.items()}
            else:
                rows[f"{kind}_B{B}"] = measure(works, a.blocks, a.iters * (ALONE_ITERS if kind == "alone" else 1), a.warmup)
    if a.trace_only:
        doc = pb.existing(a.out, dict(tool="tools/depth_err_bench.py --trace-only"))
        doc["traced_iteration"] = rows
    else:
        doc = dict(tool="tools/depth_err_bench.py", label=a.label, device=torch.cuda.get_device_name(0),
                   workload=f"compute_depth_error_on_rays of both heads on B maps of {H} x {W}, {RAYS} rays as ray_idx [B, {RAYS} // B], scale {SCALE}, "
                            "idx_img_rendered a device arange; alone_B<B>: on fixed render outputs; render_B<B>: behind a real render step (bf16x3, "
                            "64 + 128 samples) with its backward",
                   blocks=a.blocks, iters_per_block=a.iters, alone_iters_per_block=ALONE_ITERS * a.iters, warmup_iters=a.warmup, legs=list(LEGS), rows=rows)
    pb.emit(doc, a.out)


if __name__ == "__main__":
    main()
