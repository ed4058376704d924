"""The DS-NeRF sparse depth loss, timed as the torch series of the reference method and as the installed method (SURVEY 8f next-12,
DESIGN 4.14).

    python tools/colmap_depth_bench.py [--out profiles/colmap_depth_bench.json] [--blocks 5] [--iters 10] [--warmup 3]
                                       [--rows alone whole] [--batches 3 6 9] [--trace-only]

Legs.  `series`: losses.compute_colmap_depth_loss under `losses.unfused()` on a Graph with opt.hip.lazy_batch off -- the torch
restatement of base_losses.py:363-400 in the reference's order (per image a torch.where with its readback, randperm, six index and
gather operations, a render of its own, two weighted means; one more torch.where over all images): what an unmodified trainer runs; the
baseline, never the code under test.  `installed`: the same function as install_colmap_depth() puts it on the class -- one compaction,
one readback, per image its randperm, its gather and its deferred render, one batch of renders, one loss call.
Rows, for B in {3, 6, 9} images of 300 x 400 with rand_rays = 2048 (quota 682 / 341 / 227) on COLMAP maps that hold a depth at about
2 % of the pixels (about 2400 per image: every image draws): `alone_B<B>`: the method with a stand-in render (a depth that is an
elementwise function of ray_idx, no network); `whole_B<B>`: around a real Graph in bf16x3 at 64 + 128 samples, with the backward to
the networks.  Both legs of a row run in the alternating blocks of tools/paired_bench.py, of `--iters` iterations (ten times as many
in an `alone` row); per leg ms per iteration as median and min ... max over the blocks, `installed` over `series`, and whether
their blocks overlap.  After the timed blocks each leg runs one more iteration from the same seed under counters: the host readbacks
it made (single-argument torch.where calls, .item() and .tolist()), its render calls and how many launch sets they became; the loss and
the ray lists' checksum are reported.  `--trace-only` (a run of its own: tracing slows the host) times nothing: it traces ONE iteration
of each leg of every row after the warm-up (paired_bench's profiler pass) and reports the kernels, copies and memsets it launched and
the host waits, under `traced_iteration`.  One JSON document on stdout and, with --out, in that file (a --trace-only run adds its
key to the document already there)."""
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

LEGS = ("series", "installed")
H, W, RAND_RAYS, CONFIG = 300, 400, 2048, 1
ALONE_ITERS = 10                                               # an alone block runs this many times --iters: it is short work


def leg_context(leg):
    return losses.unfused() if leg == "series" else contextlib.nullcontext()


def maps(B, device):
    """colmap_depth / colmap_conf [B,1,H,W]: a depth inside the scene's range at about 2 % of the pixels, 0 elsewhere"""
    g = torch.Generator().manual_seed(B)
    lo, hi = SHAPES[CONFIG]["rng"]
    depth = lo + 0.2 + (hi - lo - 0.4) * torch.rand(B, 1, H, W, generator=g)
    depth = torch.where(torch.rand(B, 1, H, W, generator=g) < 0.02, depth, torch.zeros(()))
    conf = 0.25 + 0.75 * torch.rand(B, 1, H, W, generator=g)
    return depth.to(device), conf.to(device)


def poses(B, device):
    pose, intr = cameras(CONFIG, device)
    n = pose.shape[0]
    idx = [b % n for b in range(B)]
    return pose[idx].contiguous(), intr[idx].contiguous()


class StandInNet:
    """a render without a network: depths that are an elementwise function of ray_idx (no synchronisation, a handful of launches)"""

    def __init__(self, B, device):
        self.pose, self.intr = poses(B, device)
        self.scale = torch.ones((), device=device, requires_grad=True)
        self.lazy_stats, self.calls = dict(batches=0, requests=0), 0

    def get_w2c_pose(self, opt, data_dict, mode=None):
        return self.pose

    def render_image_at_specific_pose_and_rays(self, opt, data_dict, pose, intr, H, W, ray_idx=None, mode=None, iter=None):
        self.calls += 1
        d = (2.0 + (ray_idx % 1013).to(torch.float32) / 512.0) * self.scale
        return edict(depth=d[None, :, None], depth_fine=(d + 0.0625)[None, :, None])


class Work:
    def __init__(self, leg, B, device, whole):
        self.leg, self.B, self.whole = leg, B, whole
        depth, conf = maps(B, device)
        pose, intr = poses(B, device)
        self.opt = config_opt(CONFIG, "bf16x3", rays=RAND_RAYS, hip=dict(lazy_batch=leg != "series"))
        if whole:
            torch.manual_seed(0)
            self.net = Graph(self.opt, device)
            self.net.train()
            self.net.calls = 0
        else:
            self.net = StandInNet(B, device)
        self.data = edict(image=torch.zeros(B, 3, H, W, device=device), intr=intr, pose=pose, idx=torch.arange(B, device=device),
                          depth_range=torch.tensor([list(SHAPES[CONFIG]["rng"])] * B, dtype=torch.float32, device=device),
                          colmap_depth=depth, colmap_conf=conf)
        self.obj = types.SimpleNamespace(net=self.net, device=device, opt=self.opt)
        self.it, self.report = 0, None

    def iteration(self):
        if self.whole:
            self.net.zero_grad(set_to_none=True)
        self.it += 1
        with leg_context(self.leg):
            loss, stats, _ = losses.compute_colmap_depth_loss(self.obj, self.opt, self.data, {}, self.it, mode="train")
        loss["colmap_depth"].backward()
        self.report = dict(loss=loss["colmap_depth"].detach(), perc_col_depth=stats["perc_col_depth"])

    def result(self):
        return dict(loss=float(self.report["loss"]), perc_col_depth=self.report["perc_col_depth"])


@contextlib.contextmanager
def counters(work):
    """the host readbacks and the render calls of what runs inside"""
    c = dict(where_readbacks=0, item_or_tolist_readbacks=0, render_calls=0, ray_checksum=0)
    real = (torch.where, torch.Tensor.item, torch.Tensor.tolist, work.net.render_image_at_specific_pose_and_rays)
    rays = []

    def where(*a, **k):
        c["where_readbacks"] += len(a) == 1
        return real[0](*a, **k)

    def count(f):
        def g(t, *a, **k):
            c["item_or_tolist_readbacks"] += 1
            return f(t, *a, **k)
        return g

    def render(*a, **k):
        c["render_calls"] += 1
        rays.append(k["ray_idx"])
        return real[3](*a, **k)

    torch.where, torch.Tensor.item, torch.Tensor.tolist = where, count(real[1]), count(real[2])
    work.net.render_image_at_specific_pose_and_rays = render
    before = dict(work.net.lazy_stats)
    try:
        yield c
    finally:
        torch.where, torch.Tensor.item, torch.Tensor.tolist = real[:3]
        work.net.render_image_at_specific_pose_and_rays = real[3]
    c["readbacks"] = c["where_readbacks"] + c["item_or_tolist_readbacks"]
    c["deferred_render_batches"] = work.net.lazy_stats["batches"] - before["batches"]
    c["ray_checksum"] = int(sum(int(r.sum()) for r in rays))
    c["rays_per_render"] = [int(r.numel()) for r in rays]


def traced(work):
    """-> the device activities of ONE iteration (paired_bench.traced): kernels, copies and memsets, and the host waits"""
    t = pb.traced(work.iteration, host=True)
    return dict(kernels=len(t.kernels), copies_and_memsets=len(t.copies), host_waits=len(t.host_waits), host_waits_by_name=t.host_waits)


def measure(works, blocks, iters, warmup):
    ms = pb.device_ms(works, blocks, iters, warmup)
    out = {k: pb.flat(t) for k, t in ms.items()}
    out["result"], out["counts"] = {}, {}
    for k, w in works.items():                                 # the reported iteration: every leg from the same generator state
        torch.manual_seed(0)
        with counters(w) as c:
            w.iteration()
            torch.cuda.synchronize()
        out["result"][k], out["counts"][k] = w.result(), c
    ratio, less, overlap = pb.versus(ms["series"], ms["installed"])
    out.update(installed_over_series=ratio, installed_and_series_blocks_overlap=overlap, series_minus_installed_ms=less)
    return out


def main():
    ap = pb.parser(__doc__, iters=10, warmup=3)
    ap.add_argument("--rows", nargs="+", default=["alone", "whole"], choices=["alone", "whole"])
    ap.add_argument("--batches", nargs="+", type=int, default=[3, 6, 9])
    ap.add_argument("--trace-only", action="store_true", help="trace one iteration of each leg with the profiler; time nothing")
    a = ap.parse_args()
    device = pb.gpu_or_exit("tools/colmap_depth_bench.py")
    rows = {}
    for B in a.batches:
        for kind in a.rows:
            works = {leg: Work(leg, B, device, kind == "whole") for leg in LEGS}
            if a.trace_only:
                for w in works.values():
                    pb.device_block(w, a.warmup)
                rows[f"{kind}_B{B}"] = {leg: traced(w) for leg, w in works.items()}
            else:
                rows[f"{kind}_B{B}"] = measure(works, a.blocks, a.iters * (ALONE_ITERS if kind == "alone" else 1), a.warmup)
    if a.trace_only:
        doc = pb.existing(a.out, dict(tool="tools/colmap_depth_bench.py --trace-only"))
        doc["traced_iteration"] = rows
    else:
        doc = dict(tool="tools/colmap_depth_bench.py", label=a.label, device=torch.cuda.get_device_name(0),
                   workload=f"SparseCOLMAPDepthLoss.compute_loss on B maps of {H} x {W} with a depth at ~2 % of the pixels, rand_rays = {RAND_RAYS}; "
                            "alone_B<B>: with a stand-in render; whole_B<B>: around a real Graph (bf16x3, 64 + 128 samples) with its backward",
                   blocks=a.blocks, iters_per_block=a.iters, alone_iters_per_block=ALONE_ITERS * a.iters, warmup_iters=a.warmup, legs=list(LEGS), rows=rows)
    pb.emit(doc, a.out)


if __name__ == "__main__":
    main()
