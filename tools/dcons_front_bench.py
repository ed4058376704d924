"""The front end of the depth-consistency loss and the trainers' ray sampler, timed two ways.

    python tools/dcons_front_bench.py [--out profiles/dcons_front_bench.json] [--blocks 5] [--iters 20] [--warmup 5]
                                      [--rows alone loss sampler] [--batches 3 6 9] [--trace-only]

Legs.  `series`: what an unmodified trainer runs, restated here in the reference's operations and order -- the [0,0,0,1] row from numpy,
repeat, cat and the batched pose_inverse_4x4 (depth_cons_loss.py:168-174), sample_rays on the CPU with its meshgrid of the whole image
and the synchronous copy of the pixels (:181-185), and sample_pose with its readback of every pose, get_nearest_pose_ids in numpy, the
blend and the two inverses (:45-63); the baseline, never the code under test.  `installed`: the methods install_depth_consistency_sampler()
puts on DepthConsistencyLoss.  Both legs make the same host draws (np.random.randint, the CPU torch.randperm, np.random.rand).
Rows, for B in {3, 6, 9} views of 300 x 400 and 2048 pixels: `alone_B<B>`: the front end alone -- the pose preparation, the pixels and
the unseen pose, no render; `loss_B<B>`: the whole compute_loss around its three real renders (64 + 128 samples, bf16x3), the core
method that of install_depth_consistency() in both legs, with a backward to both networks.  `sampler_<patch>`:
RaySamplingStrategy.__call__ at 2048 rays over 3 views, without and with loss_weight.depth_patch (patch 2): `series` restates the
reference's index operations, `installed` is install_ray_sampler()'s.  The legs of a row run in the alternating blocks of
tools/paired_bench.py, of `--iters` iterations (ten times as many in the rows without a render); per leg ms per iteration as median and
min ... max over the blocks.  After ALL timing ONE iteration of each leg of the rows without a render is traced (paired_bench's
profiler pass): kernels, copies under the profiler's labels, host-to-device copies, readbacks (where they are asked for plus the
device-to-host copies: a readback that shows both ways counts twice).  `cpu_randperm_ms`: the CPU torch.randperm of the pool, which stays in both legs as the
parity contract, timed on the host alone.  `--trace-only` (a run of its own) times nothing: it traces one iteration of each leg of
EVERY row, the `loss_B<B>` rows included -- there the counts hold the renders' and the core method's launches and the two ray-count
readbacks of the core method in both legs; the difference between the legs is the front end's.  One JSON document on stdout and, with
--out, in that file (a --trace-only run adds its key to the rows of the document already there)."""
import os
import sys
import time
import types

import numpy as np
import torch

import paired_bench as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_workloads import SHAPES, cameras, config_opt      # noqa: E402
from sparf_amd import losses                                  # noqa: E402
from sparf_amd.edict import EasyDict as edict                 # noqa: E402
from sparf_amd.renderer import Graph                          # noqa: E402

LEGS = ("series", "installed")
H, W, RAYS, CONFIG, FRACTION = 300, 400, 2048, 1, 0.0
SHORT_ITERS = 10                                               # a block without a render runs this many times --iters: it is short work


# ---- the series leg: the reference's operations
def series_prepare(poses_w2c, device):
    """depth_cons_loss.py:168-174"""
    B = poses_w2c.shape[0]
    bottom = torch.from_numpy(np.array([0, 0, 0, 1])).to(device).reshape(1, 1, -1).repeat(B, 1, 1)
    poses = torch.cat((poses_w2c.detach(), bottom), axis=1)
    return poses, losses._pose_inverse_batched_torch(poses)


def series_nearest(poses_c2w, id_self):
    """data_utils.py:248-311 with one neighbour, 'vector' and the scene centre 0"""
    tar = poses_c2w[id_self][None, ...].repeat(len(poses_c2w), 0)
    centre = np.array((0, 0, 0))[None, ...]
    v1, v2 = tar[:, :3, 3] - centre, poses_c2w[:, :3, 3] - centre
    u1 = v1 / (np.linalg.norm(v1, axis=1, keepdims=True) + 1e-6)
    u2 = v2 / (np.linalg.norm(v2, axis=1, keepdims=True) + 1e-6)
    dists = np.arccos(np.clip(np.sum(u1 * u2, axis=-1), -1.0, 1.0))
    dists[id_self] = 1e3
    return np.argsort(dists)[:1][0]


def series_sample_pose(poses_c2w, id_self, pose_w2c_self):
    """depth_cons_loss.py:45-63"""
    id_other = series_nearest(poses_c2w.detach().cpu().numpy(), id_self)
    w = np.random.rand()
    pose_c2w_self = losses.pose_inverse_4x4_torch(pose_w2c_self).detach()
    return losses.pose_inverse_4x4_torch(w * pose_c2w_self + (1 - w) * poses_c2w[id_other].detach())


def series_compute_loss(self, opt, data_dict, output_dict, iteration, mode=None, plot=False, render=True):
    """depth_cons_loss.py:128-217; `render` False: the front end alone, the reference render left out"""
    B, _, H_, W_ = data_dict.image.shape
    poses_w2c, poses_c2w = series_prepare(data_dict.poses_w2c, self.device)
    id_self = np.random.randint(B)
    pixels_ref, _ = losses.sample_pixels_torch(H_, W_, nbr=max(1024, self.opt.nerf.rand_rays), fraction_in_center=self.opt.sampled_fraction_in_center)
    pixels_ref = pixels_ref.reshape(-1, 2).to(self.device)
    intr_ref, pose_w2c_ref, pose_c2w_ref = data_dict.intr[id_self], poses_w2c[id_self], poses_c2w[id_self]
    if not render:
        return pixels_ref, pose_c2w_ref, series_sample_pose(poses_c2w, id_self, pose_w2c_ref)
    ret_ref = self.net.render_image_at_specific_pose_and_rays(self.opt, data_dict, pose=pose_w2c_ref[:3], intr=intr_ref, H=H_, W=W_, pixels=pixels_ref,
                                                              mode='train', iter=iteration)
    depth_ref = ret_ref.depth_fine.squeeze(0).squeeze(-1)
    points = losses.backproject_to_3d_torch(pixels_ref, depth_ref, intr_ref, pose_c2w_ref)
    unseen = series_sample_pose(poses_c2w, id_self, pose_w2c_ref)
    return self.compute_loss_at_sampled_pose(data_dict, pose_w2c_at_unseen=unseen, intr_at_unseen=intr_ref.clone(), pseudo_gt_3dpts_in_w=points, H=H_, W=W_,
                                             pixels_in_ref=pixels_ref)


def installed_front(self, data_dict):
    """the front end of losses.dcons_compute_loss alone, the reference render left out"""
    B, _, H_, W_ = data_dict.image.shape
    id_self = np.random.randint(B)
    pixels_ref, _ = losses.sample_pixels(H_, W_, nbr=max(1024, self.opt.nerf.rand_rays), fraction_in_center=self.opt.sampled_fraction_in_center,
                                         device=self.device)
    prep = losses.sample_unseen_pose(data_dict.poses_w2c.detach(), id_self, np.random.rand())
    return pixels_ref, prep.pose_c2w_ref, prep.pose_w2c_at_unseen


class SeriesRaySampler:
    """sampling_strategies.py:23-188 without the in-mask pool: the pools as index tensors on the device, and the reference's operations"""

    def __init__(self, opt, B, device):
        self.opt, self.device, self.nbr_images, self.H, self.W = opt, device, B, H, W
        p = opt.depth_regu_patch_size
        if opt.loss_weight.depth_patch is not None:
            ys, xs = torch.arange(H - p - 1, dtype=torch.long, device=device), torch.arange(W - p - 1, dtype=torch.long, device=device)
        else:
            ys, xs = torch.arange(H, dtype=torch.long, device=device), torch.arange(W, dtype=torch.long, device=device)
        Y, X = torch.meshgrid(ys, xs, indexing="ij")
        self.all_possible_pixels = torch.stack([X, Y], dim=-1).view(-1, 2).long()
        dH, dW = int(H // 2 * opt.precrop_frac), int(W // 2 * opt.precrop_frac)
        Y, X = torch.meshgrid(torch.linspace(H // 2 - dH, H // 2 + dH - 1, 2 * dH), torch.linspace(W // 2 - dW, W // 2 + dW - 1, 2 * dW), indexing="ij")
        self.all_center_pixels = torch.stack([X, Y], -1).view(-1, 2).long().to(device)
        r = torch.arange(p, dtype=torch.long, device=device)
        Y, X = torch.meshgrid(r, r, indexing="ij")
        self.dxdy = torch.stack([X, Y], dim=-1).view(-1, 2)

    def __call__(self, nbr_pixels, sample_in_center=False, idx_imgs=None):
        p = self.opt.depth_regu_patch_size
        n = nbr_pixels // self.nbr_images
        if self.opt.loss_weight.depth_patch is not None:
            n = n // p ** 2
        centre = None
        if self.opt.sampled_fraction_in_center > 0:
            n_c = int(n * self.opt.sampled_fraction_in_center)
            n = n - n_c
            centre = self.all_center_pixels[torch.randperm(len(self.all_center_pixels), device=self.device)[:n_c]]
        pool = self.all_center_pixels if sample_in_center else self.all_possible_pixels
        pixels = pool[torch.randperm(len(pool), device=self.device)[:n]]
        if centre is not None:
            pixels = torch.cat((pixels, centre), dim=0)
        if self.opt.loss_weight.depth_patch is not None:
            x = (pixels[:, 0][:, None].repeat(1, p ** 2) + self.dxdy[:, 0]).reshape(-1)
            y = (pixels[:, 1][:, None].repeat(1, p ** 2) + self.dxdy[:, 1]).reshape(-1)
            pixels = torch.stack([x, y], dim=-1).reshape(-1, p ** 2, 2).reshape(-1, 2)
        return pixels[..., 1] * self.W + pixels[..., 0]


# ---- the work of a leg
class Work:
    def __init__(self, leg, kind, B, device, patch=None):
        self.leg, self.kind, self.B, self.device = leg, kind, B, device
        pose, intr = cameras(CONFIG, device)
        idx = [b % pose.shape[0] for b in range(B)]
        self.data = edict(idx=torch.arange(B), image=torch.zeros(B, 3, H, W, device=device), intr=intr[idx].contiguous(), poses_w2c=pose[idx].contiguous(),
                          depth_range=torch.tensor([list(SHAPES[CONFIG]["rng"])] * B, dtype=torch.float32, device=device), iter=0)
        self.counts, self.value = [], None
        if kind == "sampler":
            opt = edict(sample_fraction_in_fg_mask=0., sampled_fraction_in_center=FRACTION, precrop_frac=0.5, depth_regu_patch_size=2,
                        loss_weight=edict(depth_patch=None if patch is None else 1.0))
            self.sampler = SeriesRaySampler(opt, B, device)
            return
        self.obj = types.SimpleNamespace(device=device, opt=None, net=None)
        opt = config_opt(CONFIG, "bf16x3", rays=RAYS)
        if kind == "loss":
            torch.manual_seed(0)
            self.obj.net = Graph(opt, device)
            self.obj.net.train()
        self.obj.opt = edict(opt)
        self.obj.opt.update(diff_loss_type="huber", gradually_decrease_depth_cons_loss=False, depth_cons_loss_reduct_at_x_iter=10000, sampled_fraction_in_center=FRACTION,
                            start_ratio=edict(depth_cons=None), start_iter=edict(depth_cons=0), max_iter=1000)
        self.obj.compute_loss_at_sampled_pose = lambda data, **kw: self.core(data, **kw)

    def core(self, data, **kw):
        self.counts.append(int(kw["pixels_in_ref"].shape[0]))
        return losses.compute_loss_at_sampled_pose(self.obj, data, **kw)

    def iteration(self):
        if self.kind == "sampler":
            # (installed: the function install_ray_sampler() puts on the class, on the same instance)
            self.value = self.sampler(RAYS) if self.leg == "series" else losses.ray_sampler_call(self.sampler, RAYS)
        elif self.kind == "alone":
            self.value = series_compute_loss(self.obj, self.obj.opt, self.data, {}, 0, render=False) if self.leg == "series" else installed_front(self.obj, self.data)
        else:
            G = self.obj.net
            G.zero_grad(set_to_none=True)
            fn = series_compute_loss if self.leg == "series" else losses.dcons_compute_loss
            loss = fn(self.obj, self.obj.opt, self.data, {}, 0, mode="train")[0]["depth_cons"]
            if loss.requires_grad and loss.grad_fn is not None:
                loss.backward()
            self.value = loss.detach()


def traced(work):
    """-> the device activities of ONE iteration (paired_bench.traced); a readback counts where it is asked for AND as its copy"""
    np.random.seed(1)                                          # the same draws in every leg: the same view, pixels and blend
    torch.manual_seed(1)
    t = pb.traced(work.iteration, host=True)
    return dict(launches=len(t.kernels), copies_and_memsets=len(t.copies), copies_by_label=t.copies_by_label, host_to_device_copies=t.host_to_device,
                readbacks=t.readbacks_asked + t.readbacks_by_label)


def measure(works, blocks, iters, warmup, trace):
    ms = pb.device_ms(works, blocks, iters, warmup)
    out = {k: pb.flat(t) for k, t in ms.items()}
    ratio, less, overlap = pb.versus(ms["series"], ms["installed"])
    out.update(series_minus_installed_ms=less, installed_over_series=ratio, blocks_overlap=overlap)
    for k, w in works.items():
        if w.counts:                                           # the pixels that entered the core method: the three renders ran
            out[k]["pixels_into_the_core_min_max"] = [min(w.counts), max(w.counts)]
    if trace is not None:                                      # traced behind all timing: tracing slows the host
        trace.append((out, works))
    return out


def trace_only(a, device):
    """a run of its own (tracing slows the host): ONE traced iteration of each leg of EVERY row, the rows around the renders included
    (their counts hold the renders' and the core method's launches in both legs); adds `traced_iteration` to the rows of the document
    already at --out"""
    doc = pb.existing(a.out, dict(tool="tools/dcons_front_bench.py --trace-only", rows={}))
    names = {}
    for kind in a.rows:
        if kind == "sampler":
            names.update({f"sampler_{'no_patch' if p is None else 'depth_patch_2'}": (kind, 3, p) for p in (None, 2)})
        else:
            names.update({f"{kind}_B{B}": (kind, B, None) for B in a.batches})
    for name, (kind, B, patch) in names.items():
        works = {leg: Work(leg, kind, B, device, patch) for leg in LEGS}
        for w in works.values():
            pb.device_block(w, a.warmup)
        doc["rows"].setdefault(name, {})["traced_iteration"] = {leg: traced(w) for leg, w in works.items()}
    pb.emit(doc, a.out)


def cpu_randperm_ms(n_pool, n, iters=200):
    for _ in range(10):
        torch.randperm(n_pool)[:n]
    t0 = time.perf_counter()
    for _ in range(iters):
        torch.randperm(n_pool)[:n]
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = pb.parser(__doc__)
    ap.add_argument("--rows", nargs="+", default=["alone", "loss", "sampler"], choices=["alone", "loss", "sampler"])
    ap.add_argument("--batches", nargs="+", type=int, default=[3, 6, 9])
    ap.add_argument("--trace-only", action="store_true", help="trace one iteration of each leg of every row with the profiler; time nothing")
    a = ap.parse_args()
    device = pb.gpu_or_exit("tools/dcons_front_bench.py")
    np.random.seed(0)
    torch.manual_seed(0)
    rows, to_trace = {}, []
    if a.trace_only:
        trace_only(a, device)
        return
    for kind in a.rows:
        if kind == "sampler":
            for patch in (None, 2):
                works = {leg: Work(leg, kind, 3, device, patch) for leg in LEGS}
                rows[f"sampler_{'no_patch' if patch is None else 'depth_patch_2'}"] = measure(works, a.blocks, a.iters * SHORT_ITERS, a.warmup, to_trace)
            continue
        for B in a.batches:
            works = {leg: Work(leg, kind, B, device) for leg in LEGS}
            rows[f"{kind}_B{B}"] = measure(works, a.blocks, a.iters * (SHORT_ITERS if kind == "alone" else 1), a.warmup, to_trace if kind == "alone" else None)
    for out, works in to_trace:
        out["traced_iteration"] = {k: traced(w) for k, w in works.items()}
    doc = dict(tool="tools/dcons_front_bench.py", label=a.label, device=torch.cuda.get_device_name(0),
               workload=f"DepthConsistencyLoss.compute_loss on B views of {H} x {W}, {RAYS} pixels, centre fraction {FRACTION}: alone_B<B> its front end alone, "
                        "loss_B<B> the whole loss around its three renders (bf16x3, 64 + 128 samples) with its backward; sampler_*: "
                        f"RaySamplingStrategy.__call__ at {RAYS} rays over 3 views",
               blocks=a.blocks, iters_per_block=a.iters, short_iters_per_block=SHORT_ITERS * a.iters, warmup_iters=a.warmup, legs=list(LEGS),
               cpu_randperm_ms=dict(pool=(H - 1) * (W - 1), picks=RAYS, ms_per_draw=cpu_randperm_ms((H - 1) * (W - 1), RAYS)), rows=rows)
    pb.emit(doc, a.out)


if __name__ == "__main__":
    main()
