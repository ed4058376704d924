"""Pose evaluation and the test-time pose chain, timed two ways.

    python tools/pose_eval_bench.py [--out profiles/pose_eval_bench.json] [--blocks 5] [--iters 20] [--loop-iters 10] [--warmup 3]
    python tools/pose_eval_bench.py --trace-only --out profiles/pose_eval_bench.json      (a run of its own: adds the counts)

Legs.  `series`: the torch restatement of sparf_amd.pose_eval under its unfused() (and sparf_amd.camera's) -- the reference's literal pair
loop with its four readbacks per candidate, its backtrack and its compose: what an unmodified trainer runs; the baseline, never the code
under test.  `fused`: the installed methods -- one sparf_pose_eval launch, one sparf_pose_backtrack launch, the compose kernel.
Rows.  `evaluate_B3 / B6 / B9`: CommonPoseEvaluation.evaluate_any_poses (joint_pose_nerf_trainer.py:290-311) on B noisy views under a
random similarity, and the readback of its four values as the logger makes it.  `chain_alone`: Graph.get_w2c_pose in mode test-optim
(:728-739) at one pose: backtrack_from_aligning_the_trajectory, then camera.pose.compose with the refinement, no readback.
`chain_in_loop`: the same chain inside the test-time optimisation loop of tools/pose_optim_bench.py's view (4096 rays, 64 + 128
samples, bf16x3, the full route), called twice per iteration as the trainer does (:394 and :397), se3_to_SE3 on its kernel in both legs.
The legs of a row run in the alternating blocks of tools/paired_bench.py.  Per leg: device ms per call as median and min ... max over
the blocks, and whether the legs' ranges overlap.
--trace-only, in a run of its own: the kernels, copies and readbacks (device-to-host copies, by label) of ONE call of each row but the
loop (paired_bench's profiler pass), merged into the document of --out; `item_calls_in_code` adds the series' `.item()` synchronisations, which the trace does
not list as device copies, counted from its code.  One JSON line on stdout per run and, with --out, the document in that file."""
import contextlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat"), os.path.join(ROOT, "tools")]
import paired_bench as pb                                                      # noqa: E402
from sparf_amd import camera, pose_eval                                        # noqa: E402
from sparf_amd.edict import EasyDict as edict                                  # noqa: E402

LEGS = ("series", "fused")
VIEWS = (3, 6, 9)


class Trainer:
    """a stand-in for CommonPoseEvaluation: what the methods read of it"""

    def __init__(self, device):
        self.settings = edict(camera=edict(n_first_fixed_poses=1))
        self.device = device


for _name in pose_eval.METHODS:                                                # the installed methods, on the stand-in (install() is for a trainer's class)
    setattr(Trainer, _name, getattr(pose_eval, _name))


def poses(B, device, noise=0.05, seed=0):
    """B ground-truth world-to-camera poses and their noisy copies under a random similarity, seeded"""
    g = torch.Generator().manual_seed(seed + B)
    rnd = lambda *s: torch.randn(*s, generator=g)
    gt_c2w = camera.se3_to_SE3_torch(torch.cat([rnd(B, 3), 2 * rnd(B, 3)], -1))
    noisy = camera.compose_pair_torch(camera.se3_to_SE3_torch(noise * rnd(B, 6)), gt_c2w)
    sim = camera.se3_to_SE3_torch(rnd(1, 6))
    est = camera.compose_pair_torch(noisy, sim.expand(B, 3, 4)).clone()
    est[..., 3] *= 1.7
    return camera.invert_pose(est).to(device).contiguous(), camera.invert_pose(gt_c2w).to(device).contiguous()


def leg_context(leg):
    stack = contextlib.ExitStack()
    if leg == "series":
        stack.enter_context(pose_eval.unfused())
        stack.enter_context(camera.unfused())
    return stack


class Evaluate:
    def __init__(self, leg, B, device):
        self.leg, self.trainer = leg, Trainer(device)
        self.pose, self.gt = poses(B, device)
        # the series' `.item()` readbacks, counted from its code (four per candidate, :245-247): the trace does not list them as device copies
        self.item_calls = 4 * pose_eval.n_pairs(B) if leg == "series" else 0

    def iteration(self):
        with leg_context(self.leg):
            stats = self.trainer.evaluate_any_poses(None, self.pose, self.gt)
        return torch.stack(list(stats.values())).tolist()                      # the logger's readback


def similarity(device):
    pose, gt = poses(9, device)
    return pose_eval.evaluate_poses(pose, gt).sim3, gt


class ChainAlone:
    def __init__(self, leg, device):
        self.leg = leg
        self.sim3, gt = similarity(device)
        self.test_gt = gt[:1].contiguous()
        self.refine = camera.se3_to_SE3_torch(torch.tensor([[0.01, -0.02, 0.005, 0.03, 0.01, -0.02]])).to(device)

    def iteration(self):
        with leg_context(self.leg):
            return camera.pose.compose([self.refine, pose_eval.backtrack(self.test_gt, self.sim3)])


def chain_in_loop(leg, device):
    from pose_optim_bench import PoseView

    class ChainView(PoseView):
        def __init__(self):
            super().__init__("bf16x3", False, device, "fused")
            # the ground-truth test pose whose backtrack under the similarity is the view's own pose: the loop optimises what pose_optim_bench's does
            self.sim3, _ = similarity(device)
            R, t, s = self.sim3.R[0], self.sim3.t[0], self.sim3.s
            own = camera.invert_pose(self.pose0.detach())
            self.test_gt = camera.invert_pose(torch.cat([R @ own[..., :3], s * (R @ own[..., 3:]) + t], dim=-1)).contiguous()

        def pose(self):
            refine = camera.lie.se3_to_SE3(self.xi)
            with leg_context(leg):
                first = camera.pose.compose([refine, pose_eval.backtrack(self.test_gt, self.sim3)])      # :394, net.forward
                camera.pose.compose([refine, pose_eval.backtrack(self.test_gt, self.sim3)])              # :397, get_pose
            return first

    return ChainView()


def launches(work):
    """the device activities of ONE iteration (paired_bench.traced) -> dict(kernels, copies_and_memsets, readbacks by label, ...)"""
    work.iteration()
    t = pb.traced(work.iteration)
    return dict(kernels=len(t.kernels), copies_and_memsets=len(t.copies), readbacks=t.readbacks_by_label,
                copy_kinds={x: t.copies.count(x) for x in dict.fromkeys(t.copies)}, item_calls_in_code=getattr(work, "item_calls", 0))


def measure(works, blocks, iters, warmup):
    dev = pb.device_ms(works, blocks, iters, warmup)
    out = {k: dict(device_ms_per_call=pb.summary(dev[k])) for k in works}
    out["fused_over_series_device"], out["series_minus_fused_device_ms"], out["blocks_overlap"] = pb.versus(dev["series"], dev["fused"])
    return out


def main():
    ap = pb.parser(__doc__, warmup=3)
    ap.add_argument("--rows", nargs="+", default=["evaluate", "chain", "loop"], choices=["evaluate", "chain", "loop"])
    ap.add_argument("--loop-iters", type=int, default=10)
    ap.add_argument("--trace-only", action="store_true", help="only the launch counts of the evaluate and chain rows, merged into the document of --out")
    a = ap.parse_args()
    device = pb.gpu_or_exit("tools/pose_eval_bench.py")
    if a.trace_only:
        doc = pb.existing(a.out, dict(tool="tools/pose_eval_bench.py", rows={}))
        for B in VIEWS:
            doc["rows"].setdefault(f"evaluate_B{B}", {})["launches_per_call"] = {leg: launches(Evaluate(leg, B, device)) for leg in LEGS}
        doc["rows"].setdefault("chain_alone", {})["launches_per_call"] = {leg: launches(ChainAlone(leg, device)) for leg in LEGS}
    else:
        rows = {}
        if "evaluate" in a.rows:
            for B in VIEWS:
                works = {leg: Evaluate(leg, B, device) for leg in LEGS}
                rows[f"evaluate_B{B}"] = dict(measure(works, a.blocks, a.iters, a.warmup), values={leg: w.iteration() for leg, w in works.items()})
        if "chain" in a.rows:
            works = {leg: ChainAlone(leg, device) for leg in LEGS}
            rows["chain_alone"] = dict(measure(works, a.blocks, a.iters, a.warmup), values={leg: w.iteration().reshape(-1).tolist() for leg, w in works.items()})
        if "loop" in a.rows:
            works = {leg: chain_in_loop(leg, device) for leg in LEGS}
            rows["chain_in_loop"] = measure(works, a.blocks, a.loop_iters, a.warmup)
        doc = dict(tool="tools/pose_eval_bench.py", label=a.label, device=torch.cuda.get_device_name(0),
                   workload="evaluate_any_poses on 3, 6 and 9 views with the readback of its four values; backtrack + compose at one pose, alone and twice "
                            "per iteration of the test-time pose optimisation loop (4096 rays, 64 + 128 samples, bf16x3, full route)",
                   blocks=a.blocks, calls_per_block=a.iters, loop_iters_per_block=a.loop_iters, warmup_calls=a.warmup,
                   legs=dict(series="the torch restatement under pose_eval.unfused() and camera.unfused(): the reference's pair loop, backtrack and compose",
                             fused="sparf_pose_eval / sparf_pose_backtrack / the compose kernel"), rows=rows)
    pb.emit(doc, a.out, one_line=True)                         # one line per run


if __name__ == "__main__":
    main()
