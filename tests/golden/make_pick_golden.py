"""Generate tests/golden/pick.npz: what the REFERENCE's own sample_rays, sample_rays_for_patch, RaySamplingStrategy.__call__
(source/training/core/sampling_strategies.py) and DepthConsistencyLoss.sample_pose (source/training/core/depth_cons_loss.py:45-63) did (CPU)
on the cases of tests/pick_referee.py (tests/test_pick_cpu.py, tests/test_pick_gpu.py).

Runs only where the reference is importable (through tests/ref_harness.install_reference()): the committed file holds arrays only.  Every
function is called unmodified under seeded generators; what it drew is seen by a wrapper around torch.randperm that calls the real one,
and the camera it chose by one around the module's get_nearest_pose_ids.  Nothing of the functions is restated.  Per pixel case
<name>/perm and perm_center (the drawn prefixes; absent where nothing was drawn), pixels float32 and rays int64 (the reference leaves
float32 rays behind a centre fraction: the same integers, checked here); per strategy case <name>/draw0, draw1 (the full permutations in
draw order) and rays; per pose case <name>/poses_w2c, id_self, w (float64), id_other and the four matrices.  The poses in front of
sample_pose are prepared by the reference's own pose_inverse_4x4, as depth_cons_loss.py:168-174 does."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat")]

from tests import ref_harness                                           # noqa: E402
from tests import pick_referee as R                                     # noqa: E402

assert ref_harness.install_reference(), "the reference tree is not importable"
from easydict import EasyDict as edict                                  # noqa: E402
import source.training.core.sampling_strategies as ref_sampling        # noqa: E402
import source.training.core.depth_cons_loss as ref_dcons               # noqa: E402
from source.utils.camera import pose_inverse_4x4                       # noqa: E402


class Draws:
    """every torch.randperm result while it is open, in order"""

    def __enter__(self):
        self.seen, self.real = [], torch.randperm

        def randperm(n, **kw):
            v = self.real(n, **kw)
            self.seen.append(v.clone())
            return v
        torch.randperm = randperm
        return self.seen

    def __exit__(self, *exc):
        torch.randperm = self.real


def run_pixel_case(case):
    torch.manual_seed(case["seed"])
    kw = dict(precrop_frac=R.PRECROP, fraction_in_center=case["fraction"], nbr=case["nbr"])
    with Draws() as seen:
        if case["patch"] is None:
            pixels, rays = ref_sampling.sample_rays(case["H"], case["W"], **kw)
        else:
            pixels, rays = ref_sampling.sample_rays_for_patch(case["H"], case["W"], case["patch"], **kw)
    out = {}
    if case["nbr"] is not None:
        n_all, n_center = R.counts_of(case)
        assert len(seen) == (2 if case["fraction"] > 0 else 1)
        out["perm"] = seen[0][:n_all].numpy()
        if len(seen) == 2:
            out["perm_center"] = seen[1][:n_center].numpy()
    else:
        assert not seen
    assert pixels.dtype == torch.float32 and torch.equal(rays.double(), rays.double().round())
    out["pixels"], out["rays"] = pixels.numpy(), rays.to(torch.int64).numpy()
    return out


def strategy_opt(case):
    return edict(sample_fraction_in_fg_mask=0., sampled_fraction_in_center=case["fraction"], precrop_frac=R.PRECROP,
                 depth_regu_patch_size=case["patch"] or 2, loss_weight=edict(depth_patch=None if case["patch"] is None else 1.0))


def run_strategy_case(case):
    torch.manual_seed(case["seed"])
    data = edict(image=torch.zeros(case["B"], 3, case["H"], case["W"]))
    sampler = ref_sampling.RaySamplingStrategy(strategy_opt(case), data, torch.device("cpu"))
    with Draws() as seen:
        rays = sampler(case["nbr_pixels"], sample_in_center=case["in_center"], idx_imgs=case["idx_imgs"])
    assert len(seen) == (2 if case["fraction"] > 0 else 1) and rays.dtype == torch.int64
    out = {f"draw{i}": v.numpy() for i, v in enumerate(seen)}
    out["rays"] = rays.numpy()
    return out


def run_pose_case(B, id_self, three_by_four, seed):
    poses = R.poses_of(B, seed, three_by_four)
    p = torch.from_numpy(poses)
    if three_by_four:                                                    # depth_cons_loss.py:168-173
        bottom = torch.from_numpy(np.array([0, 0, 0, 1])).reshape(1, 1, -1).repeat(B, 1, 1)
        p = torch.cat((p, bottom), axis=1)
    poses_c2w = pose_inverse_4x4(p)
    assert p.dtype == torch.float32 and poses_c2w.dtype == torch.float32
    g = R.gap(poses_c2w[:, :3, 3].numpy(), id_self)
    assert g >= R.MIN_GAP, (B, seed, g)
    chosen, real = [], ref_dcons.get_nearest_pose_ids

    def watched(*a, **k):
        ids = real(*a, **k)
        chosen.append(int(ids[0]))
        return ids
    loss = object.__new__(ref_dcons.DepthConsistencyLoss)               # sample_pose reads nothing of the instance
    ref_dcons.get_nearest_pose_ids = watched
    try:
        np.random.seed(seed)
        unseen = loss.sample_pose(poses_c2w, id_self, p[id_self])
    finally:
        ref_dcons.get_nearest_pose_ids = real
    w = np.random.RandomState(seed).rand()                               # the same stream: what sample_pose drew
    assert len(chosen) == 1 and unseen.dtype == torch.float32
    print("   gap", g, "id_other", chosen[0], "w", w)
    return dict(poses_w2c=poses, id_self=np.int64(id_self), w=np.float64(w), id_other=np.int64(chosen[0]), pose_w2c_ref=p[id_self].numpy(),
                pose_c2w_ref=poses_c2w[id_self].numpy(), pose_c2w_other=poses_c2w[chosen[0]].numpy(), pose_w2c_at_unseen=unseen.numpy())


def main():
    arrays = {}
    for name, case in R.pixel_cases().items():
        res = run_pixel_case(case)
        arrays.update({f"{name}/{k}": v for k, v in res.items()})
        print(name, res["pixels"].shape, res["rays"].shape)
    for name, case in R.strategy_cases().items():
        res = run_strategy_case(case)
        arrays.update({f"{name}/{k}": v for k, v in res.items()})
        print(name, res["rays"].shape)
    for name, spec in R.POSE_CASES.items():
        print(name)
        arrays.update({f"{name}/{k}": v for k, v in run_pose_case(*spec).items()})
    np.savez_compressed(R.FIXTURE, **arrays)
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
