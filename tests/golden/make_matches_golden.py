"""Generate tests/golden/matches.npz: what the REFERENCE's own correspondence sampler did (CPU) on the cases of
tests/matches_referee.py FIXTURE_CASES (tests/test_matches_cpu.py, tests/test_matches_gpu.py).

Runs only where the reference is importable (through tests/ref_harness.install_reference()): the committed file holds arrays only.
Every case constructs the reference's unmodified CorrespondencesPairRenderDepthAndGet3DPtsAndReproject with tests/ref_harness.SphereFlowNet
as its flow network (two views of the unit sphere) and calls its compute_loss_pairwise -> compute_loss_at_given_img_indexes ->
compute_loss_on_image_pair chain.  A `sphere` case keeps the maps compute_correspondences stored; a pattern case replaces them by
matches_referee.mask_of / maps_of before the call.  What the chain did is observed from outside, nothing of it is restated:
  * `self.net` is a stand-in whose render records the `pixels` it is asked for and returns constant depths;
  * torch.randperm is wrapped and its result recorded;
  * ray_in_self_int / ray_in_other_int never leave the method, but with compute_photo_on_matches the method gathers the images by them
    (corres_loss.py:170-171): the images hold every pixel's flat index in channel 0, and a recording MSE_loss keeps what was gathered;
  * conf_values is an argument of compute_render_and_repro_loss_w_repro_thres, which is replaced by a recorder;
  * perc_valid_corr_mask comes back in stats_dict.
Per case: mask [H,W] bool, window (4 ints, or empty), perm (the first MAX_MATCHES entries of the permutation drawn, all that is read
of it; or empty), pixels_self / pixels_other [k,2], ray_self / ray_other [k],
conf_values [k,1], perc, rendered (the number of render calls: 0 below min_nbr_matches); corres [2,H,W] and conf [1,H,W] for the sphere
cases only (the others' are matches_referee.maps_of)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat")]

from tests import ref_harness                                           # noqa: E402
from tests import matches_referee as R                                  # noqa: E402

assert ref_harness.install_reference(), "the reference tree is not importable"
from easydict import EasyDict as edict                                  # noqa: E402
from source.training.core.corres_loss import CorrespondencesPairRenderDepthAndGet3DPtsAndReproject as Corres   # noqa: E402

PRECROP_ITERS = 100


def two_views(H, W):
    """w2c poses [2,3,4] of two cameras 3 units from the origin, 0.15 rad to either side, and their intrinsics [2,3,3]"""
    poses = []
    for a in (-0.15, 0.15):
        c2w = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])
        centre = np.array([3 * np.sin(a), 0, -3 * np.cos(a)])
        Rw = c2w.T
        poses.append(np.c_[Rw, -Rw @ centre])
    f = 1.2 * min(H, W)
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    return torch.tensor(np.stack(poses), dtype=torch.float32), torch.tensor(np.stack([K, K]), dtype=torch.float32)


class RecordingNet:
    def __init__(self):
        self.pixels = []

    def render_image_at_specific_pose_and_rays(self, opt, data_dict, pose, intr, H, W, pixels=None, mode=None, iter=None):
        self.pixels.append(pixels.clone())
        n = pixels.shape[0]
        return edict(rgb=torch.zeros(1, n, 3), depth=torch.full((1, n, 1), 3.0), opacity=torch.ones(1, n, 1))


def build_case(name, net, compute_photo=True):
    """the reference's module for a case of FIXTURE_CASES, constructed by its own __init__, and the data_dict of the call"""
    H, W, source, precrop, min_nbr = R.FIXTURE_CASES[name]
    pose, intr = two_views(H, W)
    index_image = torch.zeros(2, 3, H, W)
    index_image[:, 0] = torch.arange(H * W, dtype=torch.float32).reshape(H, W)          # exact: H W < 2^24
    train_data = edict(all=edict(idx=torch.arange(2), image=index_image, intr=intr, pose=pose))
    opt = edict(min_nbr_matches=1, use_homography_flow=False, precrop_iters=PRECROP_ITERS, precrop_frac=R.PRECROP_FRAC, start_iter=edict(corres=0),
                nerf=edict(rand_rays=2 * R.MAX_MATCHES), compute_photo_on_matches=compute_photo, gradually_decrease_corres_weight=False)
    obj = Corres(opt, net, ref_harness.SphereFlowNet(pose, intr, H, W, (0.0, 0.0, 0.0)), train_data, torch.device("cpu"))
    obj.opt.min_nbr_matches = min_nbr
    if source != "sphere":
        corres, conf = R.maps_of(H, W)
        obj.corres_maps, obj.conf_maps = torch.from_numpy(corres)[None], torch.from_numpy(conf)[None]
        obj.mask_valid_corr = torch.from_numpy(R.mask_of(H, W, source))[None, None]
        obj.filtered_flow_pairs = [(0, 0, 1)]
    assert len(obj.filtered_flow_pairs) == 1, (name, obj.filtered_flow_pairs)
    data_dict = edict(image=index_image, intr=intr, poses_w2c=pose, iter=0 if precrop else 2 * PRECROP_ITERS)
    return obj, data_dict


def run_case(name):
    H, W, source, precrop, min_nbr = R.FIXTURE_CASES[name]
    net = RecordingNet()
    obj, data_dict = build_case(name, net)
    gathered, confs, perms = [], [], []
    obj.MSE_loss = lambda pred, label: (gathered.append(label.clone()), torch.zeros(()))[1]
    obj.compute_render_and_repro_loss_w_repro_thres = lambda *a, **k: (confs.append(a[8].clone()), (torch.zeros(()), a[9]))[1]
    real_randperm = torch.randperm

    def randperm(n, **kw):
        perms.append(real_randperm(n, **kw))
        return perms[-1]

    torch.randperm = randperm
    try:
        with torch.no_grad():                            # (render_matches is accumulated in place on a leaf, corres_loss.py:179)
            loss_dict, stats, _ = obj.compute_loss_pairwise(obj.opt, data_dict, {}, data_dict.iter, mode="train")
    finally:
        torch.randperm = real_randperm
    i = obj.filtered_flow_pairs[0][0]
    out = dict(mask=obj.mask_valid_corr[i, 0].numpy(), window=np.array(R.precrop_window(H, W) if precrop else [], dtype=np.int32),
               perm=perms[0][:R.MAX_MATCHES].numpy() if perms else np.zeros(0, dtype=np.int64), rendered=np.int32(len(net.pixels)))
    if source == "sphere":
        out.update(corres=obj.corres_maps[i].numpy(), conf=obj.conf_maps[i].numpy())
    if net.pixels:
        assert len(net.pixels) == 2 and len(gathered) == 2 and len(confs) == 2 and len(perms) <= 1, name
        out.update(pixels_self=net.pixels[0].numpy(), pixels_other=net.pixels[1].numpy(), ray_self=gathered[0][:, 0].long().numpy(),
                   ray_other=gathered[1][:, 0].long().numpy(), conf_values=confs[0].numpy(), perc=stats["perc_valid_corr_mask"].numpy())
        assert out["perc"].dtype == np.float32 and out["pixels_self"].dtype == np.float32 and out["conf_values"].shape == (len(out["ray_self"]), 1)
    else:
        assert stats == {} and not perms, name
    return out


def main():
    torch.manual_seed(20269)
    np.random.seed(20269)
    out = {}
    for name in R.FIXTURE_CASES:
        case = run_case(name)
        out.update({f"{name}/{k}": v for k, v in case.items()})
        print(f"{name}: {int(case['mask'].sum())} valid, {len(case.get('ray_self', []))} rendered rows, perm drawn: {len(case['perm']) > 0}")
    np.savez_compressed(R.FIXTURE, **out)
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
