"""Generate tests/golden/colmap.npz: what the REFERENCE's own SparseCOLMAPDepthLoss.compute_loss did (CPU) on the cases of
tests/colmap_referee.py (tests/test_colmap_cpu.py).

Runs only where the reference is importable (through tests/ref_harness.install_reference()): the committed file holds arrays only.
Every case constructs the reference's unmodified class with tests/colmap_fake.DepthNet as its `net` -- a render that is an exact
function of the image and of ray_idx, and that records every ray list it is asked for -- and calls compute_loss under torch.no_grad():
the method adds in place to a leaf that requires grad (base_losses.py:368, :393), which autograd refuses on CPU tensors.  Nothing of the
method is restated.  Per case and seed: rays_<b> (the ray list of the render of image b; absent for an image without a render),
rendered (the images rendered, in call order), loss (float32), perc (float64) and rng (torch's CPU generator state after the call)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat")]

from tests import ref_harness                                           # noqa: E402
from tests import colmap_referee as R                                   # noqa: E402
from tests.colmap_fake import DepthNet                                  # noqa: E402

assert ref_harness.install_reference(), "the reference tree is not importable"
from easydict import EasyDict as edict                                  # noqa: E402
from source.training.core.base_losses import SparseCOLMAPDepthLoss     # noqa: E402


def build_case(H, W, fine=True):
    """the reference's module on the maps of a shape, and the opt and data_dict of the call"""
    depth, conf = R.maps_of(H, W)
    opt = edict(nerf=edict(rand_rays=R.RAND_RAYS))
    net = DepthNet(R.B, fine=fine)
    obj = SparseCOLMAPDepthLoss(opt, net, torch.device("cpu"))
    data = edict(image=torch.zeros(R.B, 3, H, W), intr=torch.eye(3).repeat(R.B, 1, 1), colmap_depth=torch.from_numpy(depth),
                 colmap_conf=torch.from_numpy(conf), idx=torch.arange(R.B))
    return obj, opt, data


def run_case(H, W, seed):
    obj, opt, data = build_case(H, W)
    torch.manual_seed(seed)
    with torch.no_grad():
        loss, stats, plots = obj.compute_loss(opt, data, {}, 0, mode="train")
    assert sorted(loss) == ["colmap_depth"] and sorted(stats) == ["perc_col_depth"] and plots == {}
    out = dict(loss=loss["colmap_depth"].numpy().astype(np.float32), perc=np.float64(stats["perc_col_depth"]), rng=torch.get_rng_state().numpy())
    rendered = [b for b, v in enumerate(R.select_np(data.colmap_depth.numpy(), data.colmap_conf.numpy(), R.RAND_RAYS,
                                                    [np.arange(H * W)] * R.B)["valid"]) if v]
    assert len(rendered) == len(obj.net.calls)
    out["rendered"] = np.array(rendered, dtype=np.int32)
    for b, rays in zip(rendered, obj.net.calls):
        out[f"rays_{b}"] = rays.numpy()
    return out


def main():
    out = {}
    for H, W in R.SHAPES:
        for seed in R.SEEDS:
            case = run_case(H, W, seed)
            out.update({f"{R.case_name(H, W)}/{seed}/{k}": v for k, v in case.items()})
            print(R.case_name(H, W), seed, "renders of", [len(case[f"rays_{b}"]) for b in case["rendered"]], "rays, loss", float(case["loss"]),
                  "perc", float(case["perc"]))
    np.savez_compressed(R.FIXTURE, **out)
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
