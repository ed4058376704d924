"""Generate tests/golden/photo_regu.npz: the image set and the REFERENCE's own fp32 results (CPU) for the photometric / mask / depth-patch
kernel (tests/test_photo_cpu.py, tests/test_photo_gpu.py; names, sizes and cases: tests/photo_referee.py).

Runs only where the reference is importable (through tests/ref_harness.install_reference()): the committed file holds arrays only.
The values come from the reference's UNMODIFIED BasePhotoandReguLoss.compute_loss (on an instance made without its constructor) and
compute_mse_on_rays, and from autograd on them: the gradient of each term to its own tensor.

Conditions, asserted here for every case: at most 1 % of a case's colour elements were redrawn for lying within 1e-3 of the Huber kink,
none lies there now, and the side of the kink agrees between the fp32 difference and the float64 one.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat")]

from tests import ref_harness                                           # noqa: E402
from tests import photo_referee as R                                    # noqa: E402

assert ref_harness.install_reference(), "the reference tree is not importable"
from easydict import EasyDict as edict                                  # noqa: E402
from source.training.core.base_losses import BasePhotoandReguLoss       # noqa: E402
from source.training.core.metrics import compute_mse_on_rays            # noqa: E402


def T(a, grad=False):
    return torch.from_numpy(np.array(a)).requires_grad_(grad) if a is not None else None


def reference_run(x):
    """the reference's two functions on a case's inputs -> ([5] float32, {tensor: its term's gradient})"""
    B, P = x["B"], x["patch"]
    opts = edict(start_iter=edict(photometric=0), huber_loss_for_photometric=x["kind"] == "huber", depth_regu_patch_size=P or 2,
                 loss_weight=edict(fg_mask=-1 if x["fg_mask"] is not None else None, depth_patch=-3 if P else None, distortion=None),
                 nerf=edict(rand_rays=x["N"] if x["ray_idx"] is not None else None))
    obj = object.__new__(BasePhotoandReguLoss)
    obj.opt, obj.device = opts, torch.device("cpu")
    data = edict(idx=torch.arange(B), image=T(x["image"]), fg_mask=T(x["fg_mask"]))
    leaves = {k: T(x[k], True) for k in R.TENSORS if x[k] is not None}
    output = edict(idx_img_rendered=torch.arange(B), **leaves)
    if x["ray_idx"] is not None:
        output.ray_idx = T(x["ray_idx"])
    loss, _, _ = obj.compute_loss(opts, data, output, iteration=5, mode="train")
    mse, mse_fine = compute_mse_on_rays(data, output)
    out = np.zeros(5, dtype=np.float32)
    for i, key in enumerate(R.OUT_KEYS[:3]):
        if key in loss:
            out[i] = loss[key].item()
    out[3], out[4] = mse.item(), mse_fine.item() if mse_fine is not None else 0.0
    assert set(loss.keys()) == {"render"} | ({"fg_mask"} if x["fg_mask"] is not None else set()) | ({"depth_patch"} if P else set())
    grads = {k: torch.autograd.grad(loss[R.TERM_OF[k]], t, retain_graph=True)[0].numpy() for k, t in leaves.items()}
    return out, grads


def main():
    rs = np.random.RandomState(R.SEED + 1)
    image, mask = R.make_images(rs)
    fx = dict(image=image, fg_mask=mask, pool_check=R.pool_check())
    print("foreground share", mask.mean())
    assert 0.3 < mask.mean() < 0.5
    redrawn = R.pools()["redrawn"]
    worst = 0.0
    for name, c in R.CASES.items():
        x = R.inputs(fx, name)
        rows = c["B"] * c["N"]
        heads = 2 if c["fine"] else 1
        assert redrawn[:heads, :rows].sum() <= 0.01 * heads * rows * 3, (name, int(redrawn[:heads, :rows].sum()))
        s32, s64, ab = R.kink_sides(x)
        assert np.array_equal(s32, s64), name
        assert (np.abs(ab - R.DELTA) >= R.KINK_MARGIN).all(), name
        assert rows < 63 or (s64.any() and (~s64).any())
        out, grads = reference_run(x)
        fx[f"ref_{name}"] = out
        for key in c["seeds"]:
            if key in grads:
                fx[f"seed_{name}_{key}"] = grads[key]
        w = R.want(x)
        worst = max(worst, R.fwd_excess(out, w["out"]))
        if c["patch"]:
            const = R.constant_rows(x)
            assert const.any() and (grads["depth"].reshape(-1)[const] == 0).all(), name
    for key, v in fx.items():
        assert v.dtype in (np.float32, np.bool_) and np.isfinite(v).all(), key
    np.savez_compressed(R.FIXTURE, **fx)
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes,", len(fx), "arrays,", len(R.CASES), "cases")
    print("redrawn", int(redrawn.sum()), "of", redrawn.size, "; the reference's worst distance from float64:", worst, "fp32 spacings")


if __name__ == "__main__":
    main()
