"""Generate tests/golden/metrics.npz: the REFERENCE's own fp32 results (CPU) for the evaluation-metrics kernel (tests/test_metrics_cpu.py,
tests/test_metrics_gpu.py; names, shapes and cases: tests/metrics_referee.py).

Runs only where the reference is importable (through tests/ref_harness.install_reference()): the committed file holds arrays only.
The values come from the reference's UNMODIFIED MSE_loss, ssim, create_window, gaussian, compute_metrics and compute_metrics_masked, with a
stub lpips_loss that returns a fixed tensor.  compute_metrics gives the depth errors after its min over the two scales; the errors at
each scale on its own come from the same function at scale 1, on the depth as it is and on the depth times the scale (the product the
reference forms itself, metrics.py:178).

Asserted here for every case: the reference's NaN / inf pattern equals the referee's, and the blob mask covers 30-50 % of an image of
10 x 12 pixels or more.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat")]

from tests import ref_harness                                           # noqa: E402
from tests import metrics_referee as R                                  # noqa: E402

assert ref_harness.install_reference(), "the reference tree is not importable"
from easydict import EasyDict as edict                                  # noqa: E402
from source.training.core.metrics import MSE_loss, compute_metrics, compute_metrics_masked      # noqa: E402
from third_party.pytorch_ssim.ssim import create_window, gaussian, ssim                            # noqa: E402


def T(a):
    return torch.from_numpy(np.array(a)) if a is not None else None


def lpips_stub(a, b):
    return torch.tensor(R.LPIPS)


def reference_run(x):
    """-> (values [heads,10] float32 in the order of R.OUTS, what compute_metrics returns [heads,8] in the order of R.DICT_KEYS)"""
    B, H, W = x["B"], x["H"], x["W"]
    gt = T(x["gt"])
    data = edict(idx=torch.arange(B))
    if x["mask"] is not None:
        data.fg_mask = T(x["mask"]).reshape(B, 1, H, W)
    if x["depth_gt"] is not None:
        data.depth_gt, data.valid_depth_gt = T(x["depth_gt"]).reshape(B, 1, H, W), T(x["valid"]).reshape(B, 1, H, W)
    output = edict(idx_img_rendered=torch.arange(B))
    vals, dicts = [], []
    for pk, dk in (("pred", "depth"), ("fine", "depth_fine")):
        if x[pk] is None:
            continue
        # the trainer's form: a channel-last buffer under a permuted view (nerf_trainer.py:391)
        p = T(x[pk]).permute(0, 2, 3, 1).contiguous().view(-1, H, W, 3).permute(0, 3, 1, 2)
        d = T(x[dk]).reshape(B, -1, 1) if x[dk] is not None else None
        v = np.full(len(R.OUTS), np.nan, dtype=np.float32)
        v[0] = MSE_loss(p, gt).item()
        r1 = compute_metrics(data, output, p, d, gt, lpips_stub, 1.)
        assert type(r1) is edict and all(type(val) is float for val in r1.values())
        v[1], v[2] = r1.psnr, ssim(p, gt).item()
        assert r1.ssim == v[2].item() or (np.isnan(r1.ssim) and np.isnan(v[2]))
        if x["mask"] is not None:
            mf = data.fg_mask.float()
            v[3] = MSE_loss(p * mf + (1. - mf), gt * mf + (1. - mf), mf == 1.).item()
            rm = compute_metrics_masked(data, p, gt, lpips_stub)
            assert type(rm) is dict
            v[4], v[5] = rm["psnr_masked"], rm["ssim_masked"]
        if d is not None:
            v[6], v[7] = r1.abse_depth, r1.rmse_depth
            rs = compute_metrics(data, output, p, d.clone() * x["scale"], gt, lpips_stub, 1.)
            v[8], v[9] = rs.abse_depth, rs.rmse_depth
        rd = compute_metrics(data, output, p, d, gt, lpips_stub, x["scale"], suffix="_x")
        assert set(rd.keys()) == {k + "_x" for k in R.DICT_KEYS[:5 if x["mask"] is None else 8]}
        dicts.append(np.array([rd.get(k + "_x", np.nan) for k in R.DICT_KEYS], dtype=np.float32))
        vals.append(v)
    return np.stack(vals), np.stack(dicts)


def main():
    window = create_window(R.K, 1)[0, 0].numpy()
    fx = dict(window=window, window_1d=gaussian(R.K, 1.5).numpy(), pool_check=R.pool_check())
    assert window.dtype == np.float32 and window.shape == (R.K, R.K)
    worst = 0.0
    for name, c in R.CASES.items():
        x = R.inputs(name)
        if c["mask"] == "blob" and c["H"] * c["W"] >= 120:
            assert 0.3 <= x["mask"].mean() <= 0.5, (name, x["mask"].mean())
        if c["depth"] == "some" and c["H"] * c["W"] >= 120:
            assert 0.5 <= x["valid"].mean() <= 0.7, (name, x["valid"].mean())
        ref, dicts = reference_run(x)
        w = R.want(x, window)
        assert R.same_pattern(ref, w["out"]), (name, ref, w["out"])
        dist = R.spacings(ref, w["out"])
        fx[f"ref_{name}"], fx[f"dict_{name}"], fx[f"refdist_{name}"] = ref, dicts, dist
        worst = max(worst, np.nanmax(dist))
        print(f"{name:28s} reference to float64, worst of a head: {np.nanmax(dist, axis=1)} fp32 spacings")
    np.savez_compressed(R.FIXTURE, **fx)
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes,", len(fx), "arrays,", len(R.CASES), "cases; the reference's worst distance:", worst)


if __name__ == "__main__":
    main()
