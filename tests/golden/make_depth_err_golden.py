"""Generate tests/golden/depth_err.npz: what the REFERENCE's own compute_depth_error_on_rays (source/training/core/metrics.py:81-134) did
(CPU) on the fixture cases of tests/depth_err_referee.py (tests/test_depth_err_cpu.py, tests/test_depth_err_gpu.py).

Runs only where the reference is importable (through tests/ref_harness.install_reference()): the committed file holds arrays only.
Every case calls the reference's unmodified function once per head with a data_dict of the three maps and an output_dict of
idx_img_rendered (a list) and ray_idx (where the case has one).  Nothing of the function is restated.  The file holds the inputs --
maps/depth_gt and maps/valid once, per case <name>/idx, ray_idx (absent for full images), depth, depth_fine -- and per case and
scale <name>/s<scale>/scale (float64) and ref [4] float32 = abs_e, rmse of the coarse head, then of the fine head."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat")]

from tests import ref_harness                                           # noqa: E402
from tests import depth_err_referee as R                                # noqa: E402

assert ref_harness.install_reference(), "the reference tree is not importable"
from easydict import EasyDict as edict                                  # noqa: E402
import source.training.core.metrics as ref_metrics                      # noqa: E402


def dicts_of(case):
    """the data_dict and output_dict of a case, as the trainer hands them over"""
    data = edict(depth_gt=torch.from_numpy(case["depth_gt"]), valid_depth_gt=torch.from_numpy(case["valid"]))
    out = edict(idx_img_rendered=[int(i) for i in case["idx"]], depth=torch.from_numpy(case["depth"]), depth_fine=torch.from_numpy(case["depth_fine"]))
    if case["ray_idx"] is not None:
        out.ray_idx = torch.from_numpy(case["ray_idx"])
    return data, out


def run_case(name, scale, fn=None):
    fn = fn or ref_metrics.compute_depth_error_on_rays
    case = R.build(name)
    data, out = dicts_of(case)
    with torch.no_grad():
        values = [v for head in (out.depth, out.depth_fine) for v in fn(data, out, head, scale)]
    assert all(v.dtype == torch.float32 and v.dim() == 0 for v in values)
    return case, np.array([v.item() for v in values], dtype=np.float32)


def main():
    depth_gt, valid = R.maps_of()
    arrays = {"maps/depth_gt": depth_gt, "maps/valid": valid}
    for name in R.FIXTURE_CASES:
        for scale in R.SCALES:
            case, ref = run_case(name, scale)
            assert case["depth_gt"].tobytes() == depth_gt.tobytes() and case["valid"].tobytes() == valid.tobytes()
            arrays.update({f"{name}/{k}": v for k, v in case.items() if v is not None and k not in ("depth_gt", "valid")})
            key = f"{name}/s{scale}/"
            arrays[key + "scale"], arrays[key + "ref"] = np.float64(scale), ref
            print(key, ref.tolist(), "referee", R.referee(case, scale)[0].tolist(), "K", R.referee(case, scale)[1])
    np.savez_compressed(R.FIXTURE, **arrays)
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
