"""A plain `bench.py` run: it times exactly --steps steps, prints one result line without the --full extras, and --dump-outputs writes
what the last timed step computed.  Run with `pytest -m gpu`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert line["unit"] == "rays/s" and line["dtype"] == "bf16x3" and line["metric"].startswith("training rays/sec")
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - line["config"]["rays_per_gpu_per_step"]) < 1e-6 * line["value"]
    for key in ("roofline", "cpu_baseline", "psnr_vs_ref", "parity_live", "other_modes", "other_sizes", "telemetry", "replayed_from_profiles"):
        assert key not in line, key
    assert line["sustained"] is None
    got = {p.name[:-4]: np.load(p) for p in out.iterdir()}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert abs(float(got["loss"][0]) - line["final_loss"]) <= 1e-6 * abs(line["final_loss"])
    assert got["render.rgb"].size == got["render.rgb_fine"].size == 4096 * 3
    for net in ("nerf", "nerf_fine"):
        assert got[f"param.{net}.mlp_feat.0.weight"].size == got[f"grad.{net}.mlp_feat.0.weight"].size == 256 * 63
