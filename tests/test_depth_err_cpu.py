"""The depth errors on rendered rays without a GPU: the torch restatement of sparf_amd.metrics against the fixture
(tests/golden/depth_err.npz: what the reference's own compute_depth_error_on_rays did) and the fixture against the numpy referee
(tests/depth_err_referee.py); the argument checks of the C-ABI entry point; what the glue hands the library, over a stand-in that records
calls (tests/depth_err_fake.py); install_depth_error_on_rays() / uninstall_depth_error_on_rays(); where the reference tree is present, its
unmodified function before the installation and after the uninstall; and the loss-unit rule of tests/test_tools_cpu.py for the new unit."""
import ctypes
import json
import math
import os
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest
import torch

from sparf_amd import build as BUILD, lib as L, metrics, ops
from sparf_amd.edict import EasyDict as edict
from sparf_amd.patcher import Patcher
from tests import depth_err_fake, depth_err_referee as R, ref_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The distance of the reference's own float32 values (the fixture) to the float64 referee, in fp32 spacings at the referee's value, per
# case: abs_e, rmse, abs_e_fine, rmse_fine.  Measured on the committed fixture; the reference sums |e| and e^2 in float32 over up to
# 713 rows after rounding pred * s to float32.  This is the yardstick of tests/test_depth_err_gpu.py: the kernel may be no farther from
# the reference than the reference is from the referee, plus one spacing.
REF_DISTANCE = {
    "list/s1.0": (0.48, 0.26, 0.16, 0.07), "list/s1.7": (0.27, 0.04, 0.05, 0.08),
    "per_image/s1.0": (0.18, 0.05, 0.37, 0.22), "per_image/s1.7": (1.42, 0.37, 0.51, 0.87),
    "full/s1.0": (0.46, 0.02, 0.05, 0.48), "full/s1.7": (0.52, 0.62, 0.45, 0.6),
    "subset/s1.0": (0.09, 0.5, 0.46, 0.12), "subset/s1.7": (1.58, 0.2, 1.26, 1.17),
    "hole/s1.0": (0.2, 0.22, 0.3, 0.18), "hole/s1.7": (0.51, 0.65, 1.23, 0.46),
    "empty/s1.0": (0.0, 0.0, 0.0, 0.0), "empty/s1.7": (0.0, 0.0, 0.0, 0.0),          # (0, NaN) on both sides
}


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def T(a):
    return None if a is None else torch.from_numpy(np.array(a))


def case_of(fx, name):
    """the recorded inputs of a fixture case; they are the case builder's"""
    case = dict(depth_gt=fx["maps/depth_gt"], valid=fx["maps/valid"], idx=fx[f"{name}/idx"], depth=fx[f"{name}/depth"], depth_fine=fx[f"{name}/depth_fine"],
                ray_idx=fx[f"{name}/ray_idx"] if f"{name}/ray_idx" in fx.files else None)
    return case


def dicts_of(case, idx=None):
    data = edict(depth_gt=T(case["depth_gt"]), valid_depth_gt=T(case["valid"]))
    out = edict(idx_img_rendered=[int(i) for i in case["idx"]] if idx is None else idx, depth=T(case["depth"]), depth_fine=T(case["depth_fine"]))
    if case["ray_idx"] is not None:
        out.ray_idx = T(case["ray_idx"])
    return data, out


def same_value_bits(got, want):
    got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    return got.shape == want.shape and all((math.isnan(g) and math.isnan(w)) or g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_the_fixture_holds_the_case_builders_inputs(fx):
    assert sorted({k.split("/")[0] for k in fx.files} - {"maps"}) == sorted(R.FIXTURE_CASES)
    for name in R.FIXTURE_CASES:
        built, kept = R.build(name), case_of(fx, name)
        for k, v in built.items():
            assert (v is None and kept[k] is None) or (v.dtype == kept[k].dtype and v.tobytes() == kept[k].tobytes()), (name, k)
    # what the issue asks of the cases: repeats in the list, an index [2, 0], a map without a valid pixel among the selected rays
    assert fx["maps/depth_gt"].shape == (3, 1, 16, 20) and fx["list/ray_idx"].shape == (37,) and len(set(fx["list/ray_idx"].tolist())) < 37
    assert fx["per_image/ray_idx"].shape == (3, 37) and "full/ray_idx" not in fx.files and fx["subset/idx"].tolist() == [2, 0]
    hole = R.build("hole")
    assert not R.gathered(hole["depth_gt"], hole["valid"], hole["idx"], hole["ray_idx"], 3, 37)[1][1].any() and R.referee(hole, 1.0)[1] > 0
    assert R.referee(R.build("empty"), 1.0)[1] == 0


@pytest.mark.parametrize("key", R.case_names())
def test_restatement_reproduces_the_fixture(fx, key):
    """the reference's operations in the reference's order on the CPU: the same bits"""
    name, scale = key.split("/")[0], float(fx[key + "/scale"])
    case = case_of(fx, name)
    data, out = dicts_of(case)
    got = [v for head in (out.depth, out.depth_fine) for v in metrics.compute_depth_error_on_rays(data, out, head, scale)]
    assert all(v.dim() == 0 and v.dtype == torch.float32 for v in got)
    assert same_value_bits([v.item() for v in got], fx[key + "/ref"]), ([v.item() for v in got], fx[key + "/ref"].tolist())
    # the public function on CPU tensors is the restatement, both heads, and counts the kept rows
    res = metrics.depth_error_on_rays(data.depth_gt, data.valid_depth_gt, out.depth, out.depth_fine, ray_idx=out.get("ray_idx"), img_idx=T(case["idx"]),
                                      scale=scale)
    assert same_value_bits(res.vector.numpy(), fx[key + "/ref"]) and int(res.n_valid) == R.referee(case, scale)[1] and res.n_valid.dtype == torch.int32
    assert set(res) == {"vector", "count", "abs_e", "rmse", "abs_e_fine", "rmse_fine", "n_valid"} and res.abs_e_fine.dim() == 0
    one = metrics.depth_error_on_rays(data.depth_gt, data.valid_depth_gt, out.depth, ray_idx=out.get("ray_idx"), img_idx=T(case["idx"]), scale=scale)
    assert "abs_e_fine" not in one and same_value_bits(one.vector.numpy(), [*fx[key + "/ref"][:2], 0.0, 0.0])


@pytest.mark.parametrize("key", R.case_names())
def test_fixture_against_the_referee(fx, key):
    """REF_DISTANCE is what the committed fixture measures; the reference's float32 sums stay within a few spacings of float64"""
    name, scale = key.split("/")[0], float(fx[key + "/scale"])
    want, K = R.referee(case_of(fx, name), scale)
    dist = [R.distance(g, w) for g, w in zip(fx[key + "/ref"], want)]
    print(key, "K", K, "distance of the reference to the referee in fp32 spacings", [round(d, 2) for d in dist])
    assert [round(d, 2) for d in dist] == list(REF_DISTANCE[key]), (key, dist)
    assert max(dist) <= 8.0


# ---- the entry point's argument checks
ARGS = dict(depth_gt=1, valid=1, img_idx=1, ray_idx=1, per_image=0, B_maps=3, B=2, HW=16, N=5, depth=1, depth_fine=None, scale=1.0, scale_dev=None,
            out=1, count=1, workspace=None)
MALFORMED = {
    "negative B": dict(B=-1), "negative HW": dict(HW=-1), "negative N": dict(N=-1), "no map": dict(B_maps=0), "negative maps": dict(B_maps=-2),
    "B HW above 2^30": dict(B=1 << 15, HW=(1 << 15) + 1), "B N above 2^30": dict(B=1 << 15, N=(1 << 15) + 1),
    "full images of another size": dict(ray_idx=None), "per_image 2": dict(per_image=2), "per_image -1": dict(per_image=-1),
    "no depth_gt": dict(depth_gt=None), "no depth": dict(depth=None), "no out": dict(out=None), "no count": dict(count=None),
}


def entry(**kw):
    assert tuple(ARGS) == depth_err_fake.CALLS["sparf_ray_depth_err"] and set(kw) <= set(ARGS)
    buf = np.zeros(64, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)         # host memory: never dereferenced, every call below returns before a launch
    pointers = {k for k, t in zip(ARGS, L.EXPORTS["sparf_ray_depth_err"][1]) if t is ctypes.c_void_p}
    args = [(p if v is not None else None) if k in pointers else v for k, v in dict(ARGS, **kw).items()]
    return L.load().sparf_ray_depth_err(*args, None)


@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_calls_return_1_without_a_device(name):
    assert entry(**MALFORMED[name]) == 1


def test_no_rows_and_nothing_to_write_is_no_call_and_workspace_bytes():
    assert entry(B=0, out=None, count=None, depth_gt=None, depth=None) == 0 and entry(N=0, out=None, count=None) == 0
    assert entry(N=0, ray_idx=None, out=None, count=None) == 0          # the empty index list of a call without rows has no address
    wb = L.load().sparf_ray_depth_err_workspace_bytes
    for rows in (-1, 0, 1, 4096, 4097, 8710, 1 << 30, (1 << 30) + 1):
        assert wb(rows) == depth_err_fake.workspace_bytes(rows), rows
    assert wb(4096) == 0 and wb(4097) == 80 and wb(8710) == 120


# ---- the glue over the recording stand-in
class Watch:
    """counts every .item(), .tolist() and nonzero of a tensor, and every index that holds a boolean tensor, while it is open"""
    NAMES = ("item", "tolist", "nonzero", "__getitem__")

    def __enter__(self):
        self.seen, self.patches = [], Patcher("tests.test_depth_err_cpu.Watch", "__exit__")

        def wrap(n, real):
            def method(t, *a, **k):
                if n != "__getitem__":
                    self.seen.append(n)
                elif any(torch.is_tensor(i) and i.dtype in (torch.bool, torch.uint8) for i in (a[0] if isinstance(a[0], tuple) else (a[0],))):
                    self.seen.append("boolean index")
                return real(t, *a, **k)
            return method
        for n in self.NAMES:                             # (a name torch.Tensor only inherits goes back to being inherited)
            self.patches.put(torch.Tensor, n, wrap(n, getattr(torch.Tensor, n)))
        real_nonzero = torch.nonzero
        self.patches.put(torch, "nonzero", lambda *a, **k: (self.seen.append("nonzero"), real_nonzero(*a, **k))[1])
        return self.seen

    def __exit__(self, *exc):
        self.patches.restore()


@pytest.fixture
def fake():
    with depth_err_fake.installed() as lib:
        yield lib


def test_the_watch_sees_what_the_restatement_does():
    data, out = dicts_of(R.build("list"))
    with Watch() as seen:
        metrics.compute_depth_error_on_rays(data, out, out.depth)
    assert seen.count("boolean index") == 2


def test_one_call_for_both_heads_on_the_maps_own_storage(fake):
    case = R.build("per_image")
    data, out = dicts_of(case)
    img_idx = T(case["idx"])
    with Watch() as seen:
        res = metrics.depth_error_on_rays(data.depth_gt, data.valid_depth_gt, out.depth, out.depth_fine, ray_idx=out.ray_idx, img_idx=img_idx, scale=1.7)
    assert fake.names() == ["sparf_ray_depth_err"] and seen == []
    rec, raw = fake.calls[0][1], fake.raw[0][1]
    assert rec == dict(depth_gt=True, valid=True, img_idx=True, ray_idx=True, per_image=1, B_maps=3, B=3, HW=R.HW, N=R.N, depth=True, depth_fine=True,
                       scale=1.7, scale_dev=False, out=True, count=True, workspace=False)
    assert ctypes.c_float(rec["scale"]).value == float(np.float32(1.7))          # the C ABI takes a float: rounded to float32 on the way in
    # the maps, the index and the rendered depths by their own addresses: no indexed copy, no gather
    assert raw["depth_gt"] == data.depth_gt.data_ptr() and raw["valid"] == data.valid_depth_gt.data_ptr() and raw["img_idx"] == img_idx.data_ptr()
    assert raw["ray_idx"] == out.ray_idx.data_ptr() and raw["depth"] == out.depth.data_ptr() and raw["depth_fine"] == out.depth_fine.data_ptr()
    assert raw["out"] == res.vector.data_ptr() and raw["count"] == res.count.data_ptr()
    # 0-dim views of the vector
    assert [float(res[k]) for k in ops.DEPTH_ERR_OUTS] == list(depth_err_fake.OUT) and int(res.n_valid) == depth_err_fake.COUNT
    assert all(res[k].dim() == 0 and res[k].data_ptr() == res.vector.data_ptr() + 4 * i for i, k in enumerate(ops.DEPTH_ERR_OUTS))
    assert res.n_valid.dim() == 0 and res.n_valid.data_ptr() == res.count.data_ptr()


def test_shapes_lists_and_scales(fake):
    case = R.build("list")
    data, out = dicts_of(case)
    # [B_maps,H,W] maps, a [B,N] depth, one list for all images, no index, no mask, one head
    res = metrics.depth_error_on_rays(data.depth_gt[:, 0], None, out.depth[..., 0], ray_idx=out.ray_idx)
    rec = fake.calls[-1][1]
    assert (rec["per_image"], rec["img_idx"], rec["valid"], rec["depth_fine"], rec["scale"], rec["N"]) == (0, False, False, False, 1.0, R.N)
    assert fake.raw[-1][1]["depth_gt"] == data.depth_gt.data_ptr() and set(res) == {"vector", "count", "abs_e", "rmse", "n_valid"}
    # full images: no ray_idx; above 4096 rows a workspace
    full = R.build_edge(2, 65, 67)
    metrics.depth_error_on_rays(T(full["depth_gt"]), T(full["valid"]), T(full["depth"]), T(full["depth_fine"]))
    rec = fake.calls[-1][1]
    assert (rec["ray_idx"], rec["B_maps"], rec["B"], rec["HW"], rec["N"], rec["workspace"]) == (False, 3, 2, 65 * 67, 65 * 67, True)
    # the scale: a numpy number by value; a one-element tensor on the operands' device by pointer, converted there where it is not float32
    with Watch() as seen:
        metrics.depth_error_on_rays(data.depth_gt, data.valid_depth_gt, out.depth, ray_idx=out.ray_idx, scale=np.float64(1.7))
        s32 = torch.tensor(1.7)
        metrics.depth_error_on_rays(data.depth_gt, data.valid_depth_gt, out.depth, ray_idx=out.ray_idx, scale=s32)
        metrics.depth_error_on_rays(data.depth_gt, data.valid_depth_gt, out.depth, ray_idx=out.ray_idx, scale=torch.tensor([1.7], dtype=torch.float64))
    assert seen == []
    by_value, by_pointer, converted = fake.calls[-3:]
    assert by_value[1]["scale"] == 1.7 and by_value[1]["scale_dev"] is False
    assert by_pointer[1]["scale_dev"] is True and fake.raw[-2][1]["scale_dev"] == s32.data_ptr() and converted[1]["scale_dev"] is True
    # a call without rows: the empty tensors have no address, the fine head is still marked present
    metrics.depth_error_on_rays(data.depth_gt, data.valid_depth_gt, torch.zeros(1, 0, 1), torch.zeros(1, 0, 1), ray_idx=torch.zeros(0, dtype=torch.int64))
    rec = fake.calls[-1][1]
    assert (rec["B"], rec["N"], rec["depth"], rec["ray_idx"], rec["depth_fine"]) == (1, 0, False, False, True)
    with pytest.raises(ValueError, match="full images"):
        ops.ray_depth_err(data.depth_gt, data.valid_depth_gt, out.depth)
    with pytest.raises(ValueError, match="ray_idx"):
        ops.ray_depth_err(data.depth_gt, data.valid_depth_gt, out.depth, ray_idx=out.ray_idx[:5])


def test_the_reference_signature_makes_one_call_and_passes_a_device_index(fake):
    case = R.build("subset")
    device_idx = T(case["idx"])
    data, out = dicts_of(case, idx=device_idx)
    with Watch() as seen:
        abs_e, rmse = metrics.compute_depth_error_on_rays(data, out, out.depth, 1.7)
        metrics.compute_depth_error_on_rays(data, out, out.depth_fine)
    assert fake.names() == ["sparf_ray_depth_err"] * 2 and seen == []
    assert (float(abs_e), float(rmse)) == depth_err_fake.OUT[:2] and abs_e.dim() == rmse.dim() == 0
    for (_, raw), head in zip(fake.raw, (out.depth, out.depth_fine)):
        assert raw["img_idx"] == device_idx.data_ptr() and raw["depth_gt"] == data.depth_gt.data_ptr() and raw["valid"] == data.valid_depth_gt.data_ptr()
        assert raw["depth"] == head.data_ptr() and raw["depth_fine"] is None and raw["ray_idx"] == out.ray_idx.data_ptr()
    assert (fake.calls[0][1]["B"], fake.calls[0][1]["B_maps"], fake.calls[0][1]["scale"], fake.calls[1][1]["scale"]) == (2, 3, 1.7, 1.0)
    # a host list is uploaded, except when it names every rendered image in order
    out.idx_img_rendered = [2, 0]
    metrics.compute_depth_error_on_rays(data, out, out.depth)
    assert fake.calls[-1][1]["img_idx"] is True
    data3, out3 = dicts_of(R.build("full"))
    with Watch() as seen:
        metrics.compute_depth_error_on_rays(data3, out3, out3.depth)
    assert fake.calls[-1][1]["img_idx"] is False and fake.calls[-1][1]["ray_idx"] is False and fake.calls[-1][1]["N"] == R.HW and seen == []


def test_routes_to_the_restatement(fake):
    case = R.build("list")
    data, out = dicts_of(case)
    want = R.referee(case, 1.0)[0]
    args = (data.depth_gt, data.valid_depth_gt, out.depth, out.depth_fine)
    with metrics.unfused():
        a = metrics.depth_error_on_rays(*args, ray_idx=out.ray_idx)
        metrics.compute_depth_error_on_rays(data, out, out.depth)
    b = metrics.depth_error_on_rays(data.depth_gt.double(), data.valid_depth_gt, out.depth.double(), out.depth_fine.double(), ray_idx=out.ray_idx)
    c = metrics.depth_error_on_rays(data.depth_gt, data.valid_depth_gt, out.depth.clone().requires_grad_(), out.depth_fine, ray_idx=out.ray_idx)
    assert fake.calls == []
    for res in (a, b, c):
        assert max(R.distance(g, w) for g, w in zip(res.vector.tolist(), want)) <= 8
    with torch.no_grad():                                # no gradient is asked for: the kernel
        metrics.depth_error_on_rays(data.depth_gt, data.valid_depth_gt, out.depth.clone().requires_grad_(), ray_idx=out.ray_idx)
    assert len(fake.calls) == 1


# ---- install / uninstall
def _modules():
    theirs = lambda *a, **k: "their compute_depth_error_on_rays"
    core = types.SimpleNamespace(compute_depth_error_on_rays=theirs, compute_metrics=1)
    trainer = types.SimpleNamespace(compute_depth_error_on_rays=theirs, other=2)
    bystander = types.SimpleNamespace(other=3)
    return theirs, core, trainer, bystander


def test_install_and_uninstall_restore_exactly():
    theirs, core, trainer, bystander = _modules()
    before = [dict(vars(m)) for m in (core, trainer, bystander)]
    metrics.install_depth_error_on_rays(core, trainer, bystander)
    try:
        assert core.compute_depth_error_on_rays is trainer.compute_depth_error_on_rays is metrics.compute_depth_error_on_rays
        assert not hasattr(bystander, "compute_depth_error_on_rays") and core.compute_metrics == 1
        with pytest.raises(RuntimeError, match="uninstall_depth_error_on_rays"):
            metrics.install_depth_error_on_rays(core)
        metrics.install(core)                            # independent of the other installer
        metrics.uninstall()
        assert core.compute_depth_error_on_rays is metrics.compute_depth_error_on_rays
        data, out = dicts_of(R.build("list"))
        want = R.referee(R.build("list"), 1.0)[0]
        got = trainer.compute_depth_error_on_rays(data, out, out.depth)
        assert R.distance(got[0], want[0]) <= 8 and R.distance(got[1], want[1]) <= 8
    finally:
        metrics.uninstall_depth_error_on_rays()
    assert [dict(vars(m)) for m in (core, trainer, bystander)] == before and core.compute_depth_error_on_rays is theirs
    metrics.uninstall_depth_error_on_rays()              # a second one is a no-op
    metrics.install_depth_error_on_rays(core)            # and again after an uninstall
    metrics.uninstall_depth_error_on_rays()
    assert dict(vars(core)) == before[0]


@pytest.mark.skipif(ref_harness.reference_root() is None, reason="reference tree not present")
def test_reference_function_around_an_install(fx):
    """The reference's unmodified compute_depth_error_on_rays on the fixture cases (CPU tensors): before install_depth_error_on_rays() and
    after the uninstall it returns the fixture's values, the same bits; while installed, source.training.core.metrics holds ours, which
    on CPU tensors is the restatement and returns them too.  In a process of its own: the reference's `source` package must not meet
    dropin/source here."""
    code = """
        import json, numpy as np, torch
        from tests import depth_err_referee as R
        from tests.golden import make_depth_err_golden as M
        import source.training.core.metrics as rm
        import sparf_amd.metrics as metrics
        theirs = rm.compute_depth_error_on_rays
        bits = lambda a: np.asarray(a, dtype=np.float32).tobytes().hex()
        res = {}
        for name in R.FIXTURE_CASES:
            for scale in R.SCALES:
                before = M.run_case(name, scale, rm.compute_depth_error_on_rays)[1]
                metrics.install_depth_error_on_rays(rm)
                try:
                    assert rm.compute_depth_error_on_rays is metrics.compute_depth_error_on_rays
                    during = M.run_case(name, scale, rm.compute_depth_error_on_rays)[1]
                finally:
                    metrics.uninstall_depth_error_on_rays()
                after = M.run_case(name, scale, rm.compute_depth_error_on_rays)[1]
                res[f"{name}/s{scale}"] = dict(restored=rm.compute_depth_error_on_rays is theirs, before=bits(before), during=bits(during), after=bits(after))
        print(json.dumps(res))
    """
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "compat")])
    p = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(res) == set(R.case_names())
    for key, r in res.items():
        want = fx[key + "/ref"]
        assert r["restored"], key
        for when in ("before", "during", "after"):
            got = np.frombuffer(bytes.fromhex(r[when]), dtype=np.float32)
            assert same_value_bits(got, want), (key, when, got.tolist(), want.tolist())


def test_the_unit_takes_its_block_sums_from_ordered_h():
    """the rule tests/test_tools_cpu.py states for the loss units, for this one: it includes ordered.h and holds no ballot and no shuffle
    butterfly of its own, comments included; and source_hash() covers the unit and its header"""
    assert "depth_err.hip" in BUILD.SOURCES and "depth_err.h" in BUILD.HEADERS
    text = open(os.path.join(BUILD.CSRC, "depth_err.hip")).read()
    assert '#include "ordered.h"' in text and '#include "depth_err.h"' in text
    for word in ("__ballot", "__shfl_xor", "atomicAdd", "asm"):
        assert word not in text, f"depth_err.hip has a {word} of its own"
    # the sums are ordered.h's chunked sum over the unit's policy, which hands it DEPTH_ERR_NACC totals
    assert "launch_ordered_sum<DepthErrSum>" in text and "NACC = DEPTH_ERR_NACC" in text
    header = open(os.path.join(BUILD.CSRC, "ordered.h")).read()
    assert "block_totals<S::NACC" in header and "sum_parts<S::NACC>" in header
