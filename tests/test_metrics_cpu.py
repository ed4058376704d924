"""The evaluation metrics without a GPU: the float64 referee (tests/metrics_referee.py, which states the kernel's
bound) against the fixture (tests/golden/metrics.npz: the reference's own fp32 values); the torch restatement of sparf_amd.metrics against
both; the window table of csrc/metrics.h against the reference's; what ops.image_metrics hands the library, over a stand-in that records
calls (tests/metrics_fake.py); the routes; the argument checks of the C-ABI entry point; install() / uninstall()."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from sparf_amd import lib as L, metrics, ops
from sparf_amd.edict import EasyDict as edict
from tests import metrics_fake, metrics_referee as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def wants(fx):
    cache = {}

    def get(name):
        if name not in cache:
            x = R.inputs(name)
            cache[name] = (x, R.want(x, fx["window"]))
        return cache[name]
    return get


def T(a):
    return torch.from_numpy(np.array(a)) if a is not None else None


def trainer_form(a):
    """[B,3,H,W] -> the trainer's prediction: a channel-last buffer under a permuted view (nerf_trainer.py:391)"""
    B, _, H, W = a.shape
    return T(a).permute(0, 2, 3, 1).contiguous().view(-1, H, W, 3).permute(0, 3, 1, 2)


def call(fn, x, **kw):
    B = x["B"]
    d3 = lambda a: T(a).reshape(B, -1, 1) if a is not None else None
    return fn(trainer_form(x["pred"]), T(x["gt"]), pred_fine=trainer_form(x["fine"]) if x["fine"] is not None else None,
              fg_mask=T(x["mask"]).reshape(B, 1, x["H"], x["W"]) if x["mask"] is not None else None, depth=d3(x["depth"]), depth_fine=d3(x["depth_fine"]),
              depth_gt=d3(x["depth_gt"]), valid_depth_gt=T(x["valid"]), depth_scale=x["scale"], **kw)


def test_the_pools_are_the_generators(fx):
    assert np.array_equal(R.pool_check(), fx["pool_check"])
    assert set(fx) == {"window", "window_1d", "pool_check"} | {f"{k}_{c}" for c in R.CASES for k in ("ref", "dict", "refdist")}
    assert {c["content"] for c in R.CASES.values()} == set(R.CONTENTS) and {c["mask"] for c in R.CASES.values()} == set(R.MASKS)
    assert {c["depth"] for c in R.CASES.values()} == set(R.DEPTHS) and {(c["H"], c["W"]) for c in R.CASES.values()} == set(R.SHAPES) | {(96, 128)}
    for name, c in R.CASES.items():
        x = R.inputs(name)
        if c["mask"] == "blob" and c["H"] * c["W"] >= 120:
            assert 0.3 <= x["mask"].mean() <= 0.5
        if c["mask"] == "one":
            assert x["mask"].sum() == c["B"]


def test_window_table_is_the_references(fx):
    """the eleven weights of csrc/metrics.h, bit for bit, and the float products the residual is taken against"""
    src = open(os.path.join(ROOT, "sparf_amd", "csrc", "metrics.h")).read()
    body = re.search(r"const float window\[METRICS_K\] = \{([^}]*)\}", src).group(1)
    table = np.array([float.fromhex(t.strip().rstrip("f")) for t in body.split(",")], dtype=np.float64)
    assert table.shape == (R.K,) and np.array_equal(table.astype(np.float32).astype(np.float64), table)
    assert np.array_equal(table.astype(np.float32), fx["window_1d"])
    t32 = table.astype(np.float32)
    assert np.array_equal((t32[:, None] * t32[None, :]).astype(np.float32), fx["window"])
    assert np.array_equal(metrics.gaussian_window().numpy(), fx["window_1d"]) and np.array_equal(metrics.window_2d(11, 1)[0, 0].numpy(), fx["window"])


@pytest.mark.parametrize("name", R.CASES)
def test_referee_against_the_references_values(fx, wants, name):
    x, w = wants(name)
    ref = fx[f"ref_{name}"]
    assert R.same_pattern(ref, w["out"])
    dist = R.spacings(ref, w["out"])
    print(name, "reference to float64:", np.nanmax(dist, axis=1), "fp32 spacings")
    assert np.array_equal(np.nan_to_num(dist, nan=-1.0), np.nan_to_num(fx[f"refdist_{name}"], nan=-1.0))
    c = R.CASES[name]
    if c["content"] == "identical":
        assert (w["out"][:, 0] == 0).all() and np.isposinf(w["out"][:, 1]).all() and (w["out"][:, 2] == 1.0).all() and (ref[:, 2] == 1.0).all()
    if c["mask"] == "none":
        assert np.isnan(w["out"][:, 3:5]).all() and (w["out"][:, 5] == 1.0).all() and w["counts"][0] == 0
    if c["depth"] == "none":
        assert (w["out"][:, 6] == 0).all() and np.isnan(w["out"][:, 7]).all() and w["counts"][1] == 0
    if c["mask"] is None:
        assert np.isnan(w["out"][:, 3:6]).all()
    if c["depth"] is None:
        assert np.isnan(w["out"][:, 6:]).all()


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_within_the_references_distance(fx, wants, name):
    """image_metrics on CPU tensors (the restatement) within 4x the reference's own distance from the referee on the same case"""
    x, w = wants(name)
    res = call(metrics.image_metrics, x)
    heads = w["out"].shape[0]
    got = res.vector.numpy()[:heads]
    assert res.vector.dtype == torch.float32 and res.vector.shape == (2, 10) and res.counts.dtype == torch.int32
    assert R.same_pattern(got, w["out"]) and (heads == 2 or np.isnan(res.vector.numpy()[1]).all())
    d_got, d_ref = R.spacings(got, w["out"]), fx[f"refdist_{name}"]
    print(name, "reference", np.nanmax(d_ref), "restatement", np.nanmax(d_got))
    fin = np.isfinite(w["out"])
    assert (d_got[fin] <= 4 * d_ref[fin]).all(), (d_got, d_ref)
    assert np.array_equal(res.counts.numpy(), w["counts"])
    keys = {k + s for s in ("", "_fine")[:heads] for i, k in enumerate(R.OUTS)
            if i < 3 or (i < 6 and x["mask"] is not None) or (i >= 6 and x["depth" + s] is not None)}
    assert set(res) == keys | {"vector", "counts"} | ({"n_fg"} if x["mask"] is not None else set()) | ({"n_valid"} if x["depth"] is not None else set())
    assert all(res[k].dim() == 0 for k in keys) and float(res.ssim) == float(res.vector[0, 2])


# ---- the glue over the recording stand-in
def _data(x):
    B, H, W = x["B"], x["H"], x["W"]
    data = edict(idx=torch.arange(B))
    if x["mask"] is not None:
        data.fg_mask = T(x["mask"]).reshape(B, 1, H, W)
    if x["depth_gt"] is not None:
        data.depth_gt, data.valid_depth_gt = T(x["depth_gt"]).reshape(B, 1, H, W), T(x["valid"]).reshape(B, 1, H, W)
    return data, edict(idx_img_rendered=torch.arange(B))


@pytest.mark.parametrize("fine,mask,depth", [(f, m, d) for f in (False, True) for m in (False, True) for d in (False, True)])
def test_pointers_and_strides_of_every_combination(fine, mask, depth):
    x = R.inputs("s17x65")
    B, H, W = x["B"], x["H"], x["W"]
    pred, gt = trainer_form(x["pred"]), T(x["gt"])
    pf = trainer_form(x["fine"]) if fine else None
    m = T(x["mask"]).reshape(B, 1, H, W) if mask else None
    d, df, dg, v = (T(x[k]).reshape(B, -1, 1) if depth else None for k in ("depth", "depth_fine", "depth_gt", "valid"))
    if not fine:
        df = None
    with metrics_fake.installed() as lib:
        res = metrics.image_metrics(pred, gt, pred_fine=pf, fg_mask=m, depth=d, depth_fine=df, depth_gt=dg, valid_depth_gt=v, depth_scale=1.25)
    assert len(lib.calls) == 1
    c = lib.calls[0]
    assert (c["B"], c["H"], c["W"], c["depth_scale"]) == (B, H, W, 1.25)
    # the permuted view by its own address and its own strides: nothing was copied
    assert c["pred"] == pred.data_ptr() and c["pred_stride"] == (H * W * 3, 1, W * 3, 3) == tuple(pred.stride())
    assert c["gt"] == gt.data_ptr() and c["gt_stride"] == (3 * H * W, H * W, W, 1)
    assert c["pred_fine"] == (pf.data_ptr() if fine else None) and (not fine or c["pred_fine_stride"] == tuple(pf.stride()))
    assert c["fg_mask"] == (m.data_ptr() if mask else None) and (not mask or c["fg_mask_stride"] == (H * W, W, 1))
    for key, t in (("depth", d), ("depth_fine", df), ("depth_gt", dg), ("valid_depth_gt", v)):
        assert c[key] == (t.data_ptr() if t is not None else None)
        assert t is None or c[key + "_stride"] == (H * W, 1)
    assert c["out"] == res.vector.data_ptr() and c["counts"] == res.counts.data_ptr()
    assert res.vector.reshape(-1).tolist() == list(metrics_fake.OUT) and res.counts.tolist() == list(metrics_fake.COUNTS)
    assert ("ssim_fine" in res) == fine and ("psnr_masked" in res) == mask and ("rmse_scaled" in res) == depth and ("abs_e_fine" in res) == (fine and depth)


def test_strided_operands_are_read_in_place():
    x = R.inputs("s17x65")
    B, H, W = x["B"], x["H"], x["W"]
    buf = torch.zeros(B * 3 * H * W + 5)
    off = buf[5:].view(B, 3, H, W)                        # a storage offset
    wide = torch.zeros(B, 3, H, W + 4)[..., 2:W + 2]      # a row pitch
    with metrics_fake.installed() as lib:
        metrics.image_metrics(off, wide)
        metrics.image_metrics(T(x["pred"]).reshape(-1, 3, H, W), T(x["gt"]), fg_mask=T(x["mask"]))       # a [B,H,W] mask
    a, b = lib.calls
    assert a["pred"] == buf.data_ptr() + 20 and a["gt"] == wide.data_ptr() and a["gt_stride"] == (3 * H * (W + 4), H * (W + 4), W + 4, 1)
    assert b["fg_mask_stride"] == (H * W, W, 1)


def test_compute_metrics_makes_one_call_and_one_readback(monkeypatch):
    x = R.inputs("s17x65")
    data, output = _data(x)
    pred, gt = trainer_form(x["pred"]), T(x["gt"])
    reads = dict(tolist=0, item=0)
    real_tolist, real_item = torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.__setitem__("tolist", reads["tolist"] + 1), real_tolist(self))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (reads.__setitem__("item", reads["item"] + 1), real_item(self))[1])
    seen = []

    class Lpips:                                          # the caller's callable: its own readback is its own
        def item(self):
            return R.LPIPS

    def lpips(a, b):
        seen.append((a, b))
        return Lpips()

    with metrics_fake.installed() as lib:
        res = metrics.compute_metrics(data, output, pred, T(x["depth"]).reshape(1, -1, 1), gt, lpips, 1.37, suffix="_c")
        assert len(lib.calls) == 1 and reads == dict(tolist=1, item=0)
        masked = metrics.compute_metrics_masked(data, pred, gt, lpips, suffix="_m")
        assert len(lib.calls) == 2 and reads == dict(tolist=2, item=0)
    o = metrics_fake.OUT
    assert type(res) is edict and set(res) == {k + "_c" for k in R.DICT_KEYS} and all(type(v) is float for v in res.values())
    assert (res.psnr_c, res.ssim_c, res.lpips_c, res.psnr_masked_c, res.ssim_masked_c) == (o[1], o[2], R.LPIPS, o[4], o[5])
    assert (res.abse_depth_c, res.rmse_depth_c) == (min(o[6], o[8]), min(o[7], o[9]))
    assert type(masked) is dict and masked == {"psnr_masked_m": o[4], "ssim_masked_m": o[5], "lpips_masked_m": R.LPIPS}
    assert lib.calls[0]["pred"] == pred.data_ptr() and lib.calls[0]["depth_scale"] == np.float32(1.37) and lib.calls[1]["depth"] is None
    # LPIPS as the reference calls it: on x 2 - 1, and on the composites for the masked one
    assert len(seen) == 3 and torch.equal(seen[0][0], pred * 2 - 1) and torch.equal(seen[0][1], gt * 2 - 1)
    mf = data.fg_mask.float()
    assert torch.equal(seen[1][0], (pred * mf + (1. - mf)) * 2 - 1) and torch.equal(seen[2][1], (gt * mf + (1. - mf)) * 2 - 1)


def test_nan_ordering_of_the_two_scales():
    """Python's min in the reference's argument order: with no valid pixel rmse is NaN at both scales and stays NaN; abs_e is 0"""
    x = R.inputs("none17x65")
    data, output = _data(x)
    res = metrics.compute_metrics(data, output, trainer_form(x["pred"]), T(x["depth"]).reshape(1, -1, 1), T(x["gt"]), lambda a, b: torch.tensor(R.LPIPS), 1.37)
    assert res.abse_depth == 0.0 and math.isnan(res.rmse_depth) and math.isnan(res.psnr_masked) and res.ssim_masked == 1.0


def test_routes_to_the_restatement():
    x = R.inputs("s5x7")
    pred, gt, mask = T(x["pred"]), T(x["gt"]), T(x["mask"])
    with metrics_fake.installed() as lib:
        assert "ssim" in metrics.image_metrics(pred.double(), gt.double())                   # not float32
        assert "ssim" in metrics.image_metrics(pred[:, :1], gt[:, :1])                       # one channel
        assert "ssim_masked" in metrics.image_metrics(pred, gt, fg_mask=mask.float())        # a float mask
        assert metrics.ssim(pred, gt, window_size=7).dim() == 0 and metrics.ssim(pred, gt, size_average=False).shape == pred.shape
        with metrics.unfused():
            assert "ssim" in metrics.image_metrics(pred, gt)
        assert lib.calls == []
        metrics.image_metrics(pred, gt, fg_mask=mask)
        assert float(metrics.ssim(pred, gt)) == metrics_fake.OUT[2]
        assert len(lib.calls) == 2
    assert "ssim" in metrics.image_metrics(pred, gt)                                         # CPU tensors
    one = metrics.image_metrics(pred[:, :1], gt[:, :1])
    assert float(one.ssim) == pytest.approx(float(metrics.ssim_torch(pred[:, :1], gt[:, :1])))


# ---- the C ABI without a device
def _struct(B=1, H=4, W=5, **kw):
    keep = dict(buf=(ctypes.c_float * 4096)(), out=(ctypes.c_float * 20)(), counts=(ctypes.c_int32 * 2)(), ws=(ctypes.c_double * 4096)())
    addr = ctypes.addressof
    a = L.ImageMetrics(B=B, H=H, W=W, pred=addr(keep["buf"]), gt=addr(keep["buf"]), out=addr(keep["out"]), counts=addr(keep["counts"]),
                       workspace=addr(keep["ws"]), workspace_bytes=4096 * 8, depth_scale=1.0)
    for name in ("pred_stride", "gt_stride"):
        getattr(a, name)[:] = (3 * H * W, H * W, W, 1)
    for k, v in kw.items():
        if k.endswith("_stride"):
            getattr(a, k)[:] = v
        else:
            setattr(a, k, addr(keep["buf"]) if v is True else v)
    return a, keep


MALFORMED = dict(
    null_pred=dict(pred=None), null_gt=dict(gt=None), null_out=dict(out=None), null_counts=dict(counts=None), null_workspace=dict(workspace=None),
    zero_B=dict(B=0), zero_H=dict(H=0), zero_W=dict(W=0), negative_W=dict(W=-3), too_many_pixels=dict(B=4, H=1 << 14, W=1 << 15),
    depth_without_depth_gt=dict(depth=True), depth_fine_without_depth_gt=dict(pred_fine=True, depth_fine=True),
    depth_fine_without_pred_fine=dict(depth_fine=True, depth_gt=True), workspace_too_small=dict(workspace_bytes=18 * 8 - 1),
    negative_stride=dict(pred_stride=(60, 20, -5, 1)), negative_mask_stride=dict(fg_mask=True, fg_mask_stride=(20, 5, -1)),
    negative_depth_stride=dict(depth=True, depth_gt=True, depth_stride=(-20, 1)),
)


@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_calls_return_1_without_a_device(name):
    lib = L.load()
    a, keep = _struct(**MALFORMED[name])
    assert lib.sparf_image_metrics(ctypes.byref(a), None) == 1
    assert lib.sparf_image_metrics(None, None) == 1


def test_workspace_bytes():
    lib = L.load()
    for B, H, W in ((1, 1, 1), (1, 16, 32), (1, 17, 33), (2, 96, 128), (1, 300, 400), (3, 37, 38)):
        assert lib.sparf_image_metrics_workspace_bytes(B, H, W) == metrics_fake.workspace_bytes(B, H, W) > 0
    for B, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (4, 1 << 14, 1 << 15)):
        assert lib.sparf_image_metrics_workspace_bytes(B, H, W) == 0
    assert ops.METRICS_OUTS == R.OUTS == metrics.OUTS


# ---- install / uninstall
def _modules():
    theirs = dict(compute_metrics=lambda *a, **k: "their compute_metrics", compute_metrics_masked=lambda *a, **k: "their masked", ssim_loss=lambda a, b: "their ssim")
    core = types.SimpleNamespace(**theirs, MSE_loss=1)
    base = types.SimpleNamespace(ssim_loss=theirs["ssim_loss"], compute_metrics_masked=theirs["compute_metrics_masked"], other=2)
    trainer = types.SimpleNamespace(compute_metrics=theirs["compute_metrics"], other=3)
    return theirs, core, base, trainer


def test_install_and_uninstall_restore_exactly():
    theirs, core, base, trainer = _modules()
    before = [dict(vars(m)) for m in (core, base, trainer)]
    metrics.install(core, base, trainer)
    try:
        assert core.compute_metrics is metrics.compute_metrics and core.compute_metrics_masked is metrics.compute_metrics_masked and core.ssim_loss is metrics.ssim
        assert base.ssim_loss is metrics.ssim and base.compute_metrics_masked is metrics.compute_metrics_masked and trainer.compute_metrics is metrics.compute_metrics
        assert not hasattr(base, "compute_metrics") and not hasattr(trainer, "ssim_loss") and core.MSE_loss == 1
        with pytest.raises(RuntimeError):
            metrics.install(core)
        # a three-channel mask goes to the reference's own functions, untouched
        x = R.inputs("s5x7")
        data, output = _data(x)
        data.fg_mask = data.fg_mask.repeat(1, 3, 1, 1)
        assert core.compute_metrics(data, output, T(x["pred"]), None, T(x["gt"]), None) == "their compute_metrics"
        assert base.compute_metrics_masked(data, T(x["pred"]), T(x["gt"]), None) == "their masked"
    finally:
        metrics.uninstall()
    assert [dict(vars(m)) for m in (core, base, trainer)] == before
    metrics.uninstall()                                   # a second one is a no-op
    with pytest.raises(RuntimeError):                     # no original to hand a three-channel mask to
        metrics.compute_metrics(data, output, T(x["pred"]), None, T(x["gt"]), None)


@pytest.mark.parametrize("name", ["s5x7", "s17x65", "const37x38", "none17x65", "identical5x7", "plain37x38", "depth_only17x65", "mask_only5x7", "big"])
def test_installed_functions_give_the_references_keys_types_and_values(fx, wants, name):
    """compute_metrics / compute_metrics_masked / ssim_loss under the trainer's names, on CPU tensors (the restatement): the reference's
    keys and types, and its values to 4x its own distance from float64"""
    x, w = wants(name)
    theirs, core, base, trainer = _modules()
    data, output = _data(x)
    lpips = lambda a, b: torch.tensor(R.LPIPS)
    metrics.install(core, base, trainer)
    try:
        for h, (pk, dk) in enumerate((("pred", "depth"), ("fine", "depth_fine"))):
            if x[pk] is None:
                continue
            p = trainer_form(x[pk])
            d = T(x[dk]).reshape(x["B"], -1, 1) if x[dk] is not None else None
            res = trainer.compute_metrics(data, output, p, d, T(x["gt"]), lpips, x["scale"], suffix="_x")
            ref = fx[f"dict_{name}"][h]
            assert type(res) is edict and all(type(v) is float for v in res.values())
            assert list(res) == [k + "_x" for k in R.DICT_KEYS[:8 if x["mask"] is not None else 5]]
            got = np.array([res.get(k + "_x", np.nan) for k in R.DICT_KEYS])
            assert R.same_pattern(got, ref)
            # what each key is in the order of OUTS, for the referee's value and the reference's own distance
            src = dict(psnr=1, ssim=2, psnr_masked=4, ssim_masked=5)
            for i, k in enumerate(R.DICT_KEYS):
                if k in src and np.isfinite(ref[i]):
                    j = src[k]
                    assert R.spacings(got[i], w["out"][h, j]) <= 4 * fx[f"refdist_{name}"][h, j], k
                elif k.startswith("lpips") and not np.isnan(ref[i]):
                    assert got[i] == ref[i] == np.float32(R.LPIPS)
            if x[dk] is not None and np.isfinite(ref[3:5]).all():          # the min over the two scales picks the reference's side
                for i, (a, b) in ((3, (6, 8)), (4, (7, 9))):
                    side = int(np.argmin([fx[f"ref_{name}"][h, a], fx[f"ref_{name}"][h, b]]))
                    j = (a, b)[side]
                    assert R.spacings(got[i], w["out"][h, j]) <= 4 * fx[f"refdist_{name}"][h, j]
            if x["mask"] is not None:
                rm = base.compute_metrics_masked(data, p, T(x["gt"]), lpips)
                assert type(rm) is dict and list(rm) == ["psnr_masked", "ssim_masked", "lpips_masked"] and all(type(v) is float for v in rm.values())
                assert rm["ssim_masked"] == res.ssim_masked_x
            s = base.ssim_loss(p, T(x["gt"]))
            assert torch.is_tensor(s) and s.dim() == 0 and s.item() == res.ssim_x
    finally:
        metrics.uninstall()
