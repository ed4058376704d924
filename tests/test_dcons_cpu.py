"""The depth-consistency loss without a GPU: the torch restatements of sparf_amd.losses against the fixture
(tests/golden/dcons.npz: the reference's own fp32 values) and the float64 referee (tests/dcons_referee.py, which states the bounds); the
argument checks of the C-ABI entry points; what the autograd Functions hand the library, over a stand-in that records calls
(tests/dcons_fake.py); unfused() routing; install_depth_consistency() / uninstall_depth_consistency(); and, where the reference tree is
present, its unmodified compute_loss_at_sampled_pose before and after the installation."""
import contextlib
import ctypes
import json
import os
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest
import torch

from sparf_amd import lib as L, losses, ops
from tests import dcons_fake, dcons_referee as R, ref_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def T(a, grad=False):
    return torch.from_numpy(np.array(a)).requires_grad_(grad) if a is not None else None


def held(got, ref32, want64, measure, what):
    """the restatement within 4x the reference's own distance from the referee"""
    d_ref, d_got = measure(ref32, want64), measure(got, want64)
    print(f"{what}: reference {d_ref:.3e}  restatement {d_got:.3e}")
    assert d_got <= 4 * d_ref, (what, d_got, d_ref)


def fwd_l2(got, want64):
    return R.l2(R.to_np(got).astype(np.float64) - np.asarray(want64, dtype=np.float64))


def scene(fx):
    H, W = (int(v) for v in fx["HW"])
    return dict(H=H, W=W, depth_min=T(fx["depth_min"]))


@pytest.mark.parametrize("n", R.NS)
def test_project_restatement_within_the_references_distance(fx, n):
    """the back-projecting form at every size; the points form up to the size the fixture holds reference values for"""
    src = R.project_want(fx, n)["src"]
    want = R.project_want(fx, n, guv=R.g_uv(n)[src], gz=R.g_z(n)[src])
    mask = want["mask"]
    assert np.array_equal(mask, fx["valid"][:n])
    d = T(fx["d"][:n], True)
    uv, z, index = losses.depth_consistency_project(None, T(fx["P_unseen"]), T(fx["K"]), **scene(fx), pixels_ref=T(fx["px"][:n]).long(), depth_ref=d,
                                                    intr_ref=T(fx["K"]), pose_c2w_ref=T(fx["T_c2w"]))
    assert index.dtype == torch.int32 and np.array_equal(index.numpy(), want["src"]) and uv.shape == (want["count"], 2)
    if want["count"]:
        held(uv, R.ref_of(fx, "uv", n)[mask], want["uv"], fwd_l2, "uv")
        held(z, R.ref_of(fx, "z", n)[mask], want["z"], fwd_l2, "z")
        g, = torch.autograd.grad((uv * T(R.g_uv(n)[src])).sum() + (z * T(R.g_z(n)[src])).sum(), d)
        held(g, R.ref_of(fx, "d_d", n), want["d_in"], R.rel_l2, "d_depth_ref")
    if n not in R.POINTS_NS:
        return
    Xw = T(fx["Xw"][:n], True)
    wantp = R.project_want(fx, n, Xw=fx["Xw"][:n], guv=R.g_uv(n)[src], gz=R.g_z(n)[src])
    assert np.array_equal(wantp["mask"], mask)
    uv, z, index = losses.depth_consistency_project(Xw, T(fx["P_unseen"][:3]), T(fx["K"]), fx["HW"][0], fx["HW"][1], float(fx["depth_min"]))
    assert np.array_equal(index.numpy(), want["src"])
    if want["count"]:
        held(uv, fx[f"uv_p_{n}"][mask], wantp["uv"], fwd_l2, "uv (points)")
        held(z, fx[f"z_p_{n}"][mask], wantp["z"], fwd_l2, "z (points)")
        g, = torch.autograd.grad((uv * T(R.g_uv(n)[src])).sum() + (z * T(R.g_z(n)[src])).sum(), Xw)
        held(g, fx[f"d_Xw_{n}"], wantp["d_in"], R.rel_l2, "d_points_w")


@pytest.mark.parametrize("base", R.PATTERN_BASES)
@pytest.mark.parametrize("pattern", R.PATTERNS[1:])
def test_project_restatement_mask_patterns(fx, pattern, base):
    """the rows of the first `base` points rearranged into each mask pattern, against the reference's own run on those rows"""
    rows = R.pattern_rows(fx["valid"][:base], pattern)
    n = len(rows)
    src = R.project_want(fx, n, px=fx["px"][rows], d=fx["d"][rows])["src"]
    want = R.project_want(fx, n, px=fx["px"][rows], d=fx["d"][rows], guv=R.g_uv(n)[src], gz=R.g_z(n)[src])
    mask = want["mask"]
    assert np.array_equal(mask, fx["valid"][rows]) and want["count"] == dict(all=n, none=0, first=1, last=1, alternating=n // 2)[pattern]
    d = T(fx["d"][rows], True)
    uv, z, index = losses.depth_consistency_project(None, T(fx["P_unseen"]), T(fx["K"]), **scene(fx), pixels_ref=T(fx["px"][rows]),
                                                    depth_ref=d, intr_ref=T(fx["K"]), pose_c2w_ref=T(fx["T_c2w"][:3]))
    assert np.array_equal(index.numpy(), want["src"]) and uv.shape == (want["count"], 2) and z.shape == (want["count"],)
    if want["count"]:
        held(uv, R.ref_of(fx, "uv", base, pattern)[mask], want["uv"], fwd_l2, "uv")
        held(z, R.ref_of(fx, "z", base, pattern)[mask], want["z"], fwd_l2, "z")
        g, = torch.autograd.grad((uv * T(R.g_uv(n)[src])).sum() + (z * T(R.g_z(n)[src])).sum(), d)
        held(g, R.ref_of(fx, "d_d", base, pattern), want["d_in"], R.rel_l2, "d_depth_ref")


@pytest.mark.parametrize("n", R.NS)
def test_select_restatement(fx, n):
    vis, uv, z = R.vis(n), fx["uv"][:n], fx["z"][:n]
    dst, src, count = R.compaction(vis >= np.float32(R.VIS_THRESH))
    for v in (T(vis), T(vis)[:, None]):
        uv_o, z_o, vis_o, index = losses.visibility_select(v, T(uv), T(z))
        assert np.array_equal(index.numpy(), src) and index.dtype == torch.int32
        assert np.array_equal(uv_o.numpy(), uv[src]) and np.array_equal(z_o.numpy(), z[src]) and np.array_equal(vis_o.numpy(), vis[src])


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("case", R.LOSS_CASES)
def test_loss_restatement_within_the_references_distance(fx, case, n):
    loss_type, fine = R.LOSS_CASES[case]
    inp = R.loss_inputs(fx, n, fine)
    want = R.loss_want(*inp, loss_type)
    t = [T(a, i in (0, 2, 4)) for i, a in enumerate(inp)]
    loss, avg = losses.depth_consistency_loss(t[0], t[1][:, None], t[2][None, :, None], t[3][None, :, None], t[4], t[5], loss_type=loss_type)
    ref = fx[f"loss_{case}_{n}"]
    held(loss, ref[0], want["loss"], fwd_l2, "loss")
    held(avg, ref[1], want["avg"], fwd_l2, "avg_vis_weight")
    if n in R.SEED_NS:
        leaves = [x for i, x in enumerate(t) if i in (0, 2, 4) and x is not None]
        for key, g, r in zip(("d_zp", "d_depth", "d_depth_fine"), torch.autograd.grad(loss, leaves), fx[f"seeds_{case}_{n}"]):
            held(g, r, want[key], R.rel_l2, key)
    e = inp[0] - inp[2]
    assert n < 63 or ((np.abs(e) < 1).any() and (e > 1).any() and (e < -1).any())          # both sides of |e| = 1


def test_epe_keeps_the_references_whole_vector_norm(fx):
    zp, v, dr, op, _, _ = (T(a) for a in R.loss_inputs(fx, 65, 1))
    loss, _ = losses.depth_consistency_loss(zp, v, dr, op, loss_type="epe")
    w = v * op
    assert torch.allclose(loss, (torch.norm(zp - dr) * w).sum() / (65 + 1e-6))
    with pytest.raises(ValueError):
        losses.depth_consistency_loss(zp, v, dr, op, loss_type="l3")
    with pytest.raises(ValueError):
        losses.depth_consistency_loss(zp, v, dr, op, depth_fine=dr)


def test_entry_points_check_their_arguments_without_a_device():
    """every refusal is decided before any HIP call: negative n, an unknown loss type, neither or both input forms, fine depth without
    fine opacity, a missing required pointer"""
    lib = L.load()
    buf = np.zeros(64, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)         # host memory: never dereferenced, every call below returns before a launch

    def call(name, defaults, **kw):
        assert tuple(defaults) == dcons_fake.DCONS_CALLS[name] and set(kw) <= set(defaults), name
        return getattr(lib, name)(*dict(defaults, **kw).values(), None)

    back = dict(points_w=None, pixels_ref=p, depth_ref=p, K_ref=p, pose_c2w_ref=p, ref_rows=4, pose_w2c_unseen=p, unseen_rows=3, K_unseen=p, n=2)
    project = lambda **kw: call("sparf_dcons_project", dict(back, H=10, W=10, depth_min=1.0, depth_min_dev=None, uv=p, z=p, dst=p, src=p, count=p,
                                                           workspace=None), **kw)
    project_bwd = lambda **kw: call("sparf_dcons_project_backward", dict(back, dst=p, d_uv=p, d_z=p, d_points_w=None, d_depth_ref=p), **kw)
    select = lambda **kw: call("sparf_dcons_select", dict(vis=p, uv=p, z=p, m=2, thresh=0.2, uv_out=p, z_out=p, vis_out=p, dst=p, src=p, count=p,
                                                         workspace=None), **kw)
    select_bwd = lambda **kw: call("sparf_dcons_select_backward", dict(dst=p, d_uv=p, d_z=p, m=2, d_uv_in=p, d_z_in=p), **kw)
    loss = lambda **kw: call("sparf_dcons_loss", dict(z_pseudo=p, vis=p, depth=p, opacity=p, depth_fine=p, opacity_fine=p, m=2, loss_type=0, out=p,
                                                     d_z_pseudo=p, d_depth=p, d_depth_fine=p, workspace=None), **kw)
    assert project(n=-1) == 1 and project_bwd(n=-1) == 1 and select(m=-1) == 1 and select_bwd(m=-1) == 1 and loss(m=-1) == 1
    assert loss(loss_type=3) == 1 and loss(loss_type=-1) == 1                       # epe is not a kernel case
    assert project(points_w=p) == 1 and project_bwd(points_w=p) == 1                # both forms
    for name in ("pixels_ref", "depth_ref", "K_ref", "pose_c2w_ref"):               # neither form (half of one)
        assert project(**{name: None}) == 1 and project_bwd(**{name: None}) == 1, name
    assert project(ref_rows=5) == 1 and project(unseen_rows=2) == 1 and project_bwd(unseen_rows=0) == 1
    for name in ("pose_w2c_unseen", "K_unseen", "uv", "z", "dst", "src", "count"):
        assert project(**{name: None}) == 1, name
    assert project(n=0, count=None) == 1
    for name in ("pose_w2c_unseen", "K_unseen", "dst", "d_depth_ref"):
        assert project_bwd(**{name: None}) == 1, name
    assert project_bwd(d_points_w=p) == 1                                           # the gradient of the other form
    for name in ("vis", "uv", "z", "uv_out", "z_out", "vis_out", "dst", "src", "count"):
        assert select(**{name: None}) == 1, name
    assert select_bwd(dst=None) == 1
    assert loss(opacity_fine=None) == 1 and loss(depth_fine=None) == 1              # fine depth without fine opacity, and the reverse
    assert loss(depth_fine=None, opacity_fine=None) == 1                            # a seed of a fine depth that is not there
    for name in ("z_pseudo", "vis", "depth", "opacity", "out"):
        assert loss(**{name: None}) == 1, name
    assert project_bwd(n=0) == 0 and select_bwd(m=0) == 0                           # nothing to launch
    wb = lib.sparf_dcons_workspace_bytes
    assert wb(0) == 0 and wb(-3) == 0 and wb(4096) == 0 and wb(4097) == dcons_fake.workspace_bytes(4097) == 64 and wb(8200) == 96


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(losses, "_takes_kernel", lambda values, constants: not losses._unfused)     # CPU tensors down the fused route
    with dcons_fake.installed() as lib:
        yield lib


FORM = dict(points_w=False, pixels_ref=False, depth_ref=False, K_ref=False, pose_c2w_ref=False, ref_rows=0, pose_w2c_unseen=True, unseen_rows=4,
            K_unseen=True)


def test_project_hands_over_one_form_and_gathers_in_backward(fake):
    n = 7
    Xw = torch.ones(n, 3, requires_grad=True)
    fake.keep = 5
    uv, z, index = losses.depth_consistency_project(Xw, torch.eye(4), torch.eye(3), 30, 40, 1.25)
    given = dict(FORM, points_w=True, n=n, H=30, W=40, depth_min=1.25, depth_min_dev=False, uv=True, z=True, dst=True, src=True, count=True,
                 workspace=False)
    assert fake.calls == [("sparf_dcons_project", given)]
    assert uv.shape == (5, 2) and z.shape == (5,) and index.shape == (5,) and index.dtype == torch.int32 and not index.requires_grad
    (uv.sum() + z.sum()).backward()
    assert fake.calls[1:] == [("sparf_dcons_project_backward", dict(FORM, points_w=True, n=n, dst=True, d_uv=True, d_z=True, d_points_w=True,
                                                                    d_depth_ref=False))]
    assert Xw.grad.shape == (n, 3)
    # the back-projecting form, [3,4] poses, a depth_min in host memory (read there), above the one-workgroup limit; only z used downstream
    fake.calls.clear()
    fake.keep = None
    n = dcons_fake.CHUNK + 1
    d = torch.ones(n, 1, requires_grad=True)
    uv, z, index = losses.depth_consistency_project(None, torch.eye(4)[:3], torch.eye(3), 30, 40, torch.tensor(1.25), pixels_ref=torch.zeros(n, 2).long(),
                                                    depth_ref=d, intr_ref=torch.eye(3), pose_c2w_ref=torch.eye(4)[:3])
    back = dict(FORM, pixels_ref=True, depth_ref=True, K_ref=True, pose_c2w_ref=True, ref_rows=3, unseen_rows=3, n=n)
    assert fake.calls == [("sparf_dcons_project", dict(given, **back, workspace=True))]
    assert uv.shape == (n, 2)
    z.sum().backward()
    assert fake.calls[1] == ("sparf_dcons_project_backward", dict(back, dst=True, d_uv=False, d_z=True, d_points_w=False, d_depth_ref=True))
    assert d.grad.shape == (n, 1)
    # a depth_min that the Function is handed as a tensor (one on the device) travels as a pointer and is never read here
    fake.calls.clear()
    ops.DconsProject.apply(torch.ones(2, 3), None, None, None, None, torch.eye(4), torch.eye(3), 30, 40, torch.tensor(1.25))
    assert fake.calls == [("sparf_dcons_project", dict(given, n=2, depth_min=0.0, depth_min_dev=True))]
    # nothing differentiable: the backward is never entered; no points: no readback, one call that launches nothing
    fake.calls.clear()
    uv, z, index = losses.depth_consistency_project(torch.ones(0, 3), torch.eye(4), torch.eye(3), 30, 40, 1.0)
    assert fake.names() == ["sparf_dcons_project"] and fake.calls[0][1]["n"] == 0 and uv.shape == (0, 2) and not uv.requires_grad
    with pytest.raises(ValueError):
        losses.depth_consistency_project(Xw, torch.eye(4), torch.eye(3), 30, 40, 1.0, pixels_ref=torch.zeros(7, 2), depth_ref=torch.ones(7),
                                         intr_ref=torch.eye(3), pose_c2w_ref=torch.eye(4))
    with pytest.raises(ValueError):
        losses.depth_consistency_project(None, torch.eye(4), torch.eye(3), 30, 40, 1.0, pixels_ref=torch.zeros(7, 2))
    with pytest.raises(ValueError):
        losses.depth_consistency_project(Xw, torch.eye(3), torch.eye(3), 30, 40, 1.0)


def test_project_takes_one_whole_form_on_either_route(fake):
    """world points together with part of a back-projection, or part of one alone, are refused in the public function: the kernel
    route and the torch route alike; a wrong shape is reported under the op's own name"""
    Xw, part = torch.ones(3, 3), dict(depth_ref=torch.ones(3))
    for route in ("fused", "torch"):
        with losses.unfused() if route == "torch" else contextlib.nullcontext():
            for points, kw in ((Xw, part), (Xw, dict(pose_c2w_ref=torch.eye(4))), (None, part),
                               (None, dict(pixels_ref=torch.zeros(3, 2), depth_ref=torch.ones(3), intr_ref=torch.eye(3)))):
                with pytest.raises(ValueError, match="depth_consistency_project: either"):
                    losses.depth_consistency_project(points, torch.eye(4), torch.eye(3), 30, 40, 1.0, **kw)
    assert fake.calls == []
    with pytest.raises(ValueError, match=r"^depth-consistency project: pose_w2c_unseen must be \[3, 4\] or \[4, 4\]"):
        losses.depth_consistency_project(Xw, torch.eye(3), torch.eye(3), 30, 40, 1.0)
    with pytest.raises(ValueError, match=r"^depth-consistency project: depth_ref has 2 elements for 3 points"):
        losses.depth_consistency_project(None, torch.eye(4), torch.eye(3), 30, 40, 1.0, pixels_ref=torch.zeros(3, 2), depth_ref=torch.ones(2),
                                         intr_ref=torch.eye(3), pose_c2w_ref=torch.eye(4))
    with pytest.raises(ValueError, match=r"^visibility select: vis has 2 elements for 3 points"):
        losses.visibility_select(torch.ones(2), torch.zeros(3, 2), torch.ones(3))
    with pytest.raises(ValueError, match=r"^depth-consistency loss: opacity has 2 elements for 3 points"):
        losses.depth_consistency_loss(torch.ones(3), torch.ones(3), torch.ones(3), torch.ones(2))


def test_select_and_loss_calls(fake):
    m = 6
    uv, z = torch.zeros(m, 2, requires_grad=True), torch.ones(m, requires_grad=True)
    fake.keep = 4
    uv_o, z_o, vis_o, index = losses.visibility_select(torch.ones(1, m).squeeze(0), uv, z)
    assert fake.calls == [("sparf_dcons_select", dict(vis=True, uv=True, z=True, m=m, thresh=pytest.approx(0.2), uv_out=True, z_out=True,
                                                      vis_out=True, dst=True, src=True, count=True, workspace=False))]
    assert uv_o.shape == (4, 2) and z_o.shape == (4,) and vis_o.shape == (4,) and not vis_o.requires_grad and index.dtype == torch.int32
    z_o.sum().backward()
    assert fake.calls[1] == ("sparf_dcons_select_backward", dict(dst=True, d_uv=False, d_z=True, m=m, d_uv_in=False, d_z_in=True))
    assert z.grad.shape == (m,) and uv.grad is None
    fake.calls.clear()
    dep = [torch.ones(1, 4, 1, requires_grad=True) for _ in range(2)]            # as a render returns them
    opa = [torch.ones(1, 4, 1, requires_grad=True) for _ in range(2)]            # opacity is detached by the loss
    loss, avg = losses.depth_consistency_loss(z_o.detach().requires_grad_(), vis_o, dep[0], opa[0], dep[1], opa[1], loss_type="L1")
    given = dict(z_pseudo=True, vis=True, depth=True, opacity=True, depth_fine=True, opacity_fine=True, m=4, loss_type=1, out=True, d_z_pseudo=True,
                 d_depth=True, d_depth_fine=True, workspace=False)
    assert fake.calls == [("sparf_dcons_loss", given)] and loss.dim() == 0 and avg.dim() == 0 and not avg.requires_grad
    loss.backward()
    assert fake.names() == ["sparf_dcons_loss"] and dep[0].grad.shape == (1, 4, 1) and opa[0].grad is None
    fake.calls.clear()
    big = dcons_fake.CHUNK + 1
    losses.depth_consistency_loss(torch.ones(big), torch.ones(big), torch.ones(big, requires_grad=True), torch.ones(big), loss_type="mse")
    assert fake.calls == [("sparf_dcons_loss", dict(given, depth_fine=False, opacity_fine=False, m=big, loss_type=2, d_z_pseudo=False,
                                                    d_depth_fine=False, workspace=True))]
    fake.calls.clear()
    losses.depth_consistency_loss(torch.ones(3), torch.ones(3), torch.ones(3), torch.ones(3), loss_type="epe")          # torch's
    with losses.unfused():
        losses.depth_consistency_project(torch.ones(3, 3), torch.eye(4), torch.eye(3), 30, 40, 1.0)
        losses.visibility_select(torch.ones(3), torch.zeros(3, 2), torch.ones(3))
        losses.depth_consistency_loss(torch.ones(3), torch.ones(3), torch.ones(3), torch.ones(3))
    assert fake.calls == []


def test_constants_that_need_a_gradient_take_the_restatement(monkeypatch):
    seen = []
    monkeypatch.setattr(ops.DconsProject, "apply", lambda *a: seen.append(a))
    P = torch.eye(4).requires_grad_()
    uv, z, _ = losses.depth_consistency_project(torch.tensor([[0.1, 0.2, 2.0]]), P, torch.tensor([[20.0, 0, 15], [0, 20.0, 10], [0, 0, 1]]), 30, 40, 1.0)
    assert seen == [] and uv.requires_grad and uv.shape == (1, 2)


class _Net:
    """renders that are deterministic functions of their pixel list"""

    def __init__(self):
        self.calls = []

    def render_up_to_maxdepth_at_specific_pose_and_rays(self, opt, data_dict, pose, intr, H, W, depth_max, iter, pixels=None, mode=None):
        assert not torch.is_grad_enabled() and pose.shape == (3, 4)
        self.calls.append(("to_max", pixels.shape[0]))
        return {"all_cumulated": (0.5 + 0.5 * torch.sin(pixels[:, 0] * 0.37 + depth_max))[None].clamp(0, 1)}

    def render_image_at_specific_pose_and_rays(self, opt, data_dict, pose, intr, H, W, iter, pixels=None, mode=None):
        from sparf_amd.edict import EasyDict as edict
        self.calls.append(("render", pixels.shape[0]))
        d = 2.5 + torch.cos(pixels[:, 1] * 0.11)
        o = 0.6 + 0.4 * torch.sin(pixels[:, 0] * 0.05) ** 2
        return edict(depth=d[None, :, None], opacity=o[None, :, None], rgb_fine=None, depth_fine=(d * 1.1)[None, :, None], opacity_fine=(o * 0.9)[None, :, None])


def test_install_patches_and_uninstall_restores(fx):
    class Theirs:
        def compute_loss_at_sampled_pose(self, *a, **k):
            return "theirs"

    mod = types.SimpleNamespace(DepthConsistencyLoss=Theirs)
    n = 257
    obj = Theirs()
    obj.net, obj.device = _Net(), torch.device("cpu")
    obj.opt = types.SimpleNamespace(diff_loss_type="huber", gradually_decrease_depth_cons_loss=True, depth_cons_loss_reduct_at_x_iter=100)
    from sparf_amd.edict import EasyDict as edict
    data = edict(depth_range=torch.tensor([[float(fx["depth_min"]), 6.0]]), iter=250)
    Xw = T(fx["Xw"][:n], True)
    H, W = (int(v) for v in fx["HW"])
    losses.install_depth_consistency(mod)
    try:
        with pytest.raises(RuntimeError):
            losses.install_depth_consistency(mod)
        losses.install(types.SimpleNamespace(CorrespondencesPairRenderDepthAndGet3DPtsAndReproject=type("C", (), {})))     # independent of it
        losses.uninstall()
        loss, stats, plots = obj.compute_loss_at_sampled_pose(data, T(fx["P_unseen"]), T(fx["K"]), Xw, H, W, T(fx["px"][:n]))
        count = int(fx["valid"][:n].sum())
        assert obj.net.calls[0] == ("to_max", count) and obj.net.calls[1][0] == "render" and 0 < obj.net.calls[1][1] < count
        assert set(stats) == {"nbr_px_sampling", "avg_vis_weight"} and stats["nbr_px_sampling"] == n and plots == {}
        # the same through the three public functions, by hand
        uv, z, _ = losses.depth_consistency_project(Xw, T(fx["P_unseen"]), T(fx["K"]), H, W, data.depth_range[0][0])
        with torch.no_grad():
            vis = obj.net.render_up_to_maxdepth_at_specific_pose_and_rays(None, None, torch.eye(4)[:3], None, H, W, z, 0, pixels=uv)
        uv, z, v, _ = losses.visibility_select(vis["all_cumulated"][0], uv, z)
        ret = obj.net.render_image_at_specific_pose_and_rays(None, None, None, None, H, W, 0, pixels=uv)
        want, avg = losses.depth_consistency_loss(z, v, ret.depth, ret.opacity, ret.depth_fine, ret.opacity_fine)
        assert torch.equal(loss["depth_cons"], want / 4) and torch.equal(stats["avg_vis_weight"], avg)
        loss["depth_cons"].backward()
        assert Xw.grad is not None and float(Xw.grad.abs().max()) > 0
        # either empty case: the reference's constant
        data.depth_range = torch.tensor([[100.0, 200.0]])
        out = obj.compute_loss_at_sampled_pose(data, T(fx["P_unseen"]), T(fx["K"]), Xw, H, W, T(fx["px"][:n]))
        assert out[1:] == ({}, {}) and out[0]["depth_cons"].item() == 0.0 and out[0]["depth_cons"].requires_grad
    finally:
        losses.uninstall_depth_consistency()
    assert Theirs().compute_loss_at_sampled_pose() == "theirs"


@pytest.mark.skipif(ref_harness.reference_root() is None, reason="reference tree not present")
def test_reference_method_after_install(fx):
    """The reference's unmodified compute_loss_at_sampled_pose on CPU tensors, on an instance made without its constructor whose `net`
    renders deterministic functions of the pixel list: after install_depth_consistency() against before -- the same ray counts and
    stats keys, and the loss, avg_vis_weight and the gradient to the world points within 4x the unpatched one's distance from the
    same chain in float64.  In a process of its own: the reference's `source` package must not meet dropin/source here."""
    code = """
        import json, numpy as np, torch
        from easydict import EasyDict as edict
        from tests import ref_harness, dcons_referee as R
        from tests.test_dcons_cpu import _Net
        assert ref_harness.install_reference()
        import source.training.core.depth_cons_loss as dc
        import sparf_amd.losses as losses
        fx = R.fixture()
        n = 1025
        H, W = (int(v) for v in fx["HW"])
        obj = object.__new__(dc.DepthConsistencyLoss)
        obj.device = torch.device("cpu")
        obj.opt = edict(diff_loss_type="huber", gradually_decrease_depth_cons_loss=True, depth_cons_loss_reduct_at_x_iter=100)
        def run(dtype):
            t = lambda a: torch.from_numpy(np.array(a)).to(dtype)
            obj.net = _Net()
            data = edict(iter=250, depth_range=t([[float(fx["depth_min"]), 6.0]]))
            Xw = t(fx["Xw"][:n]).requires_grad_()
            loss, stats, _ = obj.compute_loss_at_sampled_pose(data, t(fx["P_unseen"]), t(fx["K"]), Xw, H, W, t(fx["px"][:n]))
            loss["depth_cons"].backward()
            return loss["depth_cons"].detach().double().item(), float(stats["avg_vis_weight"]), Xw.grad.double().numpy(), obj.net.calls, \\
                stats["nbr_px_sampling"], sorted(stats)
        before, want = run(torch.float32), run(torch.float64)
        losses.install_depth_consistency(dc)
        try:
            after = run(torch.float32)
        finally:
            losses.uninstall_depth_consistency()
        restored = run(torch.float32)
        res = dict(loss=[abs(x[0] - want[0]) for x in (after, before)], avg=[abs(x[1] - want[1]) for x in (after, before)],
                   d_Xw=[R.rel_l2(x[2], want[2]) for x in (after, before)], calls_equal=after[3] == before[3] == want[3], calls=after[3],
                   nbr=[after[4], before[4]], keys=[after[5], before[5]], restored=restored[0] == before[0])
        print(json.dumps(res))
    """
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "compat")])
    p = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(res)
    assert res["calls_equal"] and res["calls"][0][0] == "to_max" and res["calls"][1][0] == "render" and res["restored"]
    assert res["nbr"] == [1025, 1025] and res["keys"][0] == res["keys"][1] == ["avg_vis_weight", "nbr_px_sampling"]
    for k in ("loss", "avg", "d_Xw"):
        ours, theirs = res[k]
        assert ours <= 4 * theirs and theirs > 0, (k, ours, theirs)
