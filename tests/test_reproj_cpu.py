"""The correspondence loss without a GPU: the torch restatement of sparf_amd.losses against the fixture
(tests/golden/reproj.npz: the reference's own fp32 values) and the float64 referee (tests/reproj_referee.py, which states the bounds);
the argument checks of the two C-ABI entry points; what the autograd Functions hand the library, over a stand-in that records calls
(tests/reproj_fake.py); install() / uninstall(); n = 0; and, where the reference tree is present, its compute_loss_on_image_pair after
install()."""
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
from tests import reproj_fake, reproj_referee as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


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


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("case", R.CASES)
def test_torch_term_restatement_within_the_references_distance(fx, case, n):
    inp, opts = R.term_case(fx, n, case)
    want = R.term_want(inp, opts)
    k = f"t{n}_{case}_"
    di, Tt = T(inp["di"], True), T(inp["T"], True)
    w = T(inp["w"])[:, None] if inp["w"] is not None else None
    loss, stats, valid = losses.reprojection_loss(T(inp["pi"]).long(), di, T(inp["Ki"]), T(inp["pj"]), T(inp["dj"]), T(inp["Kj"]), Tt, w,
                                                  return_valid_mask=True, **opts)
    assert valid.shape == (n, 1) and np.array_equal(valid.numpy()[:, 0], want["valid"]) and np.array_equal(want["valid"], fx[k + "valid"])
    held(loss, fx[k + "loss"], want["loss"], R.fwd_abs, "loss")
    d_di, d_T = torch.autograd.grad(loss, (di, Tt))
    held(d_di, fx[k + "d_di"], want["d_di"], R.rel_l2, "d_di")
    held(d_T, fx[k + "d_T"], want["d_T"], R.rel_l2, "d_T")
    assert set(stats) == ({"perc_val_pix_rep", "perc_val_depth_rep"} if opts["pixel_thresh"] is not None else set())
    for i, key in enumerate(("perc_val_pix_rep", "perc_val_depth_rep")):
        if key in stats:
            held(stats[key], fx[k + "stats"][i], want["stats"][i], R.fwd_abs, key)


@pytest.mark.parametrize("n", R.PAIR_NS)
@pytest.mark.parametrize("fine", [0, 1])
@pytest.mark.parametrize("case", R.PAIR_CASES)
def test_torch_pair_restatement_within_the_references_distance(fx, case, fine, n):
    inp, opts = R.pair_case(fx, n, fine, case)
    want = R.pair_want(inp, opts)
    k = f"p{n}_f{fine}_{case}_"
    leaves = {s: T(inp[s], True) for s in ("ds", "do", "fs", "fo", "Ps", "Po") if inp[s] is not None}
    loss, stats = losses.correspondence_pair_loss(T(inp["ps"]).long(), T(inp["po"]), leaves["ds"], leaves["do"], T(inp["Ks"]), T(inp["Ko"]),
                                                  leaves["Ps"], leaves["Po"], T(inp["w"])[:, None], leaves.get("fs"), leaves.get("fo"), **opts)
    held(loss, fx[k + "loss"], want["loss"], R.fwd_abs, "loss")
    for (s, leaf), g in zip(leaves.items(), torch.autograd.grad(loss, list(leaves.values()))):
        g = g[:3] if s in ("Ps", "Po") else g
        ref = fx[k + "d_" + s][:3] if s in ("Ps", "Po") else fx[k + "d_" + s]
        held(g, ref, want["d_" + s], R.rel_l2, "d_" + s)
    keys = (("perc_val_pix_rep", "perc_val_depth_rep") if opts["pixel_thresh"] is not None else ()) + ("depth_in_corr_loss",)
    assert set(stats) == set(keys)
    for key in keys:
        i = losses.STAT_KEYS.index(key)
        held(stats[key], fx[k + "stats"][i], want["stats"][i], R.fwd_abs, key)
    # [3,4] poses are the same function
    loss34, _ = losses.correspondence_pair_loss(T(inp["ps"]), T(inp["po"]), T(inp["ds"]), T(inp["do"]), T(inp["Ks"]), T(inp["Ko"]),
                                                T(inp["Ps"][:3]), T(inp["Po"][:3]), T(inp["w"]), T(inp["fs"]), T(inp["fo"]), **opts)
    assert torch.equal(loss34, loss.detach())


def test_restatement_takes_float64():
    fxd = R.fixture()
    inp, opts = R.term_case(fxd, 65, "huber_checks")
    want = R.term_want(inp, opts)
    a = {k: R.f64(v) for k, v in inp.items()}
    loss, stats = losses.reprojection_loss(a["pi"], a["di"], a["Ki"], a["pj"], a["dj"], a["Kj"], a["T"], a["w"][:, None], **opts)
    assert loss.dtype == torch.float64 and abs(loss.item() - want["loss"]) <= 1e-12 * abs(want["loss"])
    assert abs(stats["perc_val_depth_rep"].item() - want["stats"][1]) < 1e-14


def test_entry_points_check_their_arguments_without_a_device():
    """every refusal is decided before any HIP call: negative n, an unknown loss type, the depth check without depth_j, fine depths (or
    their seeds) for one view only, a missing required pointer"""
    lib = L.load()
    buf = np.zeros(64, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)         # host memory: never dereferenced, every call below returns before a launch

    def term(**kw):
        a = dict(pixels_i=p, depth_i=p, K_i=p, pixels_j=p, depth_j=p, K_j=p, T_itoj=p, weights=p, n=2, loss_type=0, pix_check=1, pix_thresh=10.0,
                 depth_check=1, depth_thresh=0.1, out=p, d_depth_i=p, d_T=p, valid=p, workspace=None)
        assert tuple(a) == reproj_fake.REPROJ_CALLS["sparf_reproj_loss"] and set(kw) <= set(a)
        a.update(kw)
        return lib.sparf_reproj_loss(*a.values(), None)

    def pair(**kw):
        a = dict(pixels_self=p, pixels_other=p, depth_self=p, depth_other=p, depth_fine_self=p, depth_fine_other=p, K_self=p, K_other=p,
                 pose_self=p, pose_other=p, weights=p, n=2, loss_type=0, pix_check=0, pix_thresh=0.0, depth_check=0, depth_thresh=0.0, out=p,
                 d_depth_self=p, d_depth_other=p, d_depth_fine_self=p, d_depth_fine_other=p, d_pose_self=p, d_pose_other=p, workspace=None)
        assert tuple(a) == reproj_fake.REPROJ_CALLS["sparf_reproj_pair_loss"] and set(kw) <= set(a)
        a.update(kw)
        return lib.sparf_reproj_pair_loss(*a.values(), None)

    assert term(n=-1) == 1 and pair(n=-1) == 1
    assert term(loss_type=4) == 1 and term(loss_type=-1) == 1 and pair(loss_type=4) == 1
    assert term(depth_j=None) == 1                                  # the depth check is on
    assert term(out=None) == 1 and pair(out=None) == 1
    for name in ("pixels_i", "depth_i", "K_i", "pixels_j", "K_j", "T_itoj"):
        assert term(**{name: None}) == 1, name
    assert pair(depth_fine_self=None) == 1 and pair(depth_fine_other=None) == 1
    assert pair(depth_fine_self=None, depth_fine_other=None) == 1   # seeds of fine depths that are not there
    assert pair(depth_fine_self=None, depth_fine_other=None, d_depth_fine_self=None) == 1
    for name in ("pixels_self", "pixels_other", "depth_self", "depth_other", "K_self", "K_other", "pose_self", "pose_other"):
        assert pair(**{name: None}) == 1, name
    assert lib.sparf_reproj_workspace_bytes(4096) == 0 and lib.sparf_reproj_workspace_bytes(0) == 0
    assert lib.sparf_reproj_workspace_bytes(4097) == reproj_fake.WORKSPACE_BYTES


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(losses, "_takes_kernel", lambda values, constants: not losses._unfused)     # CPU tensors down the fused route
    with reproj_fake.installed() as lib:
        yield lib


def _term_inputs(n, grad_T=True):
    return dict(pixels_i=torch.zeros(n, 2, dtype=torch.long), depth_i=torch.ones(n, requires_grad=True), intr_i=torch.eye(3),
                pixels_j=torch.zeros(n, 2), depth_j=torch.ones(n, 1), intr_j=torch.eye(3), T_itoj=torch.eye(4).requires_grad_(grad_T))


def test_term_enters_the_library_once_and_never_in_backward(fake):
    a = _term_inputs(5)
    loss, stats, valid = losses.reprojection_loss(**a, weights=torch.ones(5, 1), pixel_thresh=10.0, depth_thresh=0.1, return_valid_mask=True)
    given = dict(pixels_i=True, depth_i=True, K_i=True, pixels_j=True, depth_j=True, K_j=True, T_itoj=True, weights=True, n=5, loss_type=0,
                 pix_check=1, pix_thresh=10.0, depth_check=1, depth_thresh=pytest.approx(0.1), out=True, d_depth_i=True, d_T=True, valid=True,
                 workspace=False)
    assert fake.calls == [("sparf_reproj_loss", given)]
    assert loss.dim() == 0 and valid.shape == (5, 1) and valid.dtype == torch.bool
    assert set(stats) == {"perc_val_pix_rep", "perc_val_depth_rep"} and all(s.dim() == 0 and not s.requires_grad for s in stats.values())
    loss.backward()
    assert fake.names() == ["sparf_reproj_loss"]
    assert a["depth_i"].grad.shape == (5,) and a["T_itoj"].grad.shape == (4, 4)
    # no weights, no checks, no mask, T constant, mse: NULL for each; depth_j is not handed over without its check
    fake.calls.clear()
    a = _term_inputs(3, grad_T=False)
    loss, stats = losses.reprojection_loss(**a, loss_type="MSE")
    assert stats == {}
    assert fake.calls == [("sparf_reproj_loss", dict(given, depth_j=False, weights=False, n=3, loss_type=2, pix_check=0, pix_thresh=0.0, depth_check=0,
                                                     depth_thresh=0.0, d_T=False, valid=False))]
    # nothing differentiable: no seeds
    fake.calls.clear()
    losses.reprojection_loss(**{k: v.detach() for k, v in _term_inputs(3).items()}, loss_type="epe")
    assert fake.calls[0][1]["d_depth_i"] is False and fake.calls[0][1]["d_T"] is False and fake.calls[0][1]["loss_type"] == 3
    # above the one-workgroup limit the call carries a workspace
    fake.calls.clear()
    losses.reprojection_loss(**_term_inputs(reproj_fake.SINGLE_MAX + 1))
    assert fake.calls[0][1]["workspace"] is True and fake.calls[0][1]["n"] == reproj_fake.SINGLE_MAX + 1
    with pytest.raises(ValueError):
        losses.reprojection_loss(**_term_inputs(3), loss_type="l3")
    with pytest.raises(ValueError):                # the kernel reads 16 floats of T: a [3,4] is refused, not padded
        losses.reprojection_loss(**dict(_term_inputs(3), T_itoj=torch.eye(4)[:3]))
    with pytest.raises(ValueError):
        losses.reprojection_loss(**dict(_term_inputs(3), pixels_j=torch.zeros(2, 2)))
    fake.calls.clear()
    with losses.unfused():                       # the torch restatement, whatever the inputs
        losses.reprojection_loss(**_term_inputs(3))
    assert fake.calls == []


def test_pair_enters_the_library_once_and_never_in_backward(fake):
    n = 6
    d = [torch.ones(1, n, 1, requires_grad=True) for _ in range(4)]           # as a render returns them
    Ps, Po = torch.eye(4)[:3].clone().requires_grad_(), torch.eye(4).requires_grad_()
    px = torch.zeros(n, 2)
    loss, stats = losses.correspondence_pair_loss(px.long(), px, d[0], d[1], torch.eye(3), torch.eye(3), Ps, Po, torch.ones(n, 1), d[2], d[3],
                                                  loss_type="l1", pixel_thresh=5.0)
    given = dict(pixels_self=True, pixels_other=True, depth_self=True, depth_other=True, depth_fine_self=True, depth_fine_other=True, K_self=True,
                 K_other=True, pose_self=True, pose_other=True, weights=True, n=n, loss_type=1, pix_check=1, pix_thresh=5.0, depth_check=0,
                 depth_thresh=0.0, out=True, d_depth_self=True, d_depth_other=True, d_depth_fine_self=True, d_depth_fine_other=True,
                 d_pose_self=True, d_pose_other=True, workspace=False)
    assert fake.calls == [("sparf_reproj_pair_loss", given)]
    assert set(stats) == {"perc_val_pix_rep", "depth_in_corr_loss"}
    loss.backward()
    assert fake.names() == ["sparf_reproj_pair_loss"]
    assert all(t.grad.shape == (1, n, 1) for t in d) and Ps.grad.shape == (3, 4) and Po.grad.shape == (4, 4)
    # no fine depths, frozen other view and pose
    fake.calls.clear()
    ds = torch.ones(n, requires_grad=True)
    loss, stats = losses.correspondence_pair_loss(px, px, ds, torch.ones(n), torch.eye(3), torch.eye(3), Ps, torch.eye(4), None)
    assert fake.calls == [("sparf_reproj_pair_loss", dict(given, depth_fine_self=False, depth_fine_other=False, weights=False, loss_type=0,
                                                          pix_check=0, pix_thresh=0.0, d_depth_other=False, d_depth_fine_self=False,
                                                          d_depth_fine_other=False, d_pose_other=False))]
    assert set(stats) == {"depth_in_corr_loss"}
    with pytest.raises(ValueError):
        losses.correspondence_pair_loss(px, px, ds, ds, torch.eye(3), torch.eye(3), Ps, Po, None, depth_fine_self=ds)


def test_constants_that_need_a_gradient_take_the_restatement(monkeypatch):
    """the kernels give no gradient to K, the pixels or the weights: such a call is torch's (and so is any CPU or float64 call)"""
    seen = []
    monkeypatch.setattr(ops.ReprojLoss, "apply", lambda *a: seen.append(a))
    a = _term_inputs(4)
    a["intr_i"] = torch.eye(3).requires_grad_()
    loss, _ = losses.reprojection_loss(**a)
    assert seen == [] and loss.requires_grad
    on_gpu = lambda **kw: types.SimpleNamespace(**{**dict(device=torch.device("cuda"), layout=torch.strided, dtype=torch.float32, requires_grad=False), **kw})
    assert losses._takes_kernel((on_gpu(), None), (on_gpu(dtype=torch.int64), None))
    assert not losses._takes_kernel((on_gpu(),), (on_gpu(requires_grad=True),))
    assert not losses._takes_kernel((on_gpu(dtype=torch.float64),), ())
    with losses.unfused():
        assert not losses._takes_kernel((on_gpu(),), ())


def test_no_matches(fake):
    """n = 0, a pair without confident matches: the restatement gives the reference's 0 / 1e-6 = 0; the fused route still makes its one
    call (which launches no kernel) with n = 0"""
    e = torch.zeros(0)
    with losses.unfused():
        loss, stats, valid = losses.reprojection_loss(torch.zeros(0, 2), e.clone().requires_grad_(), torch.eye(3), torch.zeros(0, 2), e, torch.eye(3),
                                                      torch.eye(4), None, pixel_thresh=10.0, depth_thresh=0.1, return_valid_mask=True)
    assert loss.item() == 0.0 and valid.shape == (0, 1) and all(s.item() == 0.0 for s in stats.values())
    d = e.clone().requires_grad_()
    loss, stats = losses.correspondence_pair_loss(torch.zeros(0, 2), torch.zeros(0, 2), d, e, torch.eye(3), torch.eye(3), torch.eye(4)[:3], torch.eye(4)[:3], None)
    assert fake.names() == ["sparf_reproj_pair_loss"] and fake.calls[0][1]["n"] == 0
    loss.backward()
    assert d.grad.shape == (0,)


def test_install_patches_and_uninstall_restores(fx):
    class Theirs:
        def compute_render_and_repro_loss_w_repro_thres(self, *a, **k):
            return "theirs"

    class Derived(Theirs):
        pass

    mod = types.SimpleNamespace(CorrespondencesPairRenderDepthAndGet3DPtsAndReproject=Theirs)
    opt = types.SimpleNamespace(diff_loss_type="huber", renderrepro_do_pixel_reprojection_check=True, renderrepro_do_depth_reprojection_check=False,
                                renderrepro_pixel_reprojection_thresh=R.PIX_THRESH, renderrepro_depth_reprojection_thresh=R.DEPTH_THRESH)
    inp, _ = R.term_case(fx, 65, "huber")
    args = [T(inp[s]) for s in ("pi", "di", "Ki", "pj", "dj", "Kj", "T")] + [T(inp["w"])[:, None]]
    losses.install(mod)
    try:
        with pytest.raises(RuntimeError):
            losses.install(mod)
        stats = {"kept": 1}
        loss, out = Theirs().compute_render_and_repro_loss_w_repro_thres(opt, *args, stats)
        assert out is stats and set(stats) == {"kept", "perc_val_pix_rep"}
        want, _, _ = losses.reprojection_loss_torch(*args, "huber", R.PIX_THRESH, None)
        assert torch.equal(loss, want)
        loss3, _, valid = Derived().compute_render_and_repro_loss_w_repro_thres(opt, *args, {}, return_valid_mask=True)
        assert torch.equal(loss3, want) and valid.shape == (65, 1)
    finally:
        losses.uninstall()
    assert Theirs().compute_render_and_repro_loss_w_repro_thres() == "theirs"
    mod.CorrespondencesPairRenderDepthAndGet3DPtsAndReproject = Derived          # a class that only inherits the method gets none of its own back
    losses.install(mod)
    losses.uninstall()
    assert "compute_render_and_repro_loss_w_repro_thres" not in vars(Derived) and Derived().compute_render_and_repro_loss_w_repro_thres() == "theirs"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "source")), reason="reference tree not present")
def test_reference_pair_loss_after_install(fx):
    """The reference's unmodified compute_loss_on_image_pair on CPU tensors, on an instance made without its constructor whose `net`
    returns fixed depths: after install() against before -- the same loss, stats and pose gradients within 4x the unpatched one's
    distance from the float64 referee.  In a process of its own: the reference's `source` package must not meet dropin/source here."""
    code = """
        import json, types, numpy as np, torch
        from easydict import EasyDict as edict
        from tests import ref_harness, reproj_referee as R
        assert ref_harness.install_reference()
        import source.training.core.corres_loss as cl
        import sparf_amd.losses as losses
        fx = R.fixture()
        n, H, W = 65, 378, 504
        inp, opts = R.pair_case(fx, n, 1, "huber_checks")
        want = R.pair_want(inp, opts)
        t = lambda a: torch.from_numpy(np.array(a))
        obj = object.__new__(cl.CorrespondencesPairRenderDepthAndGet3DPtsAndReproject)
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        obj.grid = torch.stack((xx, yy), dim=-1).float()
        obj.grid_flat = (obj.grid[:, :, 1] * W + obj.grid[:, :, 0]).long()
        obj.device = torch.device("cpu")
        obj.opt = edict(nerf=edict(rand_rays=4096), compute_photo_on_matches=False, diff_loss_type="huber",
                        renderrepro_do_pixel_reprojection_check=True, renderrepro_do_depth_reprojection_check=True,
                        renderrepro_pixel_reprojection_thresh=R.PIX_THRESH, renderrepro_depth_reprojection_thresh=R.DEPTH_THRESH)
        # the matches of the fixture as the maps the method selects from (a pixel drawn twice keeps its last match: fewer than n)
        ps = t(inp["ps"]).long()
        mask = torch.zeros(H, W, dtype=torch.bool)
        corres, conf, slot = torch.zeros(H, W, 2), torch.zeros(H, W, 1), torch.zeros(H, W, dtype=torch.long)
        for i in range(n):
            x, y = int(ps[i, 0]), int(ps[i, 1])
            mask[y, x], corres[y, x], conf[y, x, 0], slot[y, x] = True, t(inp["po"])[i], float(inp["w"][i]), i
        order = slot[mask]
        def run():
            Ps, Po = t(inp["Ps"]).requires_grad_(), t(inp["Po"]).requires_grad_()
            depths = iter([(inp["ds"], inp["fs"]), (inp["do"], inp["fo"])])
            def render(opt, data_dict, pose, intr, H, W, pixels, mode, iter):
                d, f = next(depths)
                return edict(depth=t(d)[order][None, :, None], depth_fine=t(f)[order][None, :, None])
            obj.net = types.SimpleNamespace(render_image_at_specific_pose_and_rays=render)
            loss_dict, stats, _ = obj.compute_loss_on_image_pair(edict(iter=1), torch.zeros(2, H, W, 3), None, None, 0, 1, corres,
                                                                 corres.round().long()[..., :1], conf, mask, Ps, Po, t(inp["Ks"]), t(inp["Ko"]), {}, {}, {})
            loss_dict["corres"].backward()
            return loss_dict["corres"].detach(), {k: float(v) for k, v in stats.items()}, Ps.grad[:3], Po.grad[:3]
        before = run()
        losses.install(cl)
        try:
            after = run()
        finally:
            losses.uninstall()
        sub = {k: (v[order.numpy()] if v is not None and getattr(v, "shape", ())[:1] == (n,) else v) for k, v in inp.items()}
        want = R.pair_want(sub, opts)
        res = dict(loss=[R.fwd_abs(x[0], want["loss"]) for x in (after, before)], stats_equal=after[1] == before[1], keys=sorted(after[1]),
                   d_Ps=[R.rel_l2(x[2], want["d_Ps"]) for x in (after, before)], d_Po=[R.rel_l2(x[3], want["d_Po"]) for x in (after, before)])
        print(json.dumps(res))
    """
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "compat")])
    p = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(res)
    assert res["stats_equal"] and res["keys"] == ["depth_in_corr_loss", "perc_val_depth_rep", "perc_val_pix_rep"]
    for k in ("loss", "d_Ps", "d_Po"):
        ours, theirs = res[k]
        assert ours <= 4 * theirs and theirs > 0, (k, ours, theirs)
