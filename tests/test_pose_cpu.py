"""Pose parameterisations without a GPU: the torch restatement of sparf_amd.camera against the fixture
(tests/golden/pose.npz: the reference's own fp32 values) and the float64 referee (tests/pose_referee.py, which states the bounds);
the argument checks of the six C-ABI entry points; what the autograd Functions hand the library, over a stand-in that records
calls (tests/pose_fake.py); install() / uninstall(); and, where the reference tree is present, its pose models after install()."""
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

from sparf_amd import camera, lib as L, ops
from tests import pose_fake, pose_referee as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def T(a, grad=False):
    return torch.from_numpy(np.array(a)).requires_grad_(grad)


def held(got, ref32, want64, measure, what):
    """the restatement within 4x the reference's own distance from the referee"""
    d_ref, d_got = measure(ref32, want64), measure(got, want64)
    print(f"{what}: reference {d_ref:.3e}  restatement {d_got:.3e}")
    assert d_got <= 4 * d_ref, (what, d_got, d_ref)


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("case", R.XI_CASES)
def test_torch_se3_restatement_within_the_references_distance(fx, case, n):
    k = f"se3_{case}_{n}_"
    xi, base, g_pose, g_refine = (fx[k + s] for s in ("xi", "base", "g_pose", "g_refine"))
    (pose64, refine64), (dxi64, dbase64) = R.vjp(R.se3_chain, [xi, base], [g_pose, g_refine])
    (_,), (dxi_a64,) = R.vjp(R.se3, [xi], [g_pose])
    x, b = T(xi, True), T(base, True)
    refine = camera.lie.se3_to_SE3(x)
    pose = camera.pose.compose([refine, b])
    held(refine, fx[k + "refine"], refine64, R.fwd_abs, "refine")
    held(pose, fx[k + "pose"], pose64, R.fwd_abs, "pose")
    d_xi, d_base = torch.autograd.grad((pose * T(g_pose)).sum() + (refine * T(g_refine)).sum(), (x, b))
    held(d_xi, fx[k + "d_xi_b"], dxi64, R.rel_l2, "d_xi")
    held(d_base, fx[k + "d_base_b"], dbase64, R.rel_l2, "d_base")
    # the folded form is the same function; without a base the pose is the refinement
    x2 = T(xi, True)
    folded = camera.refine_se3(x2, T(base))
    held(folded, fx[k + "pose"], pose64, R.fwd_abs, "refine_se3")
    x3 = T(xi, True)
    d_a, = torch.autograd.grad((camera.lie.se3_to_SE3(x3) * T(g_pose)).sum(), x3)
    held(d_a, fx[k + "d_xi_a"], dxi_a64, R.rel_l2, "d_xi (no base)")
    if case == "zero":                      # xi starts at exactly zero in the test-time loop: finite, and the reference's
        assert np.isfinite(d_xi.numpy()).all() and np.isfinite(d_a.numpy()).all()
        assert np.array_equal(d_xi.numpy(), fx[k + "d_xi_b"]) and np.array_equal(d_a.numpy(), fx[k + "d_xi_a"])
        assert R.rel_l2(d_xi, dxi64) <= 2.0 ** -20


@pytest.mark.parametrize("n", R.NS)
def test_torch_compose_restatement(fx, n):
    k = f"cmp_{n}_"
    (o64,), (da64, db64) = R.vjp(R.compose, [fx[k + "a"], fx[k + "b"]], [fx[k + "g"]])
    a, b = T(fx[k + "a"], True), T(fx[k + "b"], True)
    out = camera.pose.compose_pair_b_at_a(a, b)
    held(out, fx[k + "out"], o64, R.fwd_abs, "out")
    d_a, d_b = torch.autograd.grad((out * T(fx[k + "g"])).sum(), (a, b))
    held(d_a, fx[k + "d_a"], da64, R.rel_l2, "d_a")
    held(d_b, fx[k + "d_b"], db64, R.rel_l2, "d_b")
    # a single [1,3,4] operand is expanded
    one = camera.pose.compose_pair_b_at_a(T(fx[k + "a"]), T(fx[k + "b"][:1]))
    assert one.shape == (n, 3, 4) and torch.equal(one[0], out[0].detach())


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("case", R.D9_CASES)
@pytest.mark.parametrize("inv", [0, 1])
def test_torch_d9_restatement(fx, case, n, inv):
    k = f"d9_{case}_{n}_"
    (p64,), (d64,) = R.vjp(lambda x: R.d9_pose(x, inv), [fx[k + "d9"]], [fx[k + "g"]])
    x = T(fx[k + "d9"], True)
    p = camera.pose_from_d9(x, invert=bool(inv))
    held(p, fx[k + f"pose{inv}"], p64, R.fwd_abs, "pose")
    d, = torch.autograd.grad((p * T(fx[k + "g"])).sum(), x)
    held(d, fx[k + f"d{inv}"], d64, R.rel_l2, "d_d9")
    if not inv:
        assert torch.equal(camera.r6d2mat(x[:, 3:]).detach(), p[:, :, :3].detach())


def test_restatement_takes_float64_and_leading_dimensions():
    xi = torch.randn(2, 5, 6, dtype=torch.float64) * 0.3
    base = torch.from_numpy(R.d9_pose(torch.randn(2, 5, 9, dtype=torch.float64)).numpy())
    out = camera.refine_se3(xi, base)
    assert out.dtype == torch.float64 and out.shape == (2, 5, 3, 4)
    assert R.rel_l2(out, R.se3_chain(xi, base)[0].numpy()) < 1e-14
    assert camera.pose_from_d9(torch.randn(2, 5, 9)).shape == (2, 5, 3, 4) and camera.r6d2mat(torch.randn(4, 6)).shape == (4, 3, 3)
    p = camera.pose_from_d9(torch.randn(7, 9, dtype=torch.float64))
    assert R.rel_l2(camera.pose.invert(camera.pose.invert(p)), p.numpy()) < 1e-14


def test_entry_points_check_their_arguments_without_a_device():
    """n == 0: 0 and nothing launched; n < 0 or a missing required pointer: 1, decided before any HIP call"""
    lib = L.load()
    buf = np.zeros(64, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)         # host memory: never dereferenced, every call below returns before a launch
    assert lib.sparf_pose_se3_forward(None, None, 0, None, None, None) == 0
    assert lib.sparf_pose_se3_backward(None, None, 0, None, None, None, None, None) == 0
    assert lib.sparf_pose_compose_forward(None, None, 0, None, None) == 0
    assert lib.sparf_pose_compose_backward(None, None, 0, None, None, None, None) == 0
    assert lib.sparf_pose_d9_forward(None, 1, 0, None, None) == 0
    assert lib.sparf_pose_d9_backward(None, 0, 0, None, None, None) == 0
    assert lib.sparf_pose_se3_forward(p, p, -1, p, p, None) == 1
    assert lib.sparf_pose_se3_forward(None, p, 2, p, p, None) == 1 and lib.sparf_pose_se3_forward(p, p, 2, p, None, None) == 1
    assert lib.sparf_pose_se3_backward(p, p, -3, p, p, p, p, None) == 1
    assert lib.sparf_pose_se3_backward(None, p, 2, p, p, p, p, None) == 1 and lib.sparf_pose_se3_backward(p, p, 2, None, p, p, p, None) == 1
    assert lib.sparf_pose_se3_backward(p, p, 2, p, p, None, p, None) == 1
    assert lib.sparf_pose_se3_backward(p, None, 2, p, None, p, p, None) == 1          # d_base asked for without a base
    assert lib.sparf_pose_compose_forward(p, p, -1, p, None) == 1
    for a in ((None, p, 2, p), (p, None, 2, p), (p, p, 2, None)):
        assert lib.sparf_pose_compose_forward(*a, None) == 1
    assert lib.sparf_pose_compose_backward(p, p, -1, p, p, p, None) == 1
    for i in (0, 1, 3, 4, 5):
        a = [p, p, 2, p, p, p]
        a[i] = None
        assert lib.sparf_pose_compose_backward(*a, None) == 1
    assert lib.sparf_pose_d9_forward(p, 0, -1, p, None) == 1 and lib.sparf_pose_d9_forward(None, 0, 2, p, None) == 1
    assert lib.sparf_pose_d9_forward(p, 1, 2, None, None) == 1
    assert lib.sparf_pose_d9_backward(p, 0, -1, p, p, None) == 1
    for i in (0, 3, 4):
        a = [p, 1, 2, p, p]
        a[i] = None
        assert lib.sparf_pose_d9_backward(*a, None) == 1


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(camera, "_on_device", lambda *t: True)        # CPU tensors down the fused route: the stand-in launches nothing
    with pose_fake.installed() as lib:
        yield lib


def test_se3_enters_the_library_once_per_direction_with_null_for_what_it_does_not_need(fake):
    xi, base = torch.zeros(3, 6, requires_grad=True), torch.zeros(1, 3, 4)
    pose = camera.refine_se3(xi, base)                  # [1,3,4] base expanded; it needs no gradient
    assert pose.shape == (3, 3, 4)
    assert fake.calls == [("sparf_pose_se3_forward", dict(xi=True, base=True, n=3, refine_out=False, pose_out=True))]
    pose.sum().backward()
    assert fake.calls[1:] == [("sparf_pose_se3_backward", dict(xi=True, base=True, n=3, d_pose=True, d_refine=False, d_xi=True, d_base=False))]
    assert xi.grad.shape == (3, 6)
    # a base that needs its gradient gets it, summed over the expansion by autograd
    fake.calls.clear()
    base = torch.zeros(1, 3, 4, requires_grad=True)
    camera.refine_se3(xi, base).sum().backward()
    assert fake.calls[1] == ("sparf_pose_se3_backward", dict(xi=True, base=True, n=3, d_pose=True, d_refine=False, d_xi=True, d_base=True))
    assert base.grad.shape == (1, 3, 4)
    # no base: NULL both ways
    fake.calls.clear()
    out = camera.lie.se3_to_SE3(torch.zeros(2, 5, 6, requires_grad=True))
    assert out.shape == (2, 5, 3, 4)
    out.sum().backward()
    assert fake.calls == [("sparf_pose_se3_forward", dict(xi=True, base=False, n=10, refine_out=False, pose_out=True)),
                          ("sparf_pose_se3_backward", dict(xi=True, base=False, n=10, d_pose=True, d_refine=False, d_xi=True, d_base=False))]
    # the refinement as a second output, with a gradient of its own
    fake.calls.clear()
    xi2 = torch.zeros(3, 6, requires_grad=True)
    pose, refine = ops.Se3Pose.apply(xi2, torch.zeros(3, 3, 4), True)
    (pose.sum() + refine.sum()).backward()
    assert fake.calls == [("sparf_pose_se3_forward", dict(xi=True, base=True, n=3, refine_out=True, pose_out=True)),
                          ("sparf_pose_se3_backward", dict(xi=True, base=True, n=3, d_pose=True, d_refine=True, d_xi=True, d_base=False))]
    # nothing differentiable: no backward entry at all
    fake.calls.clear()
    camera.refine_se3(torch.zeros(3, 6), torch.zeros(3, 3, 4))
    assert fake.names() == ["sparf_pose_se3_forward"]


def test_compose_and_d9_enter_the_library_once_per_direction(fake):
    a, b = torch.zeros(4, 3, 4, requires_grad=True), torch.zeros(1, 3, 4)
    out = camera.pose.compose([a, b])
    assert out.shape == (4, 3, 4)
    out.sum().backward()
    assert fake.calls == [("sparf_pose_compose_forward", dict(a=True, b=True, n=4, out=True)),
                          ("sparf_pose_compose_backward", dict(a=True, b=True, n=4, d_out=True, d_a=True, d_b=True))]
    assert a.grad.shape == (4, 3, 4) and b.grad is None
    fake.calls.clear()
    d9 = torch.zeros(5, 9, requires_grad=True)
    camera.pose_from_d9(d9, invert=True).sum().backward()
    assert fake.calls == [("sparf_pose_d9_forward", dict(d9=True, invert=1, n=5, pose_out=True)),
                          ("sparf_pose_d9_backward", dict(d9=True, invert=1, n=5, d_pose=True, d_d9=True))]
    fake.calls.clear()
    r = torch.zeros(2, 3, 6, requires_grad=True)
    R3 = camera.r6d2mat(r)
    assert R3.shape == (2, 3, 3, 3)
    R3.sum().backward()
    assert fake.calls == [("sparf_pose_d9_forward", dict(d9=True, invert=0, n=6, pose_out=True)),
                          ("sparf_pose_d9_backward", dict(d9=True, invert=0, n=6, d_pose=True, d_d9=True))]
    assert r.grad.shape == (2, 3, 6)
    fake.calls.clear()
    with camera.unfused():                       # the torch restatement, whatever the inputs
        camera.pose_from_d9(torch.randn(2, 9))
    assert fake.calls == []


def test_install_patches_and_uninstall_restores():
    class Lie:
        def se3_to_SE3(self, wu):
            return "theirs"

    class Pose:
        def compose(self, pose_list):
            return self.compose_pair_b_at_a(pose_a=pose_list[0], pose_b=pose_list[1])

        def compose_pair_b_at_a(self, pose_a, pose_b):
            return "theirs"

    cam = types.SimpleNamespace(lie=Lie(), pose=Pose())
    two = types.SimpleNamespace(r6d2mat=lambda d6: "theirs")
    theirs = two.r6d2mat
    camera.install(cam, two)
    try:
        with pytest.raises(RuntimeError):
            camera.install(cam)
        xi, base = torch.randn(2, 6) * 0.1, camera.pose_from_d9(torch.randn(2, 9))
        assert torch.equal(cam.lie.se3_to_SE3(xi), camera.se3_to_SE3_torch(xi))
        assert torch.equal(cam.pose.compose([camera.se3_to_SE3_torch(xi), base]), camera.refine_se3(xi, base))      # compose goes through the pair
        assert torch.equal(two.r6d2mat(torch.ones(1, 6)), camera.r6d2mat_torch(torch.ones(1, 6)))
    finally:
        camera.uninstall()
    assert cam.lie.se3_to_SE3(None) == "theirs" and cam.pose.compose([None, None]) == "theirs" and two.r6d2mat is theirs
    assert "se3_to_SE3" not in vars(cam.lie) and "compose_pair_b_at_a" not in vars(cam.pose)
    camera.install(cam)                           # without the 6D module; and again after an uninstall
    camera.uninstall()
    assert two.r6d2mat is theirs


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "source")), reason="reference tree not present")
def test_reference_pose_models_after_install(fx):
    """AxisRotationPoseParameters / FirstTwoColunmnsPoseParameters .get_w2c_poses() on CPU tensors: patched against unpatched, both
    against the float64 referee -- the patched result within 4x the unpatched one's distance.  In a process of its own: the
    reference's `source` package must not meet dropin/source in this one."""
    code = """
        import json, numpy as np, torch
        from easydict import EasyDict as edict
        import source.utils.camera as rcam
        import source.models.poses_models.two_columns as two
        from source.models.poses_models.axis_rotation import AxisRotationPoseParameters
        import sparf_amd.camera as camera
        from tests import pose_referee as R
        fx = R.fixture()
        xi, base = fx["se3_s0.05_3_xi"], torch.from_numpy(fx["se3_s0.05_3_base"])
        opt = edict(camera=edict(optimize_relative_poses=False, n_first_fixed_poses=0, optimize_c2w=False, optimize_trans=True, optimize_rot=True))
        res = {}
        axis = AxisRotationPoseParameters(opt, 3, base, torch.device("cpu"))
        with torch.no_grad():
            axis.pose_embedding.copy_(torch.from_numpy(xi))
        want = R.se3_chain(R.f64(xi), R.f64(base))[0].numpy()
        d9 = fx["d9_init_3_d9"]
        for c2w in (False, True):
            opt.camera.optimize_c2w = c2w
            six = two.FirstTwoColunmnsPoseParameters(opt, 3, base, torch.device("cpu"))
            with torch.no_grad():
                six.pose_embedding.copy_(torch.from_numpy(d9))
            want6 = R.d9_pose(R.f64(d9), c2w).numpy()
            theirs_axis, theirs_six = axis.get_w2c_poses().detach(), six.get_w2c_poses().detach()
            camera.install(rcam, two)
            try:
                assert rcam.lie.se3_to_SE3.__func__ is camera.Lie.se3_to_SE3 and two.r6d2mat is camera.r6d2mat
                ours_axis, ours_six = axis.get_w2c_poses().detach(), six.get_w2c_poses().detach()
            finally:
                camera.uninstall()
            assert two.r6d2mat is not camera.r6d2mat
            res["axis"] = (R.fwd_abs(ours_axis, want), R.fwd_abs(theirs_axis, want))
            res["six_c2w" if c2w else "six_w2c"] = (R.fwd_abs(ours_six, want6), R.fwd_abs(theirs_six, want6))
        print(json.dumps(res))
    """
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "compat"), REF])
    p = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(res)
    assert set(res) == {"axis", "six_w2c", "six_c2w"}
    for k, (ours, theirs) in res.items():
        assert theirs > 0 and ours <= 4 * theirs, (k, ours, theirs)
