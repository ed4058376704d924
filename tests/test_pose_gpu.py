"""Pose parameterisations on the GPU (csrc/pose.hip): forward and backward of ops.Se3Pose / ComposePose / D9Pose
through sparf_amd.camera against the float64 referee (tests/pose_referee.py, which states the bounds: one fp32 spacing per forward
element, relative L2 <= 2^-22 per gradient tensor) for every case of tests/golden/pose.npz; through the renderer at its smallest
shapes; and captured in a hipGraph.  Reads the fixture only."""
import functools

import numpy as np
import pytest
import torch

from sparf_amd import camera, ops
from sparf_amd.renderer import Graph
from tests import pose_referee as R
from tests.golden.recipe import make_state_dict, ring_cameras, small_opt
from tests.test_hip_gpu import dev

pytestmark = pytest.mark.gpu

FX = functools.lru_cache(maxsize=None)(R.fixture)


def G(a, grad=False):
    return torch.from_numpy(np.array(a)).to(dev()).requires_grad_(grad)


def check_fwd(got, want64, what):
    e = R.fwd_excess(got, want64)
    print(f"{what}: {e:.3f} fp32 spacings, {R.fwd_abs(got, want64):.3e} absolute")
    assert e <= 1.0, (what, e)


def check_grad(got, want64, what):
    e = R.rel_l2(got, want64)
    print(f"{what}: relative L2 {e:.3e}")
    assert np.isfinite(R.to_np(got)).all() and e <= R.GRAD_BOUND, (what, e)


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("case", R.XI_CASES)
def test_se3_against_float64(case, n):
    fx, k = FX(), f"se3_{case}_{n}_"
    xi, base, g_pose, g_refine = (fx[k + s] for s in ("xi", "base", "g_pose", "g_refine"))
    # base NULL
    (r64,), (dxi64,) = R.vjp(R.se3, [xi], [g_pose])
    x = G(xi, True)
    out = camera.lie.se3_to_SE3(x)
    check_fwd(out, r64, "se3_to_SE3")
    out.backward(G(g_pose))
    check_grad(x.grad, dxi64, "d_xi (no base)")
    # base given, both gradients, d_refine given
    (p64, r64), (dxi64, dbase64) = R.vjp(R.se3_chain, [xi, base], [g_pose, g_refine])
    x, b = G(xi, True), G(base, True)
    pose, refine = ops.Se3Pose.apply(x, b, True)
    check_fwd(pose, p64, "pose")
    check_fwd(refine, r64, "refine")
    torch.autograd.backward([pose, refine], [G(g_pose), G(g_refine)])
    check_grad(x.grad, dxi64, "d_xi")
    check_grad(b.grad, dbase64, "d_base")
    # the folded call, a base without a gradient: the same pose bits
    (_, _), (dxi64, _) = R.vjp(R.se3_chain, [xi, base], [g_pose, None])
    x = G(xi, True)
    folded = camera.refine_se3(x, G(base))
    assert torch.equal(folded, pose)
    folded.backward(G(g_pose))
    check_grad(x.grad, dxi64, "d_xi (refine_se3)")


def test_se3_expands_a_single_base_and_takes_a_strided_xi():
    fx, k = FX(), "se3_s0.05_65_"
    xi, base1, g = fx[k + "xi"], fx[k + "base"][:1], fx[k + "g_pose"]
    (p64, _), (dxi64, each64) = R.vjp(R.se3_chain, [xi, np.repeat(base1, 65, 0)], [g, None])       # each64: d base per pose, before the sum
    wide = torch.zeros(65, 12, device=dev())
    wide[:, ::2] = G(xi)
    wide.requires_grad_()
    x, b = wide[:, ::2], G(base1, True)
    assert not x.is_contiguous() and b.shape == (1, 3, 4)
    pose = camera.refine_se3(x, b)
    check_fwd(pose, p64, "pose")
    pose.backward(G(g))
    check_grad(wide.grad[:, ::2], dxi64, "d_xi")
    assert float(wide.grad[:, 1::2].abs().max()) == 0.0
    # d base: the kernel's 65 per-pose gradients (each within the gradient bound of its float64 value) summed by torch's expand backward in
    # fp32: any summation order of n terms stays within (n - 1) * 2^-24 * sum |term| per element (recursive-summation bound)
    slack = (R.GRAD_BOUND + 64 * 2.0 ** -24) * np.abs(each64).sum(0, keepdims=True)
    err = np.abs(R.to_np(b.grad).astype(np.float64) - each64.sum(0, keepdims=True))
    print("d_base over the expansion: worst error / allowance", float((err / slack).max()))
    assert b.grad.shape == (1, 3, 4) and (err <= slack).all()
    # leading dimensions are flattened
    x = G(xi[:64].reshape(4, 16, 6), True)
    out = camera.refine_se3(x, G(np.repeat(base1, 64, 0).reshape(4, 16, 3, 4)))
    assert out.shape == (4, 16, 3, 4) and torch.equal(out.reshape(64, 3, 4), pose[:64])


@pytest.mark.parametrize("n", R.NS)
def test_compose_against_float64(n):
    fx, k = FX(), f"cmp_{n}_"
    (o64,), (da64, db64) = R.vjp(R.compose, [fx[k + "a"], fx[k + "b"]], [fx[k + "g"]])
    a, b = G(fx[k + "a"], True), G(fx[k + "b"], True)
    out = camera.pose.compose([a, b])
    check_fwd(out, o64, "out")
    out.backward(G(fx[k + "g"]))
    check_grad(a.grad, da64, "d_a")
    check_grad(b.grad, db64, "d_b")
    one = camera.pose.compose_pair_b_at_a(G(fx[k + "a"]), G(fx[k + "b"][:1]))          # [1,3,4] against [n,3,4]
    assert one.shape == (n, 3, 4) and torch.equal(one[0], out[0])


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("case", R.D9_CASES)
@pytest.mark.parametrize("inv", [0, 1])
def test_d9_against_float64(case, n, inv):
    fx, k = FX(), f"d9_{case}_{n}_"
    (p64,), (d64,) = R.vjp(lambda x: R.d9_pose(x, inv), [fx[k + "d9"]], [fx[k + "g"]])
    x = G(fx[k + "d9"], True)
    pose = camera.pose_from_d9(x, invert=bool(inv))
    check_fwd(pose, p64, "pose")
    pose.backward(G(fx[k + "g"]))
    check_grad(x.grad, d64, "d_d9")
    if not inv:
        r = G(fx[k + "d9"][:, 3:], True)
        R3 = camera.r6d2mat(r)
        assert torch.equal(R3, pose[:, :, :3])
        R3.backward(G(fx[k + "g"][:, :, :3]))
        (_,), (d64r,) = R.vjp(lambda x: R.d9_pose(x, 0), [fx[k + "d9"]], [fx[k + "g"] * np.array([1, 1, 1, 0.0])])
        check_grad(r.grad, d64r[:, 3:], "d_r6")


def test_no_poses_launch_nothing():
    xi, base = torch.zeros(0, 6, device=dev(), requires_grad=True), torch.zeros(0, 3, 4, device=dev())
    out = camera.refine_se3(xi, base)
    assert out.shape == (0, 3, 4)
    out.sum().backward()
    assert xi.grad.shape == (0, 6)
    assert camera.lie.se3_to_SE3(xi).shape == (0, 3, 4) and camera.pose.compose([base, base]).shape == (0, 3, 4)
    d9 = torch.zeros(0, 9, device=dev(), requires_grad=True)
    camera.pose_from_d9(d9, invert=True).sum().backward()
    assert d9.grad.shape == (0, 9) and camera.r6d2mat(d9[:, 3:]).shape == (0, 3, 3)


H, W, B, RAYS = 12, 16, 3, 8


def _render(graph, opt, pose, intr):
    idx = (torch.arange(RAYS, device=dev()) * 23 + 5) % (H * W)
    torch.manual_seed(17)
    ret = graph.render(opt, pose, H=H, W=W, intr=intr, ray_idx=idx, depth_range=[1.2, 5.2], iter=0, mode="test-optim")
    ((ret.rgb ** 2).sum() + (ret.rgb_fine ** 2).sum() + (ret.depth_fine ** 2).sum()).backward()
    return ret


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("model", ["se3", "d9"])
def test_through_the_renderer(precision, model):
    """3 images x 8 rays x (8 + 8) samples.  Route A: the pose from the kernel, differentiated through it; route B: the same pose bits as
    a leaf.  The renders are equal, and the parameter's gradient is the float64 VJP of what arrived at the pose."""
    opt = small_opt(nerf=dict(sample_intvs=8, sample_intvs_fine=8, rand_rays=B * RAYS), hip=dict(precision=precision))
    graph = Graph(opt, dev())
    graph.nerf.load_state_dict(make_state_dict(opt, 31, 1.0))
    graph.nerf_fine.load_state_dict(make_state_dict(opt, 32, 1.0))
    base, intr = ring_cameras(B, H=H, W=W)
    intr = intr.to(dev())
    fx = FX()
    if model == "se3":
        p_np, base_np = fx["se3_s0.05_3_xi"], base.numpy()
        fused = lambda p: camera.refine_se3(p, G(base_np))
        ref = lambda p: R.se3_chain(p, R.f64(base_np))[0]
    else:
        p_np = R.to_np(torch.cat([base[:, :, 3], base[:, :2, :3].reshape(B, 6)], -1)) + 0.02 * fx["d9_init_3_g"].reshape(B, 12)[:, :9]
        p_np = p_np.astype(np.float32)
        fused = lambda p: camera.pose_from_d9(p)
        ref = lambda p: R.d9_pose(p, False)
    param = G(p_np, True)
    pose_a = fused(param)
    ret_a = _render(graph, opt, pose_a, intr)
    pose_b = pose_a.detach().clone().requires_grad_()
    ret_b = _render(graph, opt, pose_b, intr)
    for key in ("rgb", "rgb_fine", "depth", "depth_fine", "opacity_fine"):
        assert torch.equal(ret_a[key], ret_b[key]), key
    assert float(pose_b.grad.abs().max()) > 0
    (_,), (want,) = R.vjp(ref, [p_np], [R.to_np(pose_b.grad)])
    check_grad(param.grad, want, f"d_{model} through the renderer")


def test_forward_and_backward_capture_in_a_hipgraph():
    """refine_se3 and its backward for 3 poses under torch.cuda.graph on one stream: two replays, xi rewritten in place between them,
    each equal to the eager result bit for bit (no host synchronisation, no readback, nothing allocated by the library)."""
    fx = FX()
    xis = [G(fx["se3_s0.05_3_xi"]), G(fx["se3_s1.5_3_xi"]), G(fx["se3_zero_3_xi"])]
    base, g = G(fx["se3_s0.05_3_base"]), G(fx["se3_s0.05_3_g_pose"])

    def run(x):
        pose = camera.refine_se3(x, base)
        d_xi, = torch.autograd.grad(pose, x, g)
        return pose, d_xi

    eager = []
    for v in xis:
        pose, d_xi = run(v.clone().requires_grad_())
        eager.append((pose.detach().clone(), d_xi.clone()))
    xi = xis[2].clone().requires_grad_()
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(side):                    # allocator warm-up outside the capture
        for _ in range(2):
            run(xi)
    torch.cuda.current_stream(dev()).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pose, d_xi = run(xi)
    for i in (0, 1):
        with torch.no_grad():
            xi.copy_(xis[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pose.detach(), eager[i][0]) and torch.equal(d_xi, eager[i][1]), i
