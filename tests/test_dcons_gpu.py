"""The depth-consistency kernels on the device (csrc/dcons.hip behind ops.DconsProject / DconsSelect / DconsLoss and
sparf_amd.losses): every fixture case (tests/golden/dcons.npz -- the reference tree is never read here) against the float64 referee at
the bounds tests/dcons_referee.py states, and against the reference's own fp32 values; the mask patterns; determinism; the input forms
the glue accepts; n = 0 and count = 0; graph capture of the loss; and the chain behind real renders end to end.
Run with `pytest -m gpu`."""
import types

import numpy as np
import pytest
import torch

from sparf_amd import losses
from tests import dcons_referee as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def D(a, grad=False):
    return torch.from_numpy(np.array(a)).to(dev()).requires_grad_(grad) if a is not None else None


def N(t):
    return t.detach().cpu().numpy()


def no_farther(got, ref32, want64, bound_abs, what):
    """the kernel is no farther from the reference's fp32 value than the reference is from float64, plus the kernel's own bound"""
    d_got_ref = R.l2(np.asarray(got, dtype=np.float64) - np.asarray(ref32, dtype=np.float64))
    d_ref = R.l2(np.asarray(ref32, dtype=np.float64) - want64)
    print(f"{what}: kernel to reference {d_got_ref:.3e}  reference to float64 {d_ref:.3e}  bound {bound_abs:.3e}")
    assert d_got_ref <= d_ref + bound_abs, (what, d_got_ref, d_ref, bound_abs)


def spacings(want64):
    """the L2 norm of one fp32 spacing per element"""
    return R.l2(np.spacing(np.abs(np.asarray(want64)).astype(np.float32)))


def run_project(fx, px=None, d=None, Xw=None, rows34=False, upstream=True):
    """one fused project call and its backward -> dict(uv, z, index, dst, count, d_in) as numpy"""
    H, W = (int(v) for v in fx["HW"])
    P, Tc = (fx["P_unseen"][:3], fx["T_c2w"][:3]) if rows34 else (fx["P_unseen"], fx["T_c2w"])
    if Xw is not None:
        leaf = D(Xw, True)
        uv, z, index = losses.depth_consistency_project(leaf, D(P), D(fx["K"]), H, W, D(fx["depth_min"]))
    else:
        leaf = D(d, True)
        uv, z, index = losses.depth_consistency_project(None, D(P), D(fx["K"]), H, W, float(fx["depth_min"]), pixels_ref=D(px), depth_ref=leaf,
                                                        intr_ref=D(fx["K"]), pose_c2w_ref=D(Tc))
    assert type(uv.grad_fn).__name__.startswith("DconsProject"), "the fused route was not taken"
    dst = uv.grad_fn.saved_tensors[-1]
    out = dict(uv=N(uv), z=N(z), index=N(index), dst=N(dst), count=uv.shape[0])
    if upstream:
        n = leaf.shape[0]
        src = out["index"].astype(np.int64)
        out["d_in"] = N(torch.autograd.grad((uv * D(R.g_uv(n)[src])).sum() + (z * D(R.g_z(n)[src])).sum(), leaf)[0]) if n else np.zeros(leaf.shape)
    return out


def check_project(got, want, what):
    assert got["count"] == want["count"] and np.array_equal(got["index"], want["src"]) and np.array_equal(got["dst"], want["dst"]), what
    assert np.all(np.diff(got["index"]) > 0), "the compacted rows are in source order"
    figures = dict(uv=R.fwd_excess(got["uv"], want["uv"]), z=R.fwd_excess(got["z"], want["z"]), d_in=R.rel_l2(got["d_in"], want["d_in"]))
    print(what, figures)
    assert figures["uv"] <= 1 and figures["z"] <= 1 and figures["d_in"] <= R.GRAD_BOUND, (what, figures)
    assert not got["d_in"][want["dst"] < 0].any(), "zeros where dst < 0"


@pytest.mark.parametrize("n", R.NS)
def test_project_against_the_referee_and_the_reference(fx, n):
    src = R.project_want(fx, n)["src"]
    guv, gz = R.g_uv(n)[src], R.g_z(n)[src]
    want = R.project_want(fx, n, guv=guv, gz=gz)
    got = run_project(fx, px=fx["px"][:n], d=fx["d"][:n])
    check_project(got, want, f"back-projecting n={n}")
    mask = want["mask"]
    assert np.array_equal(mask, fx["valid"][:n])
    if want["count"]:
        no_farther(got["uv"], R.ref_of(fx, "uv", n)[mask], want["uv"], spacings(want["uv"]), "uv")
        no_farther(got["z"], R.ref_of(fx, "z", n)[mask], want["z"], spacings(want["z"]), "z")
        no_farther(got["d_in"], R.ref_of(fx, "d_d", n), want["d_in"], R.GRAD_BOUND * R.l2(want["d_in"]), "d_depth_ref")
    # [3,4] poses and integer pixels: the same bits
    H, W = (int(v) for v in fx["HW"])
    uv, z, index = losses.depth_consistency_project(None, D(fx["P_unseen"][:3]), D(fx["K"]), H, W, D(fx["depth_min"]), pixels_ref=D(fx["px"][:n]).long(),
                                                    depth_ref=D(fx["d"][:n])[:, None], intr_ref=D(fx["K"]), pose_c2w_ref=D(fx["T_c2w"][:3]))
    assert np.array_equal(N(uv), got["uv"]) and np.array_equal(N(z), got["z"]) and np.array_equal(N(index), got["index"])
    # the points form fed with the referee's world points (as float32, what a caller holds), against the referee on those points
    Xw = want["Xw"].astype(np.float32)
    wantp = R.project_want(fx, n, Xw=Xw, guv=guv, gz=gz)
    assert np.array_equal(wantp["mask"], mask)
    gotp = run_project(fx, Xw=Xw)
    check_project(gotp, wantp, f"points n={n}")
    if n in R.POINTS_NS and want["count"]:
        assert np.array_equal(Xw, fx["Xw"][:n])
        no_farther(gotp["uv"], fx[f"uv_p_{n}"][mask], wantp["uv"], spacings(wantp["uv"]), "uv (points)")
        no_farther(gotp["z"], fx[f"z_p_{n}"][mask], wantp["z"], spacings(wantp["z"]), "z (points)")
        no_farther(gotp["d_in"], fx[f"d_Xw_{n}"], wantp["d_in"], R.GRAD_BOUND * R.l2(wantp["d_in"]), "d_points_w")


@pytest.mark.parametrize("base", R.PATTERN_BASES)
@pytest.mark.parametrize("pattern", R.PATTERNS[1:])
def test_project_mask_patterns(fx, pattern, base):
    """the rows of the first `base` points rearranged into each mask pattern (`all` of the larger base takes the counts launch):
    against the referee, and against the reference's own run on those rows"""
    rows = R.pattern_rows(fx["valid"][:base], pattern)
    n = len(rows)
    px, d = fx["px"][rows], fx["d"][rows]
    src = R.project_want(fx, n, px=px, d=d)["src"]
    want = R.project_want(fx, n, px=px, d=d, guv=R.g_uv(n)[src], gz=R.g_z(n)[src])
    assert want["count"] == dict(all=n, none=0, first=1, last=1, alternating=n // 2)[pattern]
    assert pattern != "all" or base != R.PATTERN_BASES[-1] or n > 4096
    got = run_project(fx, px=px, d=d)
    check_project(got, want, f"{pattern} of {base}: n={n}")
    mask = want["mask"]
    assert np.array_equal(mask, fx["valid"][rows])
    if want["count"]:
        no_farther(got["uv"], R.ref_of(fx, "uv", base, pattern)[mask], want["uv"], spacings(want["uv"]), "uv")
        no_farther(got["z"], R.ref_of(fx, "z", base, pattern)[mask], want["z"], spacings(want["z"]), "z")
        no_farther(got["d_in"], R.ref_of(fx, "d_d", base, pattern), want["d_in"], R.GRAD_BOUND * R.l2(want["d_in"]), "d_depth_ref")


def select_patterns(n):
    k = np.arange(n)
    one = lambda i: (k == i).astype(np.float32)
    return dict(drawn=R.vis(n), all=np.ones(n, dtype=np.float32), none=np.zeros(n, dtype=np.float32), first=one(0), last=one(n - 1),
                alternating=(k % 2 == 0).astype(np.float32))


@pytest.mark.parametrize("n", R.NS)
def test_select_is_the_ordered_boolean_index(fx, n):
    uv, z = fx["uv"][:n], fx["z"][:n]
    for pattern, vis in select_patterns(n).items():
        dst, src, count = R.compaction(vis >= np.float32(R.VIS_THRESH))
        tu, tz = D(uv, True), D(z, True)
        uv_o, z_o, vis_o, index = losses.visibility_select(D(vis), tu, tz)
        assert type(uv_o.grad_fn).__name__.startswith("DconsSelect"), "the fused route was not taken"
        assert uv_o.shape == (count, 2) and np.array_equal(N(index), src) and np.array_equal(N(uv_o.grad_fn.saved_tensors[0]), dst), (pattern, n)
        assert np.array_equal(N(uv_o), uv[src]) and np.array_equal(N(z_o), z[src]) and np.array_equal(N(vis_o), vis[src]), (pattern, n)
        g_uv, g_z = torch.autograd.grad((uv_o * D(R.g_uv(n)[src])).sum() + (z_o * D(R.g_z(n)[src])).sum(), (tu, tz), allow_unused=True)
        want_uv, want_z = np.zeros((n, 2), dtype=np.float32), np.zeros(n, dtype=np.float32)
        want_uv[src], want_z[src] = R.g_uv(n)[src], R.g_z(n)[src]
        assert np.array_equal(N(g_uv), want_uv) and np.array_equal(N(g_z), want_z), (pattern, n)      # a gather: exact


def run_loss(inp, loss_type, shapes=False):
    t = [D(a, i in (0, 2, 4)) for i, a in enumerate(inp)]
    a = list(t)
    if shapes:                   # as a caller holds them: vis [m,1], render results [1,m,1]
        a[1] = a[1][:, None]
        a[2:] = [x[None, :, None] if x is not None else None for x in a[2:]]
    loss, avg = losses.depth_consistency_loss(*a, loss_type=loss_type)
    assert type(loss.grad_fn).__name__.startswith("DconsLoss"), "the fused route was not taken"
    leaves = [x for i, x in enumerate(t) if i in (0, 2, 4) and x is not None]
    out = dict(loss=N(loss), avg=N(avg))
    out.update({k: N(g) for k, g in zip(("d_zp", "d_depth", "d_depth_fine"), torch.autograd.grad(loss, leaves))})
    return out


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("case", R.LOSS_CASES)
def test_loss_against_the_referee_and_the_reference(fx, case, n):
    loss_type, fine = R.LOSS_CASES[case]
    inp = R.loss_inputs(fx, n, fine)
    want, got = R.loss_want(*inp, loss_type), run_loss(inp, loss_type)
    keys = ("d_zp", "d_depth", "d_depth_fine")[:3 if fine else 2]
    figures = dict(loss=R.fwd_excess(got["loss"], want["loss"]), avg=R.fwd_excess(got["avg"], want["avg"]))
    figures.update({k: R.rel_l2(got[k], want[k]) for k in keys})
    figures.update({k + "_elem": R.fwd_excess(got[k], want[k]) for k in keys})
    print(figures)
    assert figures["loss"] <= 1 and figures["avg"] <= 1
    assert all(figures[k] <= R.GRAD_BOUND and figures[k + "_elem"] <= 1 for k in keys)
    ref = fx[f"loss_{case}_{n}"]
    no_farther(got["loss"], ref[0], want["loss"], spacings(want["loss"]), "loss")
    no_farther(got["avg"], ref[1], want["avg"], spacings(want["avg"]), "avg_vis_weight")
    if n in R.SEED_NS:
        for k, r in zip(keys, fx[f"seeds_{case}_{n}"]):
            no_farther(got[k], r, want[k], R.GRAD_BOUND * R.l2(want[k]), k)
    shaped = run_loss(inp, loss_type, shapes=True)
    assert all(np.array_equal(shaped[k].reshape(-1), got[k].reshape(-1)) for k in got)


@pytest.mark.parametrize("n", [257, 8200])
def test_two_calls_give_the_same_bits(fx, n):
    a, b = (run_project(fx, px=fx["px"][:n], d=fx["d"][:n]) for _ in range(2))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    inp = R.loss_inputs(fx, n, 1)
    a, b = run_loss(inp, "huber"), run_loss(inp, "huber")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    vis = D(R.vis(n))
    a, b = (losses.visibility_select(vis, D(fx["uv"][:n], True), D(fx["z"][:n])) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_strided_inputs_give_the_bits_of_the_dense_call(fx):
    n = 257
    dense = run_project(fx, px=fx["px"][:n], d=fx["d"][:n])

    def strided(a, cols):
        big = torch.full((n, 2 * cols + 1), 7.0, device=dev())
        big[:, ::2][:, :cols] = D(a).reshape(n, cols)
        return big[:, ::2][:, :cols]

    H, W = (int(v) for v in fx["HW"])
    d = strided(fx["d"][:n], 1).requires_grad_()                            # [n,1], stride (3, 2)
    P = D(np.ascontiguousarray(fx["P_unseen"].T)).T                          # a transposed view
    assert not d.is_contiguous() and not P.is_contiguous()
    uv, z, index = losses.depth_consistency_project(None, P, D(fx["K"]), H, W, float(fx["depth_min"]), pixels_ref=strided(fx["px"][:n], 2), depth_ref=d,
                                                    intr_ref=D(fx["K"]), pose_c2w_ref=D(fx["T_c2w"]))
    src = dense["index"].astype(np.int64)
    g, = torch.autograd.grad((uv * D(R.g_uv(n)[src])).sum() + (z * D(R.g_z(n)[src])).sum(), d)
    assert g.shape == (n, 1) and np.array_equal(N(g)[:, 0], dense["d_in"])
    assert np.array_equal(N(uv), dense["uv"]) and np.array_equal(N(z), dense["z"]) and np.array_equal(N(index), dense["index"])
    # select on strided rows and a [m,1] visibility; the loss on strided operands
    vis = R.vis(n)
    a = losses.visibility_select(D(vis), D(fx["uv"][:n], True), D(fx["z"][:n]))
    b = losses.visibility_select(strided(vis, 1), strided(fx["uv"][:n], 2).requires_grad_(), strided(fx["z"][:n], 1)[:, 0])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    inp = R.loss_inputs(fx, n, 1)
    want = run_loss(inp, "huber")
    t = [strided(x, 1) for x in inp]
    t[2].requires_grad_()
    loss, avg = losses.depth_consistency_loss(*t)
    assert np.array_equal(N(loss), want["loss"]) and np.array_equal(N(avg), want["avg"])
    assert np.array_equal(N(torch.autograd.grad(loss, t[2])[0])[:, 0], want["d_depth"])


def test_no_points_and_nothing_kept(fx):
    """n = 0 and count = 0 launch nothing and return the reference's empty result"""
    H, W = (int(v) for v in fx["HW"])
    e = lambda *s: torch.zeros(*s, device=dev())
    Xw = e(0, 3).requires_grad_()
    uv, z, index = losses.depth_consistency_project(Xw, D(fx["P_unseen"]), D(fx["K"]), H, W, 1.2)
    assert type(uv.grad_fn).__name__.startswith("DconsProject") and uv.shape == (0, 2) and z.shape == (0,) and index.shape == (0,)
    (uv.sum() + z.sum()).backward()
    assert Xw.grad.shape == (0, 3)
    # every point behind depth_min: the selections are empty, the gradient zero
    d = D(fx["d"][:65], True)
    uv, z, index = losses.depth_consistency_project(None, D(fx["P_unseen"]), D(fx["K"]), H, W, 100.0, pixels_ref=D(fx["px"][:65]), depth_ref=d,
                                                    intr_ref=D(fx["K"]), pose_c2w_ref=D(fx["T_c2w"]))
    assert uv.shape == (0, 2) and z.shape == (0,) and index.shape == (0,)
    uv2, z2, v2, i2 = losses.visibility_select(e(0), uv, z)
    assert type(uv2.grad_fn).__name__.startswith("DconsSelect") and uv2.shape == (0, 2) and v2.shape == (0,) and i2.shape == (0,)
    dep = e(0).requires_grad_()
    loss, avg = losses.depth_consistency_loss(z2, v2, dep, e(0), dep * 1.0, e(0))
    assert type(loss.grad_fn).__name__.startswith("DconsLoss") and loss.item() == 0.0 and avg.item() == 0.0
    loss.backward()
    assert d.grad.shape == (65,) and not d.grad.any() and dep.grad.shape == (0,)
    uv3, z3, v3, _ = losses.visibility_select(e(65), D(fx["uv"][:65], True), D(fx["z"][:65]))          # nothing visible
    assert uv3.shape == (0, 2) and z3.shape == (0,) and v3.shape == (0,)


@pytest.mark.parametrize("n", [1025, 4097])
def test_graph_replays_of_the_loss_give_the_eager_bits(fx, n):
    """below and above the one-workgroup limit (the workspace is allocated inside the capture); forward and seeds"""
    t = [D(a) for a in R.loss_inputs(fx, n, 1)]
    t[0].requires_grad_(), t[2].requires_grad_(), t[4].requires_grad_()

    def step():
        loss, avg = losses.depth_consistency_loss(*t, loss_type="huber")
        return (loss, avg) + torch.autograd.grad(loss, (t[0], t[2], t[4]))

    eager = [x.detach().clone() for x in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for _ in range(2):
        for x in static:
            x.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b.detach()) for a, b in zip(eager, static))


def test_chain_behind_real_renders():
    """The renderer's smallest shapes: a 65-ray render of a reference view, its fine depth back-projected and projected into an unseen
    view, render_to_max there, the visibility selection, the render at the kept pixels, the loss, backward.  The render from the fused
    pixel list EQUALS the render from the same bits as a leaf, and the parameter and depth_ref gradients through the fused chain EQUAL
    those from feeding the ops' own seeds into the same renders by hand -- the plumbing adds nothing of its own.  Then the replacement
    method on the same renders."""
    from sparf_amd.edict import EasyDict as edict
    from sparf_amd.renderer import Graph
    from tests.golden.recipe import small_opt
    H, W, n = 40, 60, 65
    gen = torch.Generator().manual_seed(11)
    ps = torch.stack([torch.randint(0, W, (n,), generator=gen), torch.randint(0, H, (n,), generator=gen)], 1).to(dev())
    intr = torch.tensor([[50.0, 0, W / 2], [0, 50.0, H / 2], [0, 0, 1]], device=dev())
    P_ref = torch.tensor([[1.0, 0, 0, 0.1], [0, 1, 0, 0], [0, 0, 1, 3.0]], device=dev())
    P_un = torch.tensor([[1.0, 0, 0, -0.1], [0, 1, 0, 0.05], [0, 0, 1, 3.05], [0, 0, 0, 1]], device=dev())
    c2w_ref = losses.pose_inverse_4x4_torch(torch.cat([P_ref, P_un[3:]]))
    data = edict(depth_range=torch.tensor([[1.5, 4.5]] * 2, device=dev()), iter=10)
    thresh = 0.2

    def run(by_hand):
        opt = small_opt(hip=dict(lazy_batch=True))
        torch.manual_seed(0)
        g = Graph(opt, dev())
        g.train()
        torch.manual_seed(3)
        ref = g.render_image_at_specific_pose_and_rays(opt, data, P_ref, intr, H, W, iter=10, pixels=ps, mode="train")
        depth_ref = ref.depth_fine
        depth_ref.retain_grad()
        uv, zp, index = losses.depth_consistency_project(None, P_un, intr, H, W, data.depth_range[0][0], pixels_ref=ps, depth_ref=depth_ref,
                                                         intr_ref=intr, pose_c2w_ref=c2w_ref)
        assert type(uv.grad_fn).__name__.startswith("DconsProject") and 0 < uv.shape[0] <= n
        with torch.no_grad():
            far = g.render_up_to_maxdepth_at_specific_pose_and_rays(opt, data, P_un[:3], intr, H, W, depth_max=zp, pixels=uv, mode="train", iter=10)
        vis = far["all_cumulated_fine"].squeeze(0)
        uv2, zp2, v, index2 = losses.visibility_select(vis, uv, zp, thresh)
        assert type(uv2.grad_fn).__name__.startswith("DconsSelect") and uv2.shape[0] > 0
        pixels, pseudo = (uv2.detach().requires_grad_(), zp2.detach().requires_grad_()) if by_hand else (uv2, zp2)
        ret = g.render_image_at_specific_pose_and_rays(opt, data, P_un[:3], intr, H, W, pixels=pixels, mode="train", iter=10)
        loss, avg = losses.depth_consistency_loss(pseudo, v, ret.depth, ret.opacity, ret.depth_fine, ret.opacity_fine)
        assert type(loss.grad_fn).__name__.startswith("DconsLoss")
        loss.backward()
        if by_hand:              # what reached the leaves, into the ops' own backward
            torch.autograd.backward([uv2, zp2], [pixels.grad, pseudo.grad])
        params = {k: p.grad for k, p in g.named_parameters() if not k.endswith("progress")}
        return dict(loss=loss.detach(), depth=ret.depth.detach(), depth_fine=ret.depth_fine.detach(), counts=(uv.shape[0], uv2.shape[0]),
                    d_depth_ref=depth_ref.grad, params=params, avg=avg, graph=g, opt=opt)

    a, b = run(False), run(True)
    print("rays kept by the mask / by the visibility:", a["counts"])
    assert a["counts"] == b["counts"] and torch.equal(a["depth"], b["depth"]) and torch.equal(a["depth_fine"], b["depth_fine"])
    assert torch.equal(a["loss"], b["loss"]) and torch.isfinite(a["loss"]) and float(a["loss"]) > 0
    assert a["d_depth_ref"] is not None and float(a["d_depth_ref"].abs().max()) > 0 and torch.equal(a["d_depth_ref"], b["d_depth_ref"])
    assert a["params"] and all(v is not None and torch.isfinite(v).all() for v in a["params"].values())
    for k, v in a["params"].items():
        assert torch.equal(v, b["params"][k]), k
    # the replacement method on the same graph and draws: the same loss as the three calls
    g, opt = a["graph"], a["opt"]
    for p in g.parameters():
        p.grad = None
    mod = types.SimpleNamespace(DepthConsistencyLoss=type("Theirs", (), {}))
    losses.install_depth_consistency(mod)
    try:
        obj = mod.DepthConsistencyLoss()
        obj.net, obj.device = g, dev()
        obj.opt = edict(opt)
        obj.opt.update(diff_loss_type="huber", gradually_decrease_depth_cons_loss=True, depth_cons_loss_reduct_at_x_iter=5)
        torch.manual_seed(3)
        ref = g.render_image_at_specific_pose_and_rays(opt, data, P_ref, intr, H, W, iter=10, pixels=ps, mode="train")
        pts = losses.backproject_to_3d_torch(ps.float(), ref.depth_fine.reshape(-1), intr, c2w_ref)
        loss_dict, stats, _ = obj.compute_loss_at_sampled_pose(data, P_un, intr, pts, H, W, ps)
        assert set(stats) == {"nbr_px_sampling", "avg_vis_weight"} and stats["nbr_px_sampling"] == n
        assert type(loss_dict["depth_cons"].grad_fn).__name__.startswith("Div")
        assert torch.isfinite(loss_dict["depth_cons"]) and float(loss_dict["depth_cons"]) > 0
        # (gamma = 2 ** (10 // 5); the world points are torch's fp32 here, so the loss is close to, not equal to, the chain's)
        assert abs(float(loss_dict["depth_cons"]) * 4 - float(a["loss"])) <= 1e-3 * float(a["loss"])
        loss_dict["depth_cons"].backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for k, p in g.named_parameters() if not k.endswith("progress"))
    finally:
        losses.uninstall_depth_consistency()
