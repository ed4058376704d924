"""The correspondence-loss kernels on the device (csrc/reproj.hip behind ops.ReprojLoss / ReprojPairLoss and
sparf_amd.losses): every fixture case (tests/golden/reproj.npz -- the reference tree is never read here) against the float64 referee at
the bounds tests/reproj_referee.py states, and against the reference's own fp32 values; determinism; the input forms the glue accepts;
n = 0; the replacement method; graph capture; and the loss behind two pixel-list renders end to end.  Run with `pytest -m gpu`."""
import types

import numpy as np
import pytest
import torch

from sparf_amd import losses
from tests import reproj_referee as R

pytestmark = pytest.mark.gpu

TERM_IDS = [(n, case) for n in R.NS for case in R.CASES]
PAIR_IDS = [(n, fine, case) for n in R.PAIR_NS for fine in (0, 1) for case in R.PAIR_CASES]
PAIR_DEPTHS = ("ds", "do", "fs", "fo")


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def wants(fx):
    """the float64 values of every fixture case, computed once"""
    out = {}
    for n, case in TERM_IDS:
        out[(n, case)] = R.term_want(*R.term_case(fx, n, case))
    for n, fine, case in PAIR_IDS:
        out[(n, fine, case)] = R.pair_want(*R.pair_case(fx, n, fine, case))
    return out


def D(a, grad=False):
    return torch.from_numpy(np.array(a)).to(dev()).requires_grad_(grad) if a is not None else None


def run_term(inp, opts, **forms):
    """-> dict(loss, stats [2], valid [n], d_di, d_T) as numpy, from one fused call and its backward"""
    di, Tt = D(inp["di"], True), D(inp["T"], True)
    w = D(inp["w"])[:, None] if inp["w"] is not None else None
    loss, stats, valid = losses.reprojection_loss(D(inp["pi"]), di, D(inp["Ki"]), D(inp["pj"]), D(inp["dj"]), D(inp["Kj"]), Tt, w,
                                                  return_valid_mask=True, **opts)
    assert loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith("ReprojLoss"), "the fused route was not taken"
    d_di, d_T = torch.autograd.grad(loss, (di, Tt))
    st = [stats.get(k, torch.zeros(())).item() for k in ("perc_val_pix_rep", "perc_val_depth_rep")]
    return dict(loss=loss.detach().cpu().numpy(), stats=np.array(st, dtype=np.float32), valid=valid.cpu().numpy()[:, 0], d_di=d_di.cpu().numpy(),
                d_T=d_T.cpu().numpy())


def run_pair(inp, opts, poses34=False):
    leaves = {s: D(inp[s], True) for s in PAIR_DEPTHS + ("Ps", "Po") if inp[s] is not None}
    if poses34:
        leaves["Ps"], leaves["Po"] = D(inp["Ps"][:3], True), D(inp["Po"][:3], True)
    loss, stats = losses.correspondence_pair_loss(D(inp["ps"]), D(inp["po"]), leaves["ds"], leaves["do"], D(inp["Ks"]), D(inp["Ko"]), leaves["Ps"],
                                                  leaves["Po"], D(inp["w"])[:, None], leaves.get("fs"), leaves.get("fo"), **opts)
    assert type(loss.grad_fn).__name__.startswith("ReprojPairLoss"), "the fused route was not taken"
    out = dict(loss=loss.detach().cpu().numpy(), stats=np.array([stats.get(k, torch.zeros(())).item() for k in losses.STAT_KEYS], dtype=np.float32))
    for s, g in zip(leaves, torch.autograd.grad(loss, list(leaves.values()))):
        out["d_" + s] = g.cpu().numpy()
    return out


def l2(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


def no_farther(got, ref32, want64, bound_abs, what):
    """the kernel is no farther from the reference's fp32 value than the reference is from float64, plus the kernel's own bound"""
    d_got_ref = l2(np.asarray(got, dtype=np.float64) - np.asarray(ref32, dtype=np.float64))
    d_ref = l2(np.asarray(ref32, dtype=np.float64) - want64)
    print(f"{what}: kernel to reference {d_got_ref:.3e}  reference to float64 {d_ref:.3e}  bound {bound_abs:.3e}")
    assert d_got_ref <= d_ref + bound_abs, (what, d_got_ref, d_ref, bound_abs)


def spacing(want64):
    return float(np.max(np.spacing(np.abs(np.asarray(want64)).astype(np.float32))))


@pytest.mark.parametrize("n,case", TERM_IDS)
def test_term_against_the_referee_and_the_reference(fx, wants, n, case):
    inp, opts = R.term_case(fx, n, case)
    want, got, k = wants[(n, case)], run_term(inp, opts), f"t{n}_{case}_"
    figures = dict(loss=R.fwd_excess(got["loss"], want["loss"]), stats=R.fwd_excess(got["stats"], want["stats"]),
                   d_di_elem=R.fwd_excess(got["d_di"], want["d_di"]), d_di=R.rel_l2(got["d_di"], want["d_di"]), d_T=R.rel_l2(got["d_T"], want["d_T"]))
    print(figures)
    assert np.array_equal(got["valid"], want["valid"]) and np.array_equal(got["valid"], fx[k + "valid"])
    assert figures["loss"] <= 1 and figures["stats"] <= 1 and figures["d_di_elem"] <= 1
    assert figures["d_di"] <= R.GRAD_BOUND and figures["d_T"] <= R.GRAD_BOUND
    no_farther(got["loss"], fx[k + "loss"], want["loss"], spacing(want["loss"]), "loss")
    no_farther(got["stats"], fx[k + "stats"], want["stats"], 2 * spacing(want["stats"]), "stats")
    no_farther(got["d_di"], fx[k + "d_di"], want["d_di"], R.GRAD_BOUND * l2(want["d_di"]), "d_di")
    no_farther(got["d_T"], fx[k + "d_T"], want["d_T"], R.GRAD_BOUND * l2(want["d_T"]), "d_T")


@pytest.mark.parametrize("n,fine,case", PAIR_IDS)
def test_pair_against_the_referee_and_the_reference(fx, wants, n, fine, case):
    inp, opts = R.pair_case(fx, n, fine, case)
    want, got, k = wants[(n, fine, case)], run_pair(inp, opts), f"p{n}_f{fine}_{case}_"
    tensors = PAIR_DEPTHS[:4 if fine else 2] + ("Ps", "Po")
    assert got["d_Ps"].shape == (4, 4) and not got["d_Ps"][3].any() and not got["d_Po"][3].any()      # [4,4] poses: a constant bottom row
    got["d_Ps"], got["d_Po"] = got["d_Ps"][:3], got["d_Po"][:3]
    figures = dict(loss=R.fwd_excess(got["loss"], want["loss"]), stats=R.fwd_excess(got["stats"], want["stats"]))
    figures.update({"d_" + s: R.rel_l2(got["d_" + s], want["d_" + s]) for s in tensors})
    figures.update({"d_" + s + "_elem": R.fwd_excess(got["d_" + s], want["d_" + s]) for s in tensors[:-2]})
    print(figures)
    assert figures["loss"] <= 1 and figures["stats"] <= 1
    for s in tensors:
        assert figures["d_" + s] <= R.GRAD_BOUND, s
    for s in tensors[:-2]:
        assert figures["d_" + s + "_elem"] <= 1, s
    no_farther(got["loss"], fx[k + "loss"], want["loss"], spacing(want["loss"]), "loss")
    no_farther(got["stats"], fx[k + "stats"], want["stats"], 3 * spacing(want["stats"]), "stats")
    for s in tensors:
        ref = fx[k + "d_" + s][:3] if s in ("Ps", "Po") else fx[k + "d_" + s]
        no_farther(got["d_" + s], ref, want["d_" + s], R.GRAD_BOUND * l2(want["d_" + s]), "d_" + s)
    # [3,4] poses: the same bits, gradients of that shape
    got34 = run_pair(inp, opts, poses34=True)
    assert got34["d_Ps"].shape == (3, 4) and all(np.array_equal(got34[key], got[key]) for key in got)


@pytest.mark.parametrize("n", [1025, 4097])
def test_two_calls_give_the_same_bits(fx, n):
    inp, opts = R.term_case(fx, n, "huber_checks")
    a, b = run_term(inp, opts), run_term(inp, opts)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    if n in R.PAIR_NS:
        inp, opts = R.pair_case(fx, n, 1, "huber_checks")
        a, b = run_pair(inp, opts), run_pair(inp, opts)
        assert all(np.array_equal(a[k], b[k]) for k in a)


def test_input_forms_give_the_bits_of_the_dense_call(fx):
    """integer pixel grids, [n,1] depths, [n] weights and strided views of larger tensors"""
    n = 257
    inp, opts = R.term_case(fx, n, "huber_checks")
    dense = run_term(inp, opts)

    def strided(a, cols):
        big = torch.full((n, 2 * cols + 1), 7.0, device=dev())
        big[:, ::2][:, :cols] = D(a).reshape(n, cols)
        return big[:, ::2][:, :cols]

    di = strided(inp["di"], 1).requires_grad_()                   # [n,1], stride (3, 2)
    Tt = D(np.ascontiguousarray(inp["T"].T)).T.requires_grad_()   # a transposed view
    assert not di.is_contiguous() and not Tt.is_contiguous()
    loss, stats, valid = losses.reprojection_loss(D(inp["pi"]).long(), di, D(inp["Ki"]), strided(inp["pj"], 2), strided(inp["dj"], 1), D(inp["Kj"]), Tt,
                                                  strided(inp["w"], 1)[:, 0], return_valid_mask=True, **opts)
    d_di, d_T = torch.autograd.grad(loss, (di, Tt))
    assert d_di.shape == (n, 1) and d_T.shape == (4, 4)
    assert np.array_equal(loss.detach().cpu().numpy(), dense["loss"]) and np.array_equal(valid.cpu().numpy()[:, 0], dense["valid"])
    assert np.array_equal(d_di.cpu().numpy()[:, 0], dense["d_di"]) and np.array_equal(d_T.cpu().numpy(), dense["d_T"])
    assert stats["perc_val_pix_rep"].item() == dense["stats"][0] and stats["perc_val_depth_rep"].item() == dense["stats"][1]


def test_no_matches():
    e = lambda *s: torch.zeros(*s, device=dev())
    K, P = torch.eye(3, device=dev()), torch.eye(4, device=dev())[:3].clone().requires_grad_()
    d = e(0).requires_grad_()
    loss, stats = losses.correspondence_pair_loss(e(0, 2), e(0, 2), d, e(0), K, K, P, P.detach(), None, pixel_thresh=10.0, depth_thresh=0.1)
    assert type(loss.grad_fn).__name__.startswith("ReprojPairLoss")
    assert loss.item() == 0.0 and all(s.item() == 0.0 for s in stats.values()) and len(stats) == 3
    loss.backward()
    assert d.grad.shape == (0,) and P.grad.shape == (3, 4) and not P.grad.any()
    Tt = torch.eye(4, device=dev()).requires_grad_()
    loss, stats, valid = losses.reprojection_loss(e(0, 2), e(0), K, e(0, 2), None, K, Tt, None, pixel_thresh=10.0, return_valid_mask=True)
    loss.backward()
    assert loss.item() == 0.0 and stats["perc_val_pix_rep"].item() == 0.0 and valid.shape == (0, 1) and not Tt.grad.any()


def test_replacement_method_fills_stats_dict(fx, wants):
    class Theirs:
        def compute_render_and_repro_loss_w_repro_thres(self, *a, **k):
            raise AssertionError("not replaced")

    mod = types.SimpleNamespace(CorrespondencesPairRenderDepthAndGet3DPtsAndReproject=Theirs)
    opt = types.SimpleNamespace(diff_loss_type="huber", renderrepro_do_pixel_reprojection_check=True, renderrepro_do_depth_reprojection_check=True,
                                renderrepro_pixel_reprojection_thresh=R.PIX_THRESH, renderrepro_depth_reprojection_thresh=R.DEPTH_THRESH)
    n = 257
    inp, opts = R.term_case(fx, n, "huber_checks")
    dense = run_term(inp, opts)
    args = [D(inp["pi"]).long(), D(inp["di"], True), D(inp["Ki"]), D(inp["pj"]), D(inp["dj"]), D(inp["Kj"]), D(inp["T"]), D(inp["w"])[:, None]]
    losses.install(mod)
    try:
        stats = {"kept": 1}
        loss, out, valid = Theirs().compute_render_and_repro_loss_w_repro_thres(opt, *args, stats, return_valid_mask=True)
        assert out is stats and set(stats) == {"kept", "perc_val_pix_rep", "perc_val_depth_rep"}
        assert valid.dtype == torch.bool and valid.shape == (n, 1) and np.array_equal(valid.cpu().numpy()[:, 0], dense["valid"])
        assert np.array_equal(loss.detach().cpu().numpy(), dense["loss"]) and stats["perc_val_depth_rep"].item() == dense["stats"][1]
        assert stats["perc_val_pix_rep"].dim() == 0 and stats["perc_val_pix_rep"].device.type == "cuda"
        loss.backward()
        assert np.array_equal(args[1].grad.cpu().numpy(), dense["d_di"])
        assert len(Theirs().compute_render_and_repro_loss_w_repro_thres(opt, *args, {})) == 2
    finally:
        losses.uninstall()


@pytest.mark.parametrize("n", [1025, 4097])
def test_graph_replays_give_the_eager_bits(fx, n):
    """one term above and one below the one-workgroup limit (the workspace is allocated inside the capture), the pair with fine depths;
    forward and seeds"""
    inp, opts = R.term_case(fx, n, "huber_checks")
    t = {k: D(v) for k, v in inp.items()}
    t["di"].requires_grad_()
    pinp, popts = R.pair_case(fx, 1025, 1, "huber_checks")
    p = {k: D(v) for k, v in pinp.items()}
    p["ds"].requires_grad_(), p["Po"].requires_grad_()

    def step():
        loss, _ = losses.reprojection_loss(t["pi"], t["di"], t["Ki"], t["pj"], t["dj"], t["Kj"], t["T"], t["w"], **opts)
        ploss, _ = losses.correspondence_pair_loss(p["ps"], p["po"], p["ds"], p["do"], p["Ks"], p["Ko"], p["Ps"], p["Po"], p["w"], p["fs"], p["fo"],
                                                   **popts)
        return (loss, ploss) + torch.autograd.grad(loss + ploss, (t["di"], p["ds"], p["Po"]))

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


def test_pair_loss_behind_two_pixel_list_renders():
    """The renderer's smallest shapes, two deferred pixel-list renders of 65 rays with poses that need a gradient, the pair loss on their
    depths, backward: every gradient finite, and the parameter gradients EQUAL to those from feeding the loss's own depth seeds into a
    second, identical render's backward -- the plumbing adds nothing of its own."""
    from sparf_amd.edict import EasyDict as edict
    from sparf_amd.renderer import Graph, PendingRender
    from tests.golden.recipe import small_opt
    H, W, n = 40, 60, 65
    gen = torch.Generator().manual_seed(11)
    ps = torch.stack([torch.randint(0, W, (n,), generator=gen), torch.randint(0, H, (n,), generator=gen)], 1).to(dev())
    po = (ps.float() + torch.randn(n, 2, generator=gen).to(dev()) * 2).clamp_min(0)
    conf = torch.rand(n, 1, generator=gen).to(dev())
    intr = torch.tensor([[50.0, 0, W / 2], [0, 50.0, H / 2], [0, 0, 1]], device=dev())

    def run(through_seeds):
        opt = small_opt(hip=dict(lazy_batch=True))
        torch.manual_seed(0)
        g = Graph(opt, dev())
        g.train()
        poses = torch.tensor([[[1.0, 0, 0, 0.1], [0, 1, 0, 0], [0, 0, 1, 3.0]], [[1.0, 0, 0, -0.2], [0, 1, 0, 0.05], [0, 0, 1, 3.1]]],
                             device=dev()).requires_grad_(True)
        data = edict(depth_range=torch.tensor([[1.5, 4.5]] * 2, device=dev()))
        torch.manual_seed(3)
        a = g.render_image_at_specific_pose_and_rays(opt, data, poses[0], intr, H, W, iter=10, pixels=ps, mode="train")
        b = g.render_image_at_specific_pose_and_rays(opt, data, poses[1], intr, H, W, iter=10, pixels=po, mode="train")
        assert isinstance(a, PendingRender) and g.lazy_stats == dict(batches=0, requests=0)
        depths = [a.depth, b.depth, a.depth_fine, b.depth_fine]          # the first read launches the batch
        assert g.lazy_stats == dict(batches=1, requests=2) and depths[0].shape == (1, n, 1)
        loss, stats = losses.correspondence_pair_loss(ps, po, depths[0], depths[1], intr, intr, poses[0], poses[1], conf, depths[2], depths[3],
                                                      pixel_thresh=30.0)
        assert type(loss.grad_fn).__name__.startswith("ReprojPairLoss") and set(stats) == {"depth_in_corr_loss", "perc_val_pix_rep"}
        if through_seeds:
            torch.autograd.backward(depths, torch.autograd.grad(loss, depths))
        else:
            loss.backward()
        return loss.detach(), poses.grad, {k: v.grad for k, v in g.named_parameters() if not k.endswith("progress")}

    loss, d_pose, d_params = run(False)
    assert torch.isfinite(loss) and float(loss) > 0 and torch.isfinite(d_pose).all() and float(d_pose.abs().max()) > 0
    assert d_params and all(v is not None and torch.isfinite(v).all() for v in d_params.values()) and any(float(v.abs().max()) > 0 for v in d_params.values())
    loss2, _, d_params2 = run(True)
    assert torch.equal(loss, loss2)
    for k, v in d_params.items():
        assert torch.equal(v, d_params2[k]), k
