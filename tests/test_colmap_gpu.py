"""The DS-NeRF sparse depth loss on the device: the compact and gather kernels against the numpy referee
(tests/colmap_referee.py) bit for bit on the three shapes; the loss kernel and both seeds against the float64 referee, within one fp32
spacing of the rounded float64 value (double arithmetic, rounded once: only a rounding tie can differ); the same bits from call to
call; and the installed method on a real Graph against the package's own restatement of the reference's loop."""
import types

import numpy as np
import pytest
import torch

from sparf_amd import losses, ops
from sparf_amd.config import default_opt
from sparf_amd.edict import EasyDict as edict
from tests import colmap_referee as R

pytestmark = pytest.mark.gpu
IDS = [R.case_name(*s) for s in R.SHAPES]


def dev():
    return torch.device("cuda:0")


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def same_bits(got, want, what):
    got, want = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_compact_and_gather_against_the_referee(shape):
    H, W = shape
    depth, conf = R.maps_of(H, W)
    g = np.random.RandomState(W)
    valid = R.select_np(depth, conf, R.RAND_RAYS, [np.arange(H * W)] * R.B)["valid"]
    perms = [g.permutation(v) for v in valid]
    want = R.select_np(depth, conf, R.RAND_RAYS, perms)
    d, c = D(depth), D(conf)
    index, count = ops.colmap_compact(d)
    same_bits(count, np.array(want["valid"] + want["positive"], dtype=np.int32), "counts")
    for b in range(R.B):
        same_bits(index[b, :valid[b]], np.nonzero(depth[b].reshape(-1) > np.float32(1e-6))[0].astype(np.int32), f"index of image {b}")
    rays, target, weight, counts, perc = losses.sparse_depth_select(d, c, R.RAND_RAYS, perms=[D(p) for p in perms])
    assert counts.device is not None and (counts.valid, counts.positive, counts.rows) == (want["valid"], want["positive"], want["rows"])
    assert perc == want["perc"] and isinstance(perc, float)
    for b in range(R.B):
        same_bits(rays[b], want["rays"][b], f"rays of image {b}")
    same_bits(target, want["target"], "target")
    same_bits(weight, want["weight"], "weight")
    if shape == (65, 67):
        assert tuple(want["valid"]) == R.VALID_65x67 and tuple(want["positive"]) == R.POSITIVE_65x67 and perc == R.PERC_65x67
        # the permutation the function draws itself is torch.randperm(count, device=...) of the device's generator, for image 0 only
        torch.manual_seed(4)
        drawn = losses.sparse_depth_select(d, c, R.RAND_RAYS)
        torch.manual_seed(4)
        ref = R.select_np(depth, conf, R.RAND_RAYS, [torch.randperm(valid[0], device=dev()).cpu().numpy()] * R.B)
        for b in range(R.B):
            same_bits(drawn[0][b], ref["rays"][b], f"drawn rays of image {b}")


def _loss_case(rows, fine, seed, split):
    """random rows -> (target, weight, depths, fines as device tensors that require grad, the float64 referee's loss and seeds)"""
    g = np.random.RandomState(seed)
    K = sum(rows)
    t, w = (1.5 + 2 * g.rand(K)).astype(np.float32), (0.25 + 0.5 * g.rand(K)).astype(np.float32)
    p, pf = (t + 0.3 * g.randn(K)).astype(np.float32), (t + 0.2 * g.randn(K)).astype(np.float32)
    kept = [k for k in rows if k]
    if split:                                             # adjacent views of one buffer: read in place
        make = lambda a: list(torch.split(D(a).requires_grad_(), kept))
    else:
        make = lambda a: [x.clone().reshape(1, -1, 1).requires_grad_() for x in torch.split(D(a), kept)]
    return D(t), D(w), make(p), make(pf) if fine else None, R.loss_np(t, w, rows, p, pf if fine else None, len(rows))


@pytest.mark.parametrize("rows,split", [([32, 32, 0, 2], False), ([1500, 1499, 1101], False), ([40, 0, 25], True), ([7], True)],
                         ids=["issue-case", "above-4096", "empty-between", "one-image"])
@pytest.mark.parametrize("fine", [True, False], ids=["fine", "coarse"])
def test_loss_and_seeds_against_float64(rows, split, fine):
    t, w, p, pf, (ref, seed, seed_fine) = _loss_case(rows, fine, 7 + len(rows), split)
    loss = losses.sparse_depth_loss(t, w, rows, p, pf)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert R.within_spacings(loss.detach().cpu().numpy(), ref, 1), (float(loss), ref)
    if split:
        leaves = [p[0]._base] + ([pf[0]._base] if fine else [])
    else:
        leaves = p + (pf or [])
    grads = torch.autograd.grad(loss, leaves)
    cat = lambda ts: np.concatenate([x.reshape(-1).cpu().numpy() for x in ts])
    n = 1 if split else len(p)
    assert R.within_spacings(cat(grads[:n]), seed, 1)
    if fine:
        assert R.within_spacings(cat(grads[n:]), seed_fine, 1)
    # two calls give the same bits
    again = losses.sparse_depth_loss(t, w, rows, p, pf)
    assert torch.equal(again, loss)
    for a, b in zip(torch.autograd.grad(again, leaves), grads):
        assert torch.equal(a, b)
    # and the counts of a selection cut by the quota mark the same boundaries as the rows themselves
    count = torch.tensor([k + 5 if k == max(rows) else k for k in rows] + [0] * len(rows), dtype=torch.int32, device=dev())
    counts = losses.SparseCounts(count.tolist()[:len(rows)], [0] * len(rows), rows, max(rows), count)
    assert torch.equal(losses.sparse_depth_loss(t, w, counts, p, pf), loss)


def _setup(lazy, precision, seed=0):
    from sparf_amd.renderer import Graph
    H, W = 65, 67
    opt = default_opt(nerf=dict(sample_intvs=32, sample_intvs_fine=32, fine_sampling=True, rand_rays=R.RAND_RAYS), barf_c2f=[0.1, 0.5],
                      hip=dict(precision=precision, lazy_batch=lazy))
    torch.manual_seed(seed)
    g = Graph(opt, dev())
    g.train()
    g.nerf.progress.data.fill_(0.4)
    g.nerf_fine.progress.data.fill_(0.4)
    pose = torch.eye(4, device=dev())[:3].repeat(R.B, 1, 1)
    pose[:, 0, 3] = torch.tensor([0.1, -0.2, 0.0, 0.15], device=dev())
    pose[:, 2, 3] = 3.0
    intr = torch.tensor([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1]], device=dev()).repeat(R.B, 1, 1)
    depth, conf = R.maps_of(H, W)
    data = edict(image=torch.zeros(R.B, 3, H, W, device=dev()), intr=intr, pose=pose, idx=torch.arange(R.B, device=dev()),
                 depth_range=torch.tensor([[1.5, 4.5]] * R.B, device=dev()), colmap_depth=D(depth), colmap_conf=D(conf))
    obj = types.SimpleNamespace(net=g, device=dev(), opt=opt)
    log = []
    real = g.render_image_at_specific_pose_and_rays

    def render(*a, **k):
        ret = real(*a, **k)
        log.append((k["ray_idx"].clone(), ret))
        return ret

    g.render_image_at_specific_pose_and_rays = render
    return obj, data, log


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_installed_method_on_a_graph_against_the_loop(precision):
    from sparf_amd.renderer import PendingRender
    obj0, data0, log0 = _setup(False, precision)
    torch.manual_seed(3)
    with losses.unfused():                                # the package's restatement of the reference's loop: eager, separate renders
        loss0, stats0, _ = losses.compute_colmap_depth_loss(obj0, obj0.opt, data0, {}, 10, mode="train")
    state0 = (torch.get_rng_state(), torch.cuda.get_rng_state(dev()))
    loss0["colmap_depth"].backward()

    obj1, data1, log1 = _setup(True, precision)
    torch.manual_seed(3)
    loss1, stats1, plots1 = losses.compute_colmap_depth_loss(obj1, obj1.opt, data1, {}, 10, mode="train")
    state1 = (torch.get_rng_state(), torch.cuda.get_rng_state(dev()))
    loss1["colmap_depth"].backward()

    assert stats1 == stats0 == {"perc_col_depth": R.PERC_65x67} and plots1 == {} and sorted(loss1) == ["colmap_depth"]
    assert [len(r) for r, _ in log0] == [len(r) for r, _ in log1] == [32, 32, 2]
    assert all(not isinstance(ret, PendingRender) for _, ret in log0) and all(isinstance(ret, PendingRender) for _, ret in log1)
    assert obj1.net.lazy_stats == dict(batches=1, requests=3) and obj0.net.lazy_stats == dict(batches=0, requests=0)
    for (r0, ret0), (r1, ret1) in zip(log0, log1):
        assert torch.equal(r0, r1)
        for k in ("depth", "depth_fine"):
            assert torch.equal(ret0[k], ret1[k]), k
    assert torch.equal(state0[0], state1[0]) and torch.equal(state0[1], state1[1])
    a, b = float(loss1["colmap_depth"].detach()), float(loss0["colmap_depth"].detach())
    print("loss installed", a, "loop", b)
    assert R.within_spacings(a, b, 2), (a, b)
    for (n0, p0), (n1, p1) in zip(obj0.net.named_parameters(), obj1.net.named_parameters()):
        if n0.endswith("progress"):
            continue
        if p0.grad is None:
            assert p1.grad is None, n0
            continue
        rel = float((p1.grad - p0.grad).norm() / (p0.grad.norm() + 1e-30))
        print(n0, rel)
        assert rel <= (2e-5 if precision == "fp32" else 2e-3), (n0, rel)
