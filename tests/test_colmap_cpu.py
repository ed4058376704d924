"""The DS-NeRF sparse depth loss without a GPU: the torch restatement of sparf_amd.losses against the fixture
(tests/golden/colmap.npz: what the reference's own method did under no_grad) and the numpy referee (tests/colmap_referee.py); the
argument checks of the C-ABI entry points; what the glue hands the library, over a stand-in that records calls (tests/colmap_fake.py);
the early returns; install_colmap_depth() / uninstall_colmap_depth(); and, where the reference tree is present, its unmodified method
before and after the installation, from the same seed."""
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
from sparf_amd.edict import EasyDict as edict
from tests import colmap_fake, colmap_referee as R, ref_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [R.case_name(*s) for s in R.SHAPES]


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def T(a):
    return torch.from_numpy(np.array(a))


def maps(H, W):
    depth, conf = R.maps_of(H, W)
    return T(depth), T(conf)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), what


def module(H, W, fine=True, grad=False, **data):
    net = colmap_fake.DepthNet(R.B, fine=fine, grad=grad)
    obj = types.SimpleNamespace(net=net, device=torch.device("cpu"), opt=edict(nerf=edict(rand_rays=R.RAND_RAYS)))
    depth, conf = maps(H, W)
    d = edict(dict(dict(image=torch.zeros(R.B, 3, H, W), intr=torch.eye(3).repeat(R.B, 1, 1), colmap_depth=depth, colmap_conf=conf), **data))
    return obj, d


def test_the_case_is_the_one_the_issue_states():
    depth, conf = R.maps_of(65, 67)
    sel = R.select_np(depth, conf, R.RAND_RAYS, [np.arange(65 * 67)] * R.B)
    assert tuple(sel["valid"]) == R.VALID_65x67 and tuple(sel["positive"]) == R.POSITIVE_65x67 and sel["rows"] == [32, 32, 0, 2]
    assert sel["perc"] == R.PERC_65x67 == 0.21021814006888634 and R.QUOTA == 32
    assert sel["rays"][3].tolist() == [0, 65 * 67 - 1] and depth.dtype == np.float32


@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_restatement_reproduces_the_fixture(fx, shape, seed):
    """ray lists and perc_col_depth bit for bit, the generator left as the reference leaves it, the loss within 2 fp32 spacings (the
    reference adds fp32 means; the order of the adds may differ)"""
    H, W = shape
    key = f"{R.case_name(H, W)}/{seed}/"
    depth, conf = maps(H, W)
    torch.manual_seed(seed)
    rays, target, weight, counts, perc = losses.sparse_depth_select_torch(depth, conf, R.RAND_RAYS)
    same_bits(torch.get_rng_state().numpy(), fx[key + "rng"], "generator state")
    rendered = [b for b in range(R.B) if counts.rows[b]]
    assert rendered == fx[key + "rendered"].tolist() and isinstance(perc, float)
    same_bits(np.float64(perc), fx[key + "perc"], "perc")
    for b in range(R.B):
        if b in rendered:
            same_bits(rays[b].numpy(), fx[key + f"rays_{b}"], f"rays of image {b}")
        else:
            assert rays[b].numel() == 0 and rays[b].dtype == torch.int64
    depths = [T(R.rendered_np(b, rays[b].numpy()))[None, :, None] for b in rendered]
    fines = [T(R.rendered_np(b, rays[b].numpy(), fine=True))[None, :, None] for b in rendered]
    loss = losses.sparse_depth_loss_torch(target, weight, counts, depths, fines, R.B)
    assert loss.dtype == torch.float32 and R.within_spacings(loss.numpy(), fx[key + "loss"], 2), (float(loss), float(fx[key + "loss"]))
    assert losses.sparse_depth_select(depth, conf, R.RAND_RAYS)[3].device is None          # CPU tensors: the restatement, no library


@pytest.mark.parametrize("fine", [True, False])
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_restatement_against_the_referee(shape, fine):
    """selection bit for bit; loss within 2 fp32 spacings of the float64 value (fp32 means of at most 32 products); autograd against the
    closed-form seeds at rtol 1e-6 (fp32 products of three factors)"""
    H, W = shape
    depth, conf = R.maps_of(H, W)
    g = np.random.RandomState(H)
    perms = [g.permutation(v) for v in R.select_np(depth, conf, R.RAND_RAYS, [np.arange(H * W)] * R.B)["valid"]]
    want = R.select_np(depth, conf, R.RAND_RAYS, perms)
    state = torch.get_rng_state()
    rays, target, weight, counts, perc = losses.sparse_depth_select(T(depth), T(conf), R.RAND_RAYS, perms=[T(p) for p in perms])
    assert torch.equal(torch.get_rng_state(), state)                 # every permutation was supplied: nothing drawn
    assert (counts.valid, counts.positive, counts.rows, counts.quota) == (want["valid"], want["positive"], want["rows"], R.QUOTA)
    assert perc == want["perc"]
    for b in range(R.B):
        same_bits(rays[b].numpy(), want["rays"][b], f"rays of image {b}")
    same_bits(target.numpy(), want["target"], "target")
    same_bits(weight.numpy(), want["weight"], "weight")
    kept = [b for b in range(R.B) if want["rows"][b]]
    p = [T(R.rendered_np(b, want["rays"][b]) * np.float32(1.03)).requires_grad_() for b in kept]
    pf = [T(R.rendered_np(b, want["rays"][b], fine=True)).requires_grad_() for b in kept] if fine else None
    loss = losses.sparse_depth_loss(target, weight, counts, p, pf, batch_size=R.B)
    cat = lambda ts: np.concatenate([t.detach().numpy() for t in ts])
    ref, seed, seed_fine = R.loss_np(want["target"], want["weight"], want["rows"], cat(p), cat(pf) if fine else None, R.B)
    assert R.within_spacings(loss.detach().numpy(), ref, 2), (float(loss), ref)
    grads = torch.autograd.grad(loss, p + (pf or []))
    np.testing.assert_allclose(cat(grads[:len(p)]), seed, rtol=1e-6, atol=0)
    if fine:
        np.testing.assert_allclose(cat(grads[len(p):]), seed_fine, rtol=1e-6, atol=0)
    # the rows per image as plain ints serve as well
    assert torch.equal(losses.sparse_depth_loss(target, weight, want["rows"], p, pf), loss)


def test_entry_points_check_their_arguments_without_a_device():
    lib = L.load()
    buf = np.zeros(64, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)         # host memory: never dereferenced, every call below returns before a launch

    def call(name, defaults, **kw):
        assert tuple(defaults) == colmap_fake.COLMAP_CALLS[name] and set(kw) <= set(defaults), name
        return getattr(lib, name)(*dict(defaults, **kw).values(), None)

    compact = lambda **kw: call("sparf_colmap_compact", dict(depth=p, B=2, H=4, W=4, index=p, count=p, workspace=None), **kw)
    gather = lambda **kw: call("sparf_colmap_gather", dict(index=p, count=p, sel=None, B=2, H=4, W=4, quota=3, K=4, depth=p, conf=p, ray_idx=p,
                                                           target=p, weight=p), **kw)
    loss = lambda **kw: call("sparf_colmap_loss", dict(target=p, weight=p, count=p, B=2, quota=3, K=4, depth=p, depth_fine=None, out=p,
                                                       d_depth=None, d_depth_fine=None, workspace=None), **kw)
    assert compact(B=0) == 1 and compact(B=-1) == 1 and compact(H=-1) == 1 and compact(W=-1) == 1 and compact(H=1 << 16, W=1 << 16) == 1
    assert compact(B=1 << 16) == 1
    for name in ("depth", "index", "count"):
        assert compact(**{name: None}) == 1, name
    assert gather(B=0) == 1 and gather(H=-1) == 1 and gather(quota=-1) == 1 and gather(K=-1) == 1 and gather(K=(1 << 30) + 1, quota=1 << 30) == 1
    assert gather(H=1 << 16, W=1 << 16) == 1 and gather(K=7) == 1                   # 7 rows: more than 2 images of quota 3 hold
    for name in ("index", "count", "depth", "conf", "ray_idx", "target", "weight"):
        assert gather(**{name: None}) == 1, name
    assert gather(K=0) == 0 and gather(K=0, index=None, depth=None, ray_idx=None) == 0          # nothing to launch, no pointer looked at
    assert loss(B=0) == 1 and loss(quota=-1) == 1 and loss(K=-1) == 1 and loss(K=(1 << 30) + 1) == 1 and loss(d_depth_fine=p) == 1
    for name in ("target", "weight", "count", "depth", "out"):
        assert loss(**{name: None}) == 1, name
    assert loss(K=0) == 0 and loss(K=0, target=None, out=None) == 0
    wb = lib.sparf_colmap_workspace_bytes
    assert wb(4, 4096, 0) == 0 and wb(4, 4097, 0) == colmap_fake.workspace_bytes(4, 4097, 0) == 64 and wb(0, 0, 4096) == 0
    assert wb(0, 0, 4100) == colmap_fake.workspace_bytes(0, 0, 4100) == 16 and wb(-1, -5, -5) == 0 and wb(3, 65 * 67, 66) == 48


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(losses, "_takes_kernel", lambda values, constants: not losses._unfused)     # CPU tensors down the fused route
    with colmap_fake.installed() as lib:
        yield lib


class Readbacks:
    """counts every .item() and .tolist() of a tensor while it is open"""

    def __enter__(self):
        self.reads, self.real = [], (torch.Tensor.item, torch.Tensor.tolist)
        torch.Tensor.item = lambda t: (self.reads.append(("item", t.dtype, t.numel())), self.real[0](t))[1]
        torch.Tensor.tolist = lambda t: (self.reads.append(("tolist", t.dtype, t.numel())), self.real[1](t))[1]
        return self.reads

    def __exit__(self, *exc):
        torch.Tensor.item, torch.Tensor.tolist = self.real


def test_one_compact_one_readback_one_gather_one_loss(fake):
    H, W = 65, 67
    n = H * W
    obj, data = module(H, W, grad=True)
    torch.manual_seed(5)
    with Readbacks() as reads:
        loss, stats, plots = losses.compute_colmap_depth_loss(obj, obj.opt, data, {}, 3, mode="train")
    assert fake.names() == ["sparf_colmap_compact", "sparf_colmap_gather", "sparf_colmap_loss"]
    assert reads == [("tolist", torch.int32, 2 * R.B)]                # the one readback: the 2 B counts
    assert fake.calls[0][1] == dict(depth=True, B=R.B, H=H, W=W, index=True, count=True, workspace=True)
    assert fake.calls[1][1] == dict(index=True, count=True, sel=True, B=R.B, H=H, W=W, quota=R.QUOTA, K=66, depth=True, conf=True, ray_idx=True,
                                    target=True, weight=True)
    assert fake.calls[2][1] == dict(target=True, weight=True, count=True, B=R.B, quota=R.QUOTA, K=66, depth=True, depth_fine=True, out=True,
                                    d_depth=True, d_depth_fine=True, workspace=False)
    # the maps' own storage is handed over: no copy
    raw = [r for _, r in fake.raw]
    assert raw[0]["depth"] == raw[1]["depth"] == data.colmap_depth.data_ptr() and raw[1]["conf"] == data.colmap_conf.data_ptr()
    assert raw[1]["index"] == raw[0]["index"] and raw[1]["count"] == raw[0]["count"] == raw[2]["count"]
    assert raw[2]["target"] == raw[1]["target"] and raw[2]["weight"] == raw[1]["weight"]
    assert sorted(loss) == ["colmap_depth"] and loss["colmap_depth"].dim() == 0 and loss["colmap_depth"].requires_grad
    assert stats == {"perc_col_depth": R.PERC_65x67} and plots == {}
    # randperm for image 0 only, and the generator left as the reference leaves it; the renders of images 0, 1 and 3 in order
    state = torch.get_rng_state()
    torch.manual_seed(5)
    perm = torch.randperm(R.VALID_65x67[0])
    assert torch.equal(torch.get_rng_state(), state)
    want = R.select_np(*R.maps_of(H, W), R.RAND_RAYS, [perm.numpy()] * R.B)
    assert len(obj.net.calls) == 3
    for got, b in zip(obj.net.calls, (0, 1, 3)):
        same_bits(got.numpy(), want["rays"][b], f"rays of image {b}")
    torch.autograd.grad(loss["colmap_depth"], obj.net.scale)         # carries a gradient to what the renders depend on
    # the public functions: one compact, one gather, one readback; one loss
    fake.calls.clear(), fake.raw.clear()
    with Readbacks() as reads:
        rays, target, weight, counts, perc = losses.sparse_depth_select(data.colmap_depth, data.colmap_conf, R.RAND_RAYS, perms=[perm, None, None, None])
    assert fake.names() == ["sparf_colmap_compact", "sparf_colmap_gather"] and reads == [("tolist", torch.int32, 2 * R.B)]
    assert fake.calls[1][1]["sel"] is True and fake.calls[1][1]["K"] == 66 and perc == R.PERC_65x67
    for b in range(R.B):
        same_bits(rays[b].numpy(), want["rays"][b], f"rays of image {b}")
    same_bits(target.numpy(), want["target"], "target")
    # adjacent views of one buffer are read in place; separate tensors cost one cat
    buf = torch.arange(66, dtype=torch.float32).requires_grad_()
    views = list(torch.split(buf, [32, 32, 2]))
    losses.sparse_depth_loss(target, weight, counts, [v.reshape(1, -1, 1) for v in views])
    assert fake.raw[-1][1]["depth"] == buf.data_ptr() and fake.calls[-1][1]["depth_fine"] is False and fake.calls[-1][1]["d_depth"] is True
    losses.sparse_depth_loss(target, weight, counts, [v.clone() for v in views])
    assert fake.raw[-1][1]["depth"] != buf.data_ptr()
    # explicit rows: the counts are the rows themselves, no quota cuts them
    losses.sparse_depth_loss(target, weight, [32, 32, 0, 2], [v.detach() for v in views])
    assert fake.calls[-1][1]["quota"] == ops.COLMAP_ALL_ROWS and fake.calls[-1][1]["d_depth"] is False
    with pytest.raises(ValueError, match="rendered depths"):
        losses.sparse_depth_loss(target, weight, counts, views[:2])
    # a count exactly at the quota draws nothing; one image above it after one that is not: two gather ranges, no permutation ahead
    fake.calls.clear()
    fake.valid, fake.positive = [32, 40, 0, 5], [32, 40, 0, 5]
    obj, data = module(H, W)
    torch.manual_seed(6)
    losses.compute_colmap_depth_loss(obj, obj.opt, data, {}, 3, mode="train")
    state = torch.get_rng_state()
    torch.manual_seed(6)
    torch.randperm(40)
    assert torch.equal(torch.get_rng_state(), state)
    gathers = [c for name, c in fake.calls if name == "sparf_colmap_gather"]
    assert [(c["B"], c["K"], c["sel"]) for c in gathers] == [(1, 32, False), (3, 37, True)] and [len(c) for c in obj.net.calls] == [32, 32, 5]
    assert n > 4096


def test_nothing_valid_makes_no_gather_and_no_loss_call(fake):
    obj, data = module(16, 16)
    data.colmap_depth = torch.zeros_like(data.colmap_depth)
    data.colmap_depth[3, 0, 0, 0] = 5e-7                             # positive, not valid
    state = torch.get_rng_state()
    loss, stats, plots = losses.compute_colmap_depth_loss(obj, obj.opt, data, {}, 0, mode="train")
    assert fake.names() == ["sparf_colmap_compact"] and obj.net.calls == [] and torch.equal(torch.get_rng_state(), state)
    assert float(loss["colmap_depth"].detach()) == 0.0 and loss["colmap_depth"].requires_grad and stats == {"perc_col_depth": 1 / (R.B * 256)}
    rays, target, weight, counts, perc = losses.sparse_depth_select(data.colmap_depth, data.colmap_conf, R.RAND_RAYS)
    assert fake.names() == ["sparf_colmap_compact"] * 2 and [r.numel() for r in rays] == [0] * R.B and target.numel() == 0 and counts.rows == [0] * R.B
    zero = losses.sparse_depth_loss(target, weight, counts, [])
    assert fake.names() == ["sparf_colmap_compact"] * 2 and float(zero.detach()) == 0.0 and zero.requires_grad


def test_unfused_and_float64_maps_make_no_library_call(fake):
    obj, data = module(16, 16)
    with losses.unfused():
        a = losses.compute_colmap_depth_loss(obj, obj.opt, data, {}, 0, mode="train")
        losses.sparse_depth_select(data.colmap_depth, data.colmap_conf, R.RAND_RAYS)
    obj64, data64 = module(16, 16)
    data64.colmap_depth, data64.colmap_conf = data64.colmap_depth.double(), data64.colmap_conf.double()
    b = losses.compute_colmap_depth_loss(obj64, obj64.opt, data64, {}, 0, mode="train")
    losses.sparse_depth_select(data64.colmap_depth, data64.colmap_conf, R.RAND_RAYS)
    assert fake.calls == []
    assert a[1] == b[1] == {"perc_col_depth": R.select_np(*R.maps_of(16, 16), R.RAND_RAYS, [np.arange(256)] * R.B)["perc"]}
    assert [len(c) for c in obj.net.calls] == [32, 2, 2] and b[0]["colmap_depth"].dtype == torch.float64


def _class():
    class SparseCOLMAPDepthLoss:
        def compute_loss(self, *a, **k):
            return ("theirs", a, k)

    return SparseCOLMAPDepthLoss


def test_install_patches_and_uninstall_restores():
    cls = _class()
    mod = types.SimpleNamespace(SparseCOLMAPDepthLoss=cls, BasePhotoandReguLoss=type("BasePhotoandReguLoss", (), {}))
    theirs = vars(cls)["compute_loss"]
    losses.install_colmap_depth(mod)
    try:
        with pytest.raises(RuntimeError):
            losses.install_colmap_depth(mod)
        losses.install_photometric(mod)                             # independent of the other installs
        losses.uninstall_photometric()
        assert vars(cls)["compute_loss"] is losses.compute_colmap_depth_loss
        obj, data = module(65, 67, grad=True)
        inst = cls()
        inst.net, inst.device, inst.opt = obj.net, obj.device, obj.opt
        for mode in (None, "val", "test-optim"):
            assert inst.compute_loss(inst.opt, data, {}, 0, mode=mode) == ({}, {}, {}) and inst.net.calls == []
        torch.manual_seed(2)
        loss, stats, plots = inst.compute_loss(inst.opt, data, {}, 0, mode="train", plot=False)
        torch.manual_seed(2)
        rays, target, weight, counts, perc = losses.sparse_depth_select_torch(data.colmap_depth, data.colmap_conf, R.RAND_RAYS)
        net = colmap_fake.DepthNet(R.B)
        rets = [net.render_image_at_specific_pose_and_rays(None, None, net.pose[b], None, 65, 67, ray_idx=rays[b], mode="train") for b in (0, 1, 3)]
        by_hand = losses.sparse_depth_loss_torch(target, weight, counts, [r.depth for r in rets], [r.depth_fine for r in rets], R.B)
        assert torch.equal(loss["colmap_depth"].detach(), by_hand) and stats == {"perc_col_depth": perc} and plots == {}
        assert float(torch.autograd.grad(loss["colmap_depth"], inst.net.scale)[0]) != 0.0
    finally:
        losses.uninstall_colmap_depth()
    assert vars(cls)["compute_loss"] is theirs and cls().compute_loss(1)[0] == "theirs"
    losses.install_colmap_depth(mod)                                # and again after an uninstall
    losses.uninstall_colmap_depth()


@pytest.mark.skipif(ref_harness.reference_root() is None, reason="reference tree not present")
def test_reference_method_after_install():
    """The reference's unmodified SparseCOLMAPDepthLoss.compute_loss on CPU tensors under no_grad, constructed by its own __init__ on the
    cases of the fixture: after install_colmap_depth() against before, from the same seed -- identical keys, perc_col_depth, render
    requests and generator state, the loss within 2 fp32 spacings.  In a process of its own: the reference's `source` package must not
    meet dropin/source here."""
    code = """
        import json, numpy as np, torch
        from tests import colmap_referee as R
        from tests.golden import make_colmap_golden as M
        import source.training.core.base_losses as bl
        import sparf_amd.losses as losses
        def run(shape, seed):
            obj, opt, data = M.build_case(*shape)
            torch.manual_seed(seed)
            with torch.no_grad():
                loss, stats, plots = obj.compute_loss(opt, data, {}, 0, mode="train")
            return loss, stats, plots, torch.get_rng_state(), obj.net.calls
        res = {}
        for shape in R.SHAPES:
            before = run(shape, 21)
            losses.install_colmap_depth(bl)
            try:
                after = run(shape, 21)
            finally:
                losses.uninstall_colmap_depth()
            restored = run(shape, 21)
            res[R.case_name(*shape)] = dict(
                keys=sorted(after[0]) == sorted(before[0]) == ["colmap_depth"] and sorted(after[1]) == sorted(before[1]) == ["perc_col_depth"],
                perc=after[1]["perc_col_depth"] == before[1]["perc_col_depth"], plots=after[2] == before[2] == {},
                state=bool(torch.equal(after[3], before[3])),
                renders=len(after[4]) == len(before[4]) and all(torch.equal(a, b) for a, b in zip(after[4], before[4])),
                loss=R.within_spacings(after[0]["colmap_depth"].numpy(), before[0]["colmap_depth"].numpy(), 2),
                restored=bool(torch.equal(restored[0]["colmap_depth"], before[0]["colmap_depth"])), nrender=len(after[4]))
        print(json.dumps(res))
    """
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "compat")])
    p = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(res) == set(IDS)
    for name, r in res.items():
        assert all(r[k] for k in ("keys", "perc", "plots", "state", "renders", "loss", "restored")) and r["nrender"] == 3, (name, r)
