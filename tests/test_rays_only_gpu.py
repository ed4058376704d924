"""Ray-gradient-only passes (C ABI 7, SPARF_SAVE_MASKS) on the GPU: the route performs the arithmetic of the training pass in the same
order and leaves out what only the weight gradient needs, so EVERY comparison here is torch.equal against the existing full route on
the same inputs -- outputs, mask words, ray gradients, pose gradients, an Adam trajectory.  The oracle bounds of the full route
(tests/test_hip_gpu.py, tests/test_graph_gpu.py) carry over through that equality.

Shapes: the project's smallest ragged ones (tests/test_hip_gpu.py): 70 rays x 24 samples = 1 680 rows, neither a multiple of 128 nor of
256; 515 x 64 = 32 960 rows, a partial last round of either tile size."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from sparf_amd import lib as L
from sparf_amd import ops
from sparf_amd.renderer import Graph
from tests.golden.recipe import make_state_dict, ring_cameras, small_opt
from tests.test_hip_gpu import dev, make_scene, params_list

pytestmark = pytest.mark.gpu

M = L.SAVE_MASKS
MASK_TILE = 9 * 1024
FILL = 0x55
SHAPES = [(70, 24), (515, 64)]
PRECS = [("fp32", L.PREC_FP32), ("bf16", L.PREC_BF16), ("bf16x3", L.PREC_X3)]
NOISE_SCALE = 0.5


def _bytes(x):
    return x.detach().contiguous().view(torch.uint8)


def _same(a, b):
    return torch.equal(_bytes(a), _bytes(b))


def _scene(prec, R, N, inverse=False):
    """one pass worth of inputs on the device: barf_c2f on (progress inside the ramp), density noise on"""
    d = dev()
    opt = small_opt(barf_c2f=[0.4, 0.7], nerf=dict(depth=dict(param="inverse", range=[1, 0])) if inverse else {})
    sd = make_state_dict(opt, 21, progress=0.55)
    center, dirs, jitter, noise = make_scene(R, N, 6)
    t = O.sample_depth(opt, 1, R, N, [1, 0] if inverse else [1.2, 5.2], "train", jitter)[0, :, :, 0].to(d).contiguous()
    plist = params_list(sd, d)
    return dict(opt=opt, sd=sd, c=center.to(d).contiguous(), dr=dirs.to(d).contiguous(), t=t, nz=noise[0].to(d).contiguous(), plist=plist,
                packed=ops.pack_weights(plist, prec), c2f=ops.c2f_weights(sd["progress"].to(d), opt.barf_c2f, d))


def _nine_grads(R, N, seed=3):
    """an upstream gradient for each of the nine outputs of a pass (ops.PASS_KEYS order)"""
    g = torch.Generator().manual_seed(seed)
    shapes = [(R, 3), (R,), (R,), (R, N), (R,), (R,), (R,), (R, N), (R, N, 3)]
    return tuple((torch.rand(*s, generator=g) - 0.5).to(dev()) for s in shapes)


def _forward(prec, s, fill=True):
    lib = L.load()
    fa, out, save, keep = ops.build_pass_fwd(prec, s["c"], s["dr"], s["t"], s["nz"], NOISE_SCALE, False, s["packed"], s["c2f"], True)
    if fill:
        save.fill_(FILL)
    L.check(lib.sparf_pass_forward(ctypes.byref(fa), L.stream_ptr(dev())), "fwd")
    torch.cuda.synchronize()
    return fa, out, save, keep


@pytest.mark.parametrize("R,N", SHAPES)
@pytest.mark.parametrize("name,prec", PRECS, ids=[p[0] for p in PRECS])
def test_pass_through_the_c_abi_equals_the_training_pass(name, prec, R, N):
    lib = L.load()
    st = L.stream_ptr(dev())
    s = _scene(prec, R, N)
    fa_f, out_f, save_f, k1 = _forward(prec, s)
    fa_m, out_m, save_m, k2 = _forward(prec | M, s)
    for k in out_f:
        assert _same(out_f[k], out_m[k]), k
    # the masks-only save area = the mask KiB of every tile block of the full save area
    ntiles = (R * N + 255) // 256 * 8
    assert save_m.numel() == ntiles * MASK_TILE and save_f.numel() % ntiles == 0
    full_masks = save_f.view(ntiles, -1)[:, -MASK_TILE:]
    assert torch.equal(save_m.view(ntiles, MASK_TILE), full_masks)
    assert int((save_m != FILL).sum()) > save_m.numel() // 8                       # (the comparison is of real content)

    grads = _nine_grads(R, N)
    args = (s["c"], s["dr"], s["t"], s["nz"], NOISE_SCALE, False, s["packed"], s["c2f"])
    ba_f, gp_f, dc_f, dd_f, k3 = ops.build_pass_bwd(prec, *args, save_f, out_f, grads, True)
    ba_m, gp_m, dc_m, dd_m, k4 = ops.build_pass_bwd(prec | M, *args, save_m, out_m, grads, True)
    assert gp_m is None and ba_m.grad_params is None and k4[0].numel() < k3[0].numel()
    for x in (dc_f, dd_f, dc_m, dd_m):
        x.fill_(float("nan"))
    L.check(lib.sparf_pass_backward(ctypes.byref(ba_f), st), "bwd")
    L.check(lib.sparf_pass_backward(ctypes.byref(ba_m), st), "bwd masks")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dc_f).all()) and float(dc_f.abs().max()) > 0 and float(dd_f.abs().max()) > 0
    assert _same(dc_f, dc_m) and _same(dd_f, dd_m)
    # accumulate_rays = 1 on pre-filled buffers
    pre = torch.rand(2, R, 3, generator=torch.Generator().manual_seed(9)).to(dev())
    once = (dc_f.clone(), dd_f.clone())
    for ba, dc, dd in ((ba_f, dc_f, dd_f), (ba_m, dc_m, dd_m)):
        dc.copy_(pre[0]); dd.copy_(pre[1])
        ba.accumulate_rays = 1
        L.check(lib.sparf_pass_backward(ctypes.byref(ba), st), "bwd accumulate")
    torch.cuda.synchronize()
    assert _same(dc_f, dc_m) and _same(dd_f, dd_m)
    assert not torch.equal(dc_f, once[0]) and torch.allclose(dc_f, once[0] + pre[0], rtol=1e-5, atol=1e-6)
    # what the flag refuses: no ray gradients; combined with the 8-bit format
    ba_m.d_center, ba_m.d_dir = None, None
    assert lib.sparf_pass_backward(ctypes.byref(ba_m), st) != 0
    fa_m.prec = prec | M | L.SAVE_Q8
    assert lib.sparf_pass_forward(ctypes.byref(fa_m), st) != 0
    # an empty batch is nothing to do
    ba_m.nrays = 0
    ba_m.prec = prec | M
    assert lib.sparf_pass_backward(ctypes.byref(ba_m), st) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("R,N", SHAPES)
def test_single_kernel_launches_of_the_bf16x3_pass(R, N):
    """sparf_launch_kernel with the flag: which = 0 brings back what the pass's forward left, 3 / 4 (the two geometries of the data gradient)
    and 1 (the plan of the pass) what its backward left in d point / d view encoding; 2 has nothing to launch."""
    lib = L.load()
    st = L.stream_ptr(dev())
    prec = L.PREC_X3 | M
    s = _scene(L.PREC_X3, R, N)
    fa, out, save, k1 = _forward(prec, s)
    fwd_bufs = dict(sigma_raw=out["sigma_raw"], rgb_samples=out["rgb_samples"], save=save)
    of_the_pass = {k: x.clone() for k, x in fwd_bufs.items()}
    for x in fwd_bufs.values():
        _bytes(x).fill_(FILL)
    L.check(lib.sparf_launch_kernel(0, ctypes.byref(fa), None, st), "mlp_fwd")
    torch.cuda.synchronize()
    for k, x in fwd_bufs.items():
        assert _same(x, of_the_pass[k]), k

    ba, gp, dc, dd, k2 = ops.build_pass_bwd(prec, s["c"], s["dr"], s["t"], s["nz"], NOISE_SCALE, False, s["packed"], s["c2f"], save, out,
                                            _nine_grads(R, N), True)
    ws = k2[0]
    off = (ctypes.c_int64 * 8)()                          # {gradient area, d_sigma, d_z, d_len, partial blocks, dp, dv, total}
    assert lib.sparf_debug_bwd_workspace(prec, R, N, 1, off) == 0 and off[7] == ws.numel()
    assert off[1] == off[0] == 0 and off[5] == off[4]                              # no gradient area, no partial blocks
    ws.fill_(FILL)
    L.check(lib.sparf_pass_backward(ctypes.byref(ba), st), "bwd")
    torch.cuda.synchronize()
    ws_of_the_pass = ws.clone()
    assert int((ws_of_the_pass[off[5]:] != FILL).sum()) > (off[7] - off[5]) // 8
    for which in (3, 4, 1):
        ws[off[5]:].fill_(FILL)                           # d point, d view encoding: what the data gradient writes
        L.check(lib.sparf_launch_kernel(which, ctypes.byref(fa), ctypes.byref(ba), st), "dgrad")
        torch.cuda.synchronize()
        assert torch.equal(ws, ws_of_the_pass), (which, int((ws != ws_of_the_pass).sum()))
    assert lib.sparf_launch_kernel(2, ctypes.byref(fa), ctypes.byref(ba), st) != 0
    torch.cuda.synchronize()


class Recorder:
    """wraps lib.sparf_pass_forward / sparf_pass_backward: (prec, grad_params) of every call"""

    def __init__(self, monkeypatch):
        lib = L.load()
        self.fwd, self.bwd = [], []
        real_f, real_b = lib.sparf_pass_forward, lib.sparf_pass_backward

        def fwd(a, stream):
            self.fwd.append((a._obj.prec, a._obj.nsamp))
            return real_f(a, stream)

        def bwd(a, stream):
            self.bwd.append((a._obj.prec, a._obj.nsamp, a._obj.grad_params))
            return real_b(a, stream)

        monkeypatch.setattr(lib, "sparf_pass_forward", fwd)
        monkeypatch.setattr(lib, "sparf_pass_backward", bwd)

    def clear(self):
        self.fwd, self.bwd = [], []


def _pass_autograd(prec, s, frozen, far=None, segs=None, loss_of=None):
    """one ops.nerf_pass / nerf_pass_segments under autograd with rays that require a gradient; frozen: no parameter does"""
    plist = [p.clone().requires_grad_(not frozen) for p in s["plist"]]
    cg, dg = s["c"].clone().requires_grad_(True), s["dr"].clone().requires_grad_(True)
    farg = (far[0], far[1], ops.pack_weights(plist, far[1])) if far is not None else None
    if segs is None:
        out = ops.nerf_pass(cg, dg, s["t"], s["nz"], NOISE_SCALE, False, prec, s["packed"], s["c2f"], plist, far=farg)
        outs = [out]
    else:
        outs = ops.nerf_pass_segments(cg, dg, s["t"], s["nz"], False, prec, s["packed"], s["c2f"], plist, segs, far=farg)
    loss_of(outs).backward()
    torch.cuda.synchronize()
    return outs, cg.grad, dg.grad, plist


@pytest.mark.parametrize("R,N,R1", [(70, 24, 20), (515, 64, 100)])
@pytest.mark.parametrize("name,prec", PRECS, ids=[p[0] for p in PRECS])
def test_two_segments_the_first_without_upstream_gradient(monkeypatch, name, prec, R, N, R1):
    s = _scene(prec, R, N)
    segs = [(0, R1, 0.0), (R1, R - R1, NOISE_SCALE)]
    w = _nine_grads(R - R1, N, seed=5)
    loss_of = lambda outs: sum((outs[1][k] * g).sum() for k, g in zip(ops.PASS_KEYS, w))
    rec = Recorder(monkeypatch)
    full = _pass_autograd(prec, s, False, segs=segs, loss_of=loss_of)
    assert [p for p, *_ in rec.bwd] == [prec]
    rec.clear()
    rays = _pass_autograd(prec, s, True, segs=segs, loss_of=loss_of)
    assert rec.fwd == [(prec | M, N)] and rec.bwd == [(prec | M, N, None)]
    for a, b in zip(full[0], rays[0]):
        for k in a:
            assert _same(a[k], b[k]), k
    assert _same(full[1], rays[1]) and _same(full[2], rays[2])
    assert float(full[1][R1:].abs().max()) > 0 and float(full[1][:R1].abs().max()) == 0       # the first segment's rays receive zero
    assert all(p.grad is None for p in rays[3]) and all(p.grad is not None for p in full[3])


@pytest.mark.parametrize("R,N", SHAPES)
def test_inverse_depth_bf16x3_pass_with_fp32_far_rows(monkeypatch, R, N):
    prec, far = L.PREC_X3, (8, L.PREC_FP32)
    s = _scene(prec, R, N, inverse=True)
    w = _nine_grads(R, N, seed=7)
    w = tuple(g / float(s["t"].max()) if k in ("depth", "depth_var") else g for k, g in zip(ops.PASS_KEYS, w))
    loss_of = lambda outs: sum((outs[0][k] * g).sum() for k, g in zip(ops.PASS_KEYS, w))
    rec = Recorder(monkeypatch)
    full = _pass_autograd(prec, s, False, far=far, loss_of=loss_of)
    rays = _pass_autograd(prec, s, True, far=far, loss_of=loss_of)
    assert [p for p, *_ in rec.bwd] == [prec, prec | M]
    for k in full[0][0]:
        assert _same(full[0][0][k], rays[0][0][k]), k
    assert float(full[1].abs().max()) > 0
    assert _same(full[1], rays[1]) and _same(full[2], rays[2])
    # far rows take part: without them the same pass gives other ray gradients
    plain = _pass_autograd(prec, s, True, loss_of=loss_of)
    assert not torch.equal(plain[2], rays[2])


# ---------------------------------------------------------------------------------------------- Graph
H, W = 12, 16


def _graph(precision, **over):
    opt = small_opt(barf_c2f=[0.4, 0.7], nerf=dict(sample_intvs=64, sample_intvs_fine=128, rand_rays=H * W, density_noise_reg=True),
                    hip=dict(precision=precision, **over))
    g = Graph(opt, dev())
    g.nerf.load_state_dict(make_state_dict(opt, 31, 0.55))
    g.nerf_fine.load_state_dict(make_state_dict(opt, 32, 0.55))
    return opt, g


_OUT_W = {}


def _loss(ret):
    """a fixed random linear functional of every differentiable output of a render"""
    tot = 0
    for k in sorted(ret.keys()):
        v = ret[k]
        if not (torch.is_tensor(v) and v.requires_grad):
            continue
        key = (k, tuple(v.shape))
        if key not in _OUT_W:
            _OUT_W[key] = (torch.rand(*v.shape, generator=torch.Generator().manual_seed(len(_OUT_W) + 1)) - 0.5).to(dev())
        tot = tot + (v * _OUT_W[key]).sum()
    return tot


def _render_once(graph, opt, mode, seed=11):
    """one Graph.render of the whole 12 x 16 image under a pose that requires a gradient, its backward; the draws (stratified jitter,
    density noise, fine grid) are those of `seed`.  -> (outputs, pose.grad)"""
    pose, intr = ring_cameras(1, H=H, W=W)
    pose = pose.to(dev()).requires_grad_(True)
    torch.manual_seed(seed)
    graph.zero_grad(set_to_none=True)
    ret = graph.render(opt, pose, H=H, W=W, intr=intr.to(dev()), ray_idx=torch.arange(H * W, device=dev()), depth_range=[1.2, 5.2], iter=0, mode=mode)
    _loss(ret).backward()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in ret.items() if torch.is_tensor(v)}, pose.grad.clone()


def _weights(graph):
    """the 40 weight / bias tensors of both networks (not `progress`, which never receives a gradient)"""
    return graph.nerf.hip_params() + graph.nerf_fine.hip_params()


def _param_grads(net):
    return [None if p.grad is None else p.grad.clone() for p in net.hip_params()]


def _assert_same_render(a, b):
    assert set(a[0]) == set(b[0])
    for k in a[0]:
        assert _same(a[0][k], b[0][k]), k
    assert float(a[1].abs().max()) > 0 and _same(a[1], b[1])


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_graph_render_with_frozen_networks(monkeypatch, precision):
    opt, graph = _graph(precision)
    prec = L.PREC_IDS[precision]
    rec = Recorder(monkeypatch)
    full = _render_once(graph, opt, "train")
    assert all(p.grad is not None for p in _weights(graph))
    assert rec.fwd == [(prec, 64), (prec, 192)] and all(p == prec and gp for p, _, gp in rec.bwd) and len(rec.bwd) == 2
    rec.clear()
    graph.requires_grad_(False)
    rays = _render_once(graph, opt, "train")
    _assert_same_render(full, rays)
    assert all(p.grad is None for p in _weights(graph))
    assert rec.fwd == [(prec | M, 64), (prec | M, 192)]
    assert sorted(rec.bwd) == [(prec | M, 64, None), (prec | M, 192, None)]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_mixed_render_coarse_frozen_fine_trainable(monkeypatch, precision):
    opt, graph = _graph(precision)
    prec = L.PREC_IDS[precision]
    full = _render_once(graph, opt, "train")
    fine_full = _param_grads(graph.nerf_fine)
    rec = Recorder(monkeypatch)
    graph.nerf.requires_grad_(False)
    mixed = _render_once(graph, opt, "train")
    _assert_same_render(full, mixed)
    assert all(p.grad is None for p in graph.nerf.hip_params())
    for a, b in zip(fine_full, _param_grads(graph.nerf_fine)):
        assert a is not None and float(a.abs().max()) > 0 and _same(a, b)
    assert rec.fwd == [(prec | M, 64), (prec, 192)]
    assert sorted((p, n, gp is None) for p, n, gp in rec.bwd) == sorted([(prec | M, 64, True), (prec, 192, False)])


@pytest.mark.parametrize("fused", [True, False], ids=["fused_render", "pass_by_pass"])
def test_test_optim_rays_only_option(monkeypatch, fused):
    precision = "bf16x3"
    prec = L.PREC_IDS[precision]
    opt, graph = _graph(precision, fused_render=fused)
    rec = Recorder(monkeypatch)
    default = _render_once(graph, opt, "test-optim")                       # the option at its default: .grad populated, as today
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in _weights(graph))
    assert all(p == prec for p, _ in rec.fwd) and len(rec.fwd) == 2
    rec.clear()
    opt.hip.test_optim_rays_only = True
    rays = _render_once(graph, opt, "test-optim")
    _assert_same_render(default, rays)
    assert all(p.grad is None for p in _weights(graph))
    assert rec.fwd == [(prec | M, 64), (prec | M, 192)] and all(gp is None for _, _, gp in rec.bwd) and len(rec.bwd) == 2
    rec.clear()
    train_on = _render_once(graph, opt, "train")                           # mode "train" ignores the option
    assert all(p.grad is not None for p in _weights(graph))
    assert rec.fwd == [(prec, 64), (prec, 192)]
    opt.hip.test_optim_rays_only = False
    train_off = _render_once(graph, opt, "train")
    _assert_same_render(train_on, train_off)


def test_render_batch_of_two_pose_renders_with_frozen_networks(monkeypatch):
    opt, graph = _graph("bf16x3")
    prec = L.PREC_IDS["bf16x3"]
    pose0, intr = ring_cameras(3, H=H, W=W)
    intr = intr.to(dev())
    rs = np.random.RandomState(2)
    px = torch.from_numpy(rs.uniform(0, [W, H], size=(19, 2)).astype(np.float32)).to(dev())
    idx = torch.from_numpy(rs.randint(0, H * W, size=(23,))).to(dev())

    def run():
        p = pose0.to(dev()).requires_grad_(True)
        reqs = [dict(pose=p[:2], H=H, W=W, intr=intr[:2], pixels=px, depth_range=[1.2, 5.2], mode="val"),
                dict(pose=p, H=H, W=W, intr=intr, ray_idx=idx, depth_range=[1.5, 4.0], mode="val")]
        graph.zero_grad(set_to_none=True)
        rets = graph.render_batch(opt, reqs, iter=0)
        (_loss(rets[0]) + _loss(rets[1])).backward()
        torch.cuda.synchronize()
        return [{k: v.detach().clone() for k, v in r.items() if torch.is_tensor(v)} for r in rets], p.grad.clone()

    full = run()
    rec = Recorder(monkeypatch)
    graph.requires_grad_(False)
    rays = run()
    for a, b in zip(full[0], rays[0]):
        for k in a:
            assert _same(a[k], b[k]), k
    assert float(full[1].abs().max()) > 0 and _same(full[1], rays[1])
    assert all(p.grad is None for p in _weights(graph))
    assert rec.fwd and all(p == prec | M for p, _ in rec.fwd) and rec.bwd and all(p == prec | M and gp is None for p, _, gp in rec.bwd)


def test_twenty_iterations_of_test_time_pose_optimisation():
    """The loop shape of the reference's test-time photometric pose optimisation: Adam on a zero-initialised 6-vector through the closed-form
    twist exponential, random rays per iteration from a seeded generator.  The 6-vector after EVERY iteration is the same bits on both routes."""
    from bench_workloads import compose, se3_exp
    pose0, intr = ring_cameras(1, H=H, W=W)
    pose0, intr = pose0.to(dev()), intr.to(dev())
    target = torch.rand(1, H * W, 3, generator=torch.Generator().manual_seed(4)).to(dev())

    def run(frozen):
        opt, graph = _graph("bf16x3")
        opt.nerf.sample_intvs, opt.nerf.sample_intvs_fine = 16, 16
        graph.requires_grad_(not frozen)
        xi = torch.zeros(1, 6, device=dev(), requires_grad=True)
        optim = torch.optim.Adam([xi], lr=1e-2)
        gen = torch.Generator().manual_seed(8)
        traj = []
        for it in range(20):
            idx = torch.randperm(H * W, generator=gen)[:64].to(dev())
            torch.manual_seed(100 + it)
            optim.zero_grad()
            ret = graph.render(opt, compose(se3_exp(xi), pose0), H=H, W=W, intr=intr, ray_idx=idx, depth_range=[1.2, 5.2], iter=0, mode="test-optim")
            loss = ((ret.rgb - target[:, idx]) ** 2).mean() + ((ret.rgb_fine - target[:, idx]) ** 2).mean()
            loss.backward()
            optim.step()
            traj.append(xi.detach().clone())
        return torch.stack(traj), graph

    full, g_full = run(False)
    rays, g_rays = run(True)
    assert float(full[-1].abs().max()) > 1e-3                              # the pose moves
    for it in range(20):
        assert _same(full[it], rays[it]), it
    assert all(p.grad is None for p in _weights(g_rays)) and all(p.grad is not None for p in _weights(g_full))
