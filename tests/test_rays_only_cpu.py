"""Ray-gradient-only passes (C ABI 7, SPARF_SAVE_MASKS), the part that needs no GPU: the ABI version and its mirrors, the host arithmetic
of the masks-only save area and of the backward workspace, the routing function of the Python glue, the compiled instruction
stream of the seven new kernels against their plane-saving counterparts (tools/kernel_stream.py; a unit without a current object is
compiled first), and the route as the C ABI sees it -- ops.NerfPass, ops.RenderFn, Graph.render and Graph.render_batch on CPU tensors
over a stand-in library (tests/glue_fake.py) that launches nothing and records the precision id and grad_params of every pass call."""
import importlib.util
import os
import re

import pytest

from sparf_amd import lib as L
from sparf_amd import ops
from tests.glue_fake import fake  # noqa: F401  (the stand-in library, as a fixture)
from tests.test_kernel_stream_cpu import _BWD, _BWX, _FWD, ALL_KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = [L.PREC_BF16, L.PREC_FP32, L.PREC_X3]
MASK_TILE = 9 * 1024                         # SB_COUNT * MASK_TILE_BYTES (csrc/layout.h)
GRAD_COLS = 7 * 256 + 288 + 128 + 32         # csrc/layout.h


def ntiles32(rows):
    return (rows + 255) // 256 * 256 // 32


def test_abi_version_and_its_mirrors_agree_on_7():
    hdr = open(os.path.join(ROOT, "include", "sparf_hip.h")).read()
    assert re.search(r"^#define SPARF_ABI_VERSION 7\b", hdr, flags=re.M)
    assert re.search(r"^#define SPARF_SAVE_MASKS 32\b", hdr, flags=re.M)
    assert L.ABI_VERSION == 7 and L.SAVE_MASKS == 32
    assert L.load().sparf_abi_version() == 7
    assert L.base_prec(L.PREC_X3 | L.SAVE_MASKS) == L.PREC_X3 and L.base_prec(L.PREC_BF16 | L.SAVE_Q8) == L.PREC_BF16


@pytest.mark.parametrize("rows", [1, 1680, 32960])
@pytest.mark.parametrize("prec", PRECS)
def test_masks_only_save_area_is_the_mask_kib_of_every_tile(prec, rows):
    lib = L.load()
    assert lib.sparf_save_bytes(prec | L.SAVE_MASKS, rows) == ntiles32(rows) * MASK_TILE
    assert lib.sparf_save_bytes(prec, rows) > lib.sparf_save_bytes(prec | L.SAVE_MASKS, rows)


@pytest.mark.parametrize("prec", PRECS)
def test_masks_with_q8_is_refused_like_an_invalid_precision(prec):
    lib = L.load()
    bad = prec | L.SAVE_MASKS | L.SAVE_Q8
    assert lib.sparf_save_bytes(bad, 1680) == lib.sparf_save_bytes(7, 1680) == -1
    assert lib.sparf_bwd_workspace_bytes(bad, 70, 24, 1) == lib.sparf_bwd_workspace_bytes(7, 70, 24, 1) == -1
    assert lib.sparf_save_bytes(7 | L.SAVE_MASKS, 1680) == -1           # (an invalid base id stays invalid under the flag)


@pytest.mark.parametrize("R,N", [(70, 24), (515, 64), (4096, 192)])
@pytest.mark.parametrize("prec", PRECS)
def test_backward_workspace_drops_the_gradient_area_and_the_partial_blocks(prec, R, N):
    lib = L.load()
    full, masks = lib.sparf_bwd_workspace_bytes(prec, R, N, 1), lib.sparf_bwd_workspace_bytes(prec | L.SAVE_MASKS, R, N, 1)
    grad_area = ntiles32(R * N) * GRAD_COLS * 32 * (4 if prec == L.PREC_FP32 else 2)
    assert 0 < masks <= full - grad_area, (full, masks, grad_area)
    # what is left: d sigma, d z, d |ray|, d point, d view encoding -- each rounded up to 256 bytes
    al = lambda b: (b + 255) // 256 * 256
    assert masks == al(R * N * 4) + al(R * N * 12) + al(R * 4) + al(R * N * 12) + al(R * N * 128)


@pytest.mark.parametrize("prec", PRECS)
def test_masks_without_ray_gradients_is_refused(prec):
    lib = L.load()
    assert lib.sparf_bwd_workspace_bytes(prec | L.SAVE_MASKS, 70, 24, 0) == -1
    assert lib.sparf_bwd_workspace_bytes(prec, 70, 24, 0) > 0


def test_routing_truth_table():
    N, F, M = ops.SAVE_NONE, ops.SAVE_FULL, ops.SAVE_MASKS
    for name, prec in L.PREC_IDS.items():
        q8 = name.endswith("+q8")
        for grad in (False, True):
            for rays in (False, True):
                for params in (False, True):
                    want = N if not grad or not (rays or params) else M if (rays and not params and not q8) else F
                    assert ops.save_kind(grad, rays, params, prec) == want, (name, grad, rays, params)
    # the cases by name: pose optimisation against a frozen network; a '+q8' mode keeps the full route; a training pass; nothing
    # differentiable = the inference kernel, as before; no grad mode = nothing
    assert ops.save_kind(True, True, False, L.PREC_X3) == M
    assert ops.save_kind(True, True, False, L.PREC_X3 | L.SAVE_Q8) == F
    assert ops.save_kind(True, True, True, L.PREC_X3) == F and ops.save_kind(True, False, True, L.PREC_FP32) == F
    assert ops.save_kind(True, False, False, L.PREC_X3) == N and ops.save_kind(False, True, False, L.PREC_X3) == N
    # the mixed render: decided per pass -- coarse network frozen, fine network trainable, rays with a gradient
    assert [ops.save_kind(True, True, p, L.PREC_X3) for p in (False, True)] == [M, F]
    assert ops.pass_prec_of(L.PREC_X3, M) == L.PREC_X3 | L.SAVE_MASKS and ops.pass_prec_of(L.PREC_X3, F) == L.PREC_X3
    assert ops.pass_prec_of(L.PREC_FP32, N) == L.PREC_FP32


# new unit -> its counterpart: (unit, mangled kernel name) of tests/test_kernel_stream_cpu.py ALL_KERNELS, + MFMA count where that file pins one
COUNTERPART = {
    "rays_fwd_bf16.hip": (("mlp_fwd_bf16_train.hip", _FWD % (0, 1)), None),
    "rays_fwd_fp32.hip": (("mlp_fwd_fp32_train.hip", _FWD % (1, 1)), None),
    "rays_fwd_x3.hip": (("mlp_fwd_x3_train.hip", _FWD % (2, 1)), 3168),
    "rays_bwd.hip": (("mlp_bwd.hip", _BWD % (0, 1, 0, 0)), None),
    "rays_bwd_fp32.hip": (("mlp_bwd_fp32.hip", _BWD % (1, 1, 1, 0)), None),
    "rays_bwd_x3.hip": (("mlp_bwd_x3.hip", _BWX % (1, 8, 0)), 2088),
    "rays_bwd_x3w4.hip": (("mlp_bwd_x3w4.hip", _BWX % (1, 4, 0)), None),
}


@pytest.fixture(scope="module")
def stream():
    spec = importlib.util.spec_from_file_location("kernel_stream", os.path.join(ROOT, "tools", "kernel_stream.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_new_units_are_built_and_named_apart_from_the_mlp_units(stream):
    from sparf_amd import build as B
    assert set(COUNTERPART) <= set(B.SOURCES)
    assert not set(COUNTERPART) & set(stream.MLP_UNITS)


@pytest.mark.parametrize("unit", sorted(COUNTERPART))
def test_compiled_stream_against_the_plane_saving_counterpart(stream, unit):
    (cunit, cname), mfma = COUNTERPART[unit]
    figs = stream.figures(unit)
    assert len(figs) == 1, list(figs)                    # one kernel per new unit
    (name, f), = figs.items()
    c = stream.figures(cunit)[cname]
    _, vgpr_allowed, scratch_allowed, _ = ALL_KERNELS[(cunit, cname)]
    print(unit, name, f)
    print("   counterpart", cunit, c)
    assert f["mfma"] == c["mfma"] and (mfma is None or f["mfma"] == mfma), (f, c)
    assert f["group_segment_fixed_size"] == c["group_segment_fixed_size"], (f, c)
    assert f["vgpr_count"] <= vgpr_allowed, (f, vgpr_allowed)
    assert f["private_segment_fixed_size"] <= min(scratch_allowed, c["private_segment_fixed_size"]), (f, c)
    assert f["sgpr_spill_count"] == 0 and f["v_readlane_b32"] == 0 and f["v_writelane_b32"] == 0, f          # no parked scalars
    assert f["buffer_store_dwordx4"] < c["buffer_store_dwordx4"], (f["buffer_store_dwordx4"], c["buffer_store_dwordx4"])


# ---------------------------------------------------------------------------------------------- the route as the C ABI sees it, no GPU
def _params(requires_grad):
    import torch
    return [torch.zeros(n, requires_grad=requires_grad) for (o, i) in L.LAYER_SHAPES for n in ((o, i), (o,))]


@pytest.mark.parametrize("name", ["bf16x3", "fp32", "bf16x3+q8"])
def test_nerf_pass_routes_frozen_networks_to_the_flag(fake, name):
    import torch
    prec = L.PREC_IDS[name]
    R, N = 5, 8
    for frozen, rays in ((False, True), (True, True), (True, False), (False, False)):
        fake.fwd, fake.bwd = [], []
        c, d = torch.zeros(R, 3, requires_grad=rays), torch.ones(R, 3, requires_grad=rays)
        params = _params(not frozen)
        out = ops.nerf_pass(c, d, torch.ones(R, N), None, 0.0, False, prec, torch.zeros(8, dtype=torch.uint8), torch.ones(16), params)
        masks = frozen and rays and not name.endswith("+q8")
        want = prec | L.SAVE_MASKS if masks else prec
        assert fake.fwd == [(want, N, rays or not frozen)], (frozen, rays, fake.fwd)
        if rays or not frozen:
            (out["rgb"].sum() + out["depth"].sum()).backward()
            assert fake.bwd == [(want, N, not masks)], (frozen, rays, fake.bwd)
            assert (c.grad is not None) == rays and all((p.grad is not None) == (not frozen) for p in params)


def _render_fused(fake, prec, frozen_c, frozen_f, rays):
    import torch
    R, Nc, Nf = 6, 4, 4
    cfg = dict(R=R, Nc=Nc, Nf=Nf, fine=True, dmin=1.0, dmax=2.0, scale=1.0, inverse=False, u_const=0.5, noise_scale=0.0, white_bg=False,
               prec_c=prec, prec_f=prec, far_c=None, far_f=None, c2f=None)
    c, d = torch.zeros(R, 3, requires_grad=rays), torch.ones(R, 3, requires_grad=rays)
    theta = [None if fz else torch.zeros(L.N_PARAMS, requires_grad=True) for fz in (frozen_c, frozen_f)]
    blob = torch.zeros(8, dtype=torch.uint8)
    fake.fwd, fake.bwd = [], []
    coarse, fine = ops.render_fused(c, d, cfg, None, torch.full((Nf,), 0.5), None, None, None, blob, blob, None, None, torch.ones(()), torch.ones(()), *theta)
    return c, theta, coarse, fine


def test_render_fn_decides_per_pass(fake):
    prec, M = L.PREC_X3, L.SAVE_MASKS
    # both frozen under rays with a gradient: both passes carry the flag, no grad_params, pose gradients come back
    c, theta, coarse, fine = _render_fused(fake, prec, True, True, True)
    assert fake.fwd == [(prec | M, 4, True), (prec | M, 8, True)]
    (coarse["rgb"].sum() + fine["rgb"].sum()).backward()
    assert fake.bwd == [(prec | M, 4, False), (prec | M, 8, False)] and c.grad is not None
    # the mixed render: coarse frozen, fine trainable
    c, theta, coarse, fine = _render_fused(fake, prec, True, False, True)
    assert fake.fwd == [(prec | M, 4, True), (prec, 8, True)]
    (coarse["rgb"].sum() + fine["rgb"].sum()).backward()
    assert fake.bwd == [(prec | M, 4, False), (prec, 8, True)] and c.grad is not None and theta[1].grad is not None
    # a training render; a render with nothing differentiable (the inference kernels, as before); '+q8' keeps the full route
    c, theta, coarse, fine = _render_fused(fake, prec, False, False, True)
    assert fake.fwd == [(prec, 4, True), (prec, 8, True)]
    fine["rgb"].sum().backward()
    assert fake.bwd == [(prec, 8, True)] and theta[1].grad is not None
    _render_fused(fake, prec, True, True, False)
    assert fake.fwd == [(prec, 4, False), (prec, 8, False)]
    q8 = prec | L.SAVE_Q8
    _render_fused(fake, q8, True, True, True)
    assert fake.fwd == [(q8, 4, True), (q8, 8, True)]


@pytest.mark.parametrize("fused", [True, False], ids=["fused_render", "pass_by_pass"])
def test_graph_option_test_optim_rays_only(fake, monkeypatch, fused):
    """opt.hip.test_optim_rays_only through Graph.render: off by default; on, a render in mode "test-optim" hands the networks' parameters to
    no autograd node and both passes carry the flag; mode "train" ignores it"""
    import torch
    from sparf_amd import frequency_nerf, renderer
    from sparf_amd.config import HIP_DEFAULTS, hip_option
    from tests.golden.recipe import ring_cameras, small_opt
    assert HIP_DEFAULTS["test_optim_rays_only"] is False and hip_option(small_opt(), "test_optim_rays_only") is False
    for mod in (renderer, frequency_nerf):
        monkeypatch.setattr(mod, "max_rows_per_call", lambda prec=None, device=None, need=None, far=None: 1 << 20)
    opt = small_opt(hip=dict(precision="bf16x3", fused_render=fused, fused_rays=False))
    graph = renderer.Graph(opt, torch.device("cpu"))
    prec, M = L.PREC_X3, L.SAVE_MASKS
    H, W = 6, 8
    pose0, intr = ring_cameras(1, H=H, W=W)

    def run(mode):
        fake.fwd, fake.bwd = [], []
        graph.zero_grad(set_to_none=True)
        pose = pose0.clone().requires_grad_(True)
        ret = graph.render(opt, pose, H=H, W=W, intr=intr, ray_idx=torch.arange(16), depth_range=[1.2, 5.2], iter=0, mode=mode)
        (ret.rgb.sum() + ret.rgb_fine.sum()).backward()
        weights = graph.nerf.hip_params() + graph.nerf_fine.hip_params()
        return [f[0] for f in fake.fwd], sorted(fake.bwd), [p.grad is not None for p in weights], pose.grad is not None

    full = ([prec, prec], [(prec, 8, True), (prec, 16, True)], [True] * 40, True)
    assert run("test-optim") == full                      # the default: as before
    opt.hip.test_optim_rays_only = True
    assert run("test-optim") == ([prec | M, prec | M], [(prec | M, 8, False), (prec | M, 16, False)], [False] * 40, True)
    assert run("train") == full
    # frozen networks need no option
    opt.hip.test_optim_rays_only = False
    graph.nerf.requires_grad_(False)
    assert run("train") == ([prec | M, prec], sorted([(prec | M, 8, False), (prec, 16, True)]), [False] * 20 + [True] * 20, True)


def test_render_batch_segment_path_routes_frozen_networks(fake, monkeypatch):
    import torch
    from sparf_amd import frequency_nerf, renderer
    from tests.golden.recipe import ring_cameras, small_opt
    for mod in (renderer, frequency_nerf):
        monkeypatch.setattr(mod, "max_rows_per_call", lambda prec=None, device=None, need=None, far=None: 1 << 20)
    opt = small_opt(hip=dict(precision="bf16x3", fused_rays=False))
    graph = renderer.Graph(opt, torch.device("cpu"))
    prec, M = L.PREC_X3, L.SAVE_MASKS
    H, W = 6, 8
    pose0, intr = ring_cameras(2, H=H, W=W)

    def run():
        fake.fwd, fake.bwd = [], []
        pose = pose0.clone().requires_grad_(True)
        reqs = [dict(pose=pose[:1], H=H, W=W, intr=intr[:1], ray_idx=torch.arange(10), depth_range=[1.2, 5.2], mode="val"),
                dict(pose=pose, H=H, W=W, intr=intr, ray_idx=torch.arange(7), depth_range=[1.5, 4.0], mode="val")]
        rets = graph.render_batch(opt, reqs, iter=0)
        (rets[0].rgb_fine.sum() + rets[1].depth_fine.sum() + rets[1].rgb.sum()).backward()
        return [f[0] for f in fake.fwd], sorted(b[0::2] for b in fake.bwd), pose.grad is not None

    assert run() == ([prec, prec], [(prec, True), (prec, True)], True)
    graph.requires_grad_(False)
    assert run() == ([prec | M, prec | M], [(prec | M, False), (prec | M, False)], True)
