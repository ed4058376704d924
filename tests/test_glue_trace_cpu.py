"""What ops.NerfPass (through nerf_pass / nerf_pass_segments) and ops.RenderFn (through render_fused) hand the C ABI, checked without a
GPU: every size query, sampling call and pass call they issue on CPU tensors over a stand-in library that launches nothing
(tests/glue_fake.py), in order, with every scalar, every struct field and the aliasing of every pointer, against
tests/golden/glue_trace.json -- recorded by this file's own recorder on the commit BEFORE the pass preparers existed
(`python -m tests.test_glue_trace_cpu --record` writes the file; it goes through the three public functions only)."""
import json
import os

import pytest
import torch

from sparf_amd import lib as L
from sparf_amd import ops
from tests.glue_fake import installed

TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glue_trace.json")
X3, FP32 = L.PREC_IDS["bf16x3"], L.PREC_FP32


def _blob():
    return torch.zeros(8, dtype=torch.uint8)


def _rays(R, grad):
    return torch.zeros(R, 3, requires_grad=grad), torch.ones(R, 3, requires_grad=grad)


def _params(grad):
    return [torch.zeros(n, requires_grad=grad) for (o, i) in L.LAYER_SHAPES for n in ((o, i), (o,))]


def _loss(out, R):
    """a dense upstream gradient on rgb, a broadcast one (not contiguous: the glue must make it dense) on depth_var"""
    return (out["rgb"] * torch.full((R, 3), 2.0)).sum() + out["depth_var"].sum()


def nerf_pass(prec=X3, R=6, N=8, rays=False, params=True, noise=False, grad=True, far=None):
    c, d = _rays(R, rays)
    far = (far[0], far[1], _blob()) if far is not None else None
    with torch.set_grad_enabled(grad):
        out = ops.nerf_pass(c, d, torch.ones(R, N), torch.zeros(R, N) if noise else None, 0.25 if noise else 0.0, True, prec, _blob(),
                            torch.ones(16), _params(params), far=far)
    if grad:
        _loss(out, R).backward()


def nerf_pass_segments():
    R, N = 7, 4
    c, d = _rays(R, True)
    outs = ops.nerf_pass_segments(c, d, torch.ones(R, N), torch.zeros(R, N), False, X3, _blob(), torch.ones(16), _params(True),
                                  [(0, 3, 0.125), (3, 0, 0.0), (3, 4, 0.5)])
    assert [o["rgb"].shape[0] for o in outs] == [3, 0, 4]
    (_loss(outs[0], 3) + outs[2]["weights"].sum()).backward()


def render_fused(fine=True, noise=False, c2f=None, far=None, frozen_c=False, grad=True, loss=("c", "f")):
    R, Nc, Nf = 5, 4, 4
    cfg = dict(R=R, Nc=Nc, Nf=Nf, fine=fine, dmin=1.0, dmax=2.5, scale=1.5, inverse=False, u_const=0.5, noise_scale=0.5 if noise else 0.0,
               white_bg=False, prec_c=X3, prec_f=X3, far_c=far, far_f=far, c2f=c2f)
    c, d = _rays(R, True)
    theta = [None if frozen_c else torch.zeros(L.N_PARAMS, requires_grad=True), torch.zeros(L.N_PARAMS, requires_grad=True) if fine else None]
    fblob = lambda on: _blob() if (far is not None and on) else None
    with torch.set_grad_enabled(grad):
        coarse, fine_out = ops.render_fused(c, d, cfg, torch.zeros(R, Nc), torch.full((Nf,), 0.5) if fine else None,
                                            torch.zeros(R, Nc) if noise else None, torch.zeros(R, Nc + Nf) if (noise and fine) else None, None,
                                            _blob(), _blob() if fine else None, fblob(True), fblob(fine), torch.ones(()),
                                            torch.ones(()) if fine else None, *theta)
    if grad:
        sum(_loss(o, R) for tag, o in (("c", coarse), ("f", fine_out)) if tag in loss).backward()


# name -> the call that issues the case: R = 5-7 rays, N = 4-8 samples (32 for the far tiles), bf16x3 unless the name says otherwise
CASES = {
    "nerf_pass/a_training_noise": lambda: nerf_pass(noise=True),
    "nerf_pass/b_no_grad": lambda: nerf_pass(grad=False),
    "nerf_pass/c_frozen_rays_masks": lambda: nerf_pass(rays=True, params=False),
    "nerf_pass/d_frozen_rays_q8_full": lambda: nerf_pass(prec=L.PREC_IDS["bf16x3+q8"], rays=True, params=False),
    "nerf_pass/e_fp32": lambda: nerf_pass(prec=FP32, rays=True),
    "nerf_pass/f_far_rows_training": lambda: nerf_pass(rays=True, far=(2, FP32)),
    "nerf_pass/g_far_tiles_inference": lambda: nerf_pass(N=32, grad=False, far=(8.0, FP32)),
    "nerf_pass_segments/a_three_segments": nerf_pass_segments,
    "render_fused/a_c2f_noise_both": lambda: render_fused(noise=True, c2f=(0.1, 0.5)),
    "render_fused/b_fine_only": lambda: render_fused(loss=("f",)),
    "render_fused/c_fine_off": lambda: render_fused(fine=False, loss=("c",)),
    "render_fused/d_far_rows_coarse_frozen": lambda: render_fused(far=(2, FP32), frozen_c=True),
    "render_fused/e_no_grad": lambda: render_fused(grad=False),
}


def record(name):
    """-> the C-ABI calls one case issues, in order (as JSON holds them)"""
    with installed() as lib:
        CASES[name]()
        return json.loads(json.dumps(lib.trace))


@pytest.fixture(scope="module")
def golden():
    with open(TRACE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_glue_hands_the_c_abi_what_the_recorded_trace_says(golden, name):
    got, want = record(name), golden[name]
    assert [e["call"] for e in got] == [e["call"] for e in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, i, {k: (g["args"].get(k), w["args"].get(k)) for k in w["args"] if g["args"].get(k) != w["args"].get(k)})


def test_the_trace_holds_the_situations_it_is_there_for(golden):
    """the recorded cases do show the routes, the aliasing and the flags they were chosen for (a trace recorded from a case table that
    missed them would pin nothing)"""
    M, Q8 = L.SAVE_MASKS, L.SAVE_Q8
    assert sorted(golden) == sorted(CASES)
    calls = lambda name, call: [e["args"] for e in golden[name] if e["call"] == call]
    fwd, bwd = (lambda name: calls(name, "sparf_pass_forward")), (lambda name: calls(name, "sparf_pass_backward"))
    for name in CASES:           # a backward reads what its forward wrote, at the same addresses
        by_n = {f["nsamp"]: f for f in fwd(name)}
        for b in bwd(name):
            f = by_n[b["nsamp"]]
            assert b["save"] is not None and all(b[k] == f[k] for k in ("save", "sigma_raw", "t", "raylen", "rgb_samples", "weights", "packed", "c2f", "prec"))
            assert (b["grad_params"] is None) == bool(b["prec"] & M) and b["ws"] is not None and b["tables"] is not None
    a = "nerf_pass/a_training_noise"
    assert fwd(a)[0]["noise"] is not None and fwd(a)[0]["noise_scale"] == 0.25 and fwd(a)[0]["white_bg"] == 1
    assert bwd(a)[0]["g_rgb"] is not None and bwd(a)[0]["g_depth_var"] is not None and bwd(a)[0]["g_depth"] is None and bwd(a)[0]["d_dir"] is None
    assert fwd("nerf_pass/b_no_grad")[0]["save"] is None and not bwd("nerf_pass/b_no_grad")
    assert fwd("nerf_pass/c_frozen_rays_masks")[0]["prec"] == X3 | M and bwd("nerf_pass/c_frozen_rays_masks")[0]["d_center"] is not None
    assert fwd("nerf_pass/d_frozen_rays_q8_full")[0]["prec"] == X3 | Q8 and bwd("nerf_pass/d_frozen_rays_q8_full")[0]["grad_params"] is not None
    assert fwd("nerf_pass/e_fp32")[0]["prec"] == FP32
    f = fwd("nerf_pass/f_far_rows_training")[0]
    assert (f["far_count"], f["far_prec"]) == (2, FP32) and None not in (f["far_packed"], f["far_ws"], f["far_venc_ws"])
    assert [e["args"]["rows"] for e in golden["nerf_pass/f_far_rows_training"] if e["call"] == "sparf_save_bytes"] == [6 * 8, 6 * 2]
    f = fwd("nerf_pass/g_far_tiles_inference")[0]
    assert (f["far_count"], f["far_thr"], f["nsamp"], f["far_ws"], f["save"]) == (-1, 8.0, 32, None, None)
    f, b = fwd("nerf_pass_segments/a_three_segments")[0], bwd("nerf_pass_segments/a_three_segments")[0]
    assert [(s["ray0"], s["nrays"], s["noise_scale"]) for s in f["seg"]] == [(0, 3, 0.125), (3, 0, 0.0), (3, 4, 0.5)] and f["noise_scale"] == 0.0
    assert b["nseg"] == 3 and b["g_rgb"] is None and [(s["g_rgb"] is None, s["g_weights"] is None) for s in b["seg"]] == [(False, True), (True, True), (True, False)]
    a = "render_fused/a_c2f_noise_both"
    assert [e["call"] for e in golden[a]].count("sparf_c2f_weights") == 2 and len(calls(a, "sparf_sample_fine_hostgrid")) == 1
    assert [x["accumulate_rays"] for x in bwd(a)] == [0, 1] and bwd(a)[0]["d_center"] == bwd(a)[1]["d_center"] and bwd(a)[0]["grad_params"] != bwd(a)[1]["grad_params"]
    assert fwd(a)[0]["c2f"] != fwd(a)[1]["c2f"] and fwd(a)[0]["center"] == fwd(a)[1]["center"]
    # the fine pass runs on the resampler's output, which read the coarse pass's weights and depths
    rs = calls(a, "sparf_sample_fine_hostgrid")[0]
    assert rs["out"] == fwd(a)[1]["t"] and rs["weights"] == fwd(a)[0]["weights"] and rs["t_coarse"] == fwd(a)[0]["t"] == calls(a, "sparf_sample_coarse")[0]["out"]
    assert [x["nsamp"] for x in bwd("render_fused/b_fine_only")] == [8] and bwd("render_fused/b_fine_only")[0]["accumulate_rays"] == 0
    assert [x["nsamp"] for x in fwd("render_fused/c_fine_off")] == [4] and not calls("render_fused/c_fine_off", "sparf_sample_fine_hostgrid")
    d = "render_fused/d_far_rows_coarse_frozen"
    assert [x["prec"] for x in fwd(d)] == [X3 | M, X3] and [x["grad_params"] is None for x in bwd(d)] == [True, False]
    assert all(x["far_count"] == 2 and x["far_ws"] is not None for x in fwd(d)) and fwd(d)[0]["far_packed"] != fwd(d)[1]["far_packed"]
    e = "render_fused/e_no_grad"
    assert all(x["save"] is None for x in fwd(e)) and not bwd(e) and not calls(e, "sparf_save_bytes")


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--record"]:
        with open(TRACE, "w") as f:
            json.dump({k: record(k) for k in sorted(CASES)}, f, indent=0, sort_keys=True)
            f.write("\n")
