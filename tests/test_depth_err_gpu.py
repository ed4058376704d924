"""The depth errors on rendered rays on the GPU against the float64 referee (tests/depth_err_referee.py) and against
the reference's own fp32 values (tests/golden/depth_err.npz) on every fixture case; the chunk edges; no and one valid row; the fine head,
the scale forms, determinism and the image index bit for bit; the installed function behind a real small render; and graph captures.

Bounds: the kernel does double arithmetic on the stored fp32 operands and rounds each value once, so it lies within ONE fp32 spacing of
the referee (only a rounding tie can differ); and it is no farther from the reference's fp32 value than that value is from the referee
(tests/test_depth_err_cpu.py REF_DISTANCE holds those distances), plus one spacing."""
import math
import types

import numpy as np
import pytest
import torch

from sparf_amd import metrics
from sparf_amd.edict import EasyDict as edict
from tests import depth_err_referee as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def D(a):
    return torch.from_numpy(np.array(a)).to(dev()) if a is not None else None


def run(case, scale=1.0, fine=True, **over):
    """one call on a case's inputs -> (vector [4] float32 and count [1] int32 on the host, the result dict)"""
    kw = dict(ray_idx=D(case["ray_idx"]), img_idx=D(case["idx"]), scale=scale)
    kw.update(over)
    res = metrics.depth_error_on_rays(D(case["depth_gt"]), D(case["valid"]), D(case["depth"]), D(case["depth_fine"]) if fine else None, **kw)
    assert res.vector.is_cuda and res.vector.dtype == torch.float32 and res.count.dtype == torch.int32 and res.abs_e.dim() == 0
    return res.vector.cpu().numpy(), res.count.cpu().numpy(), res


def bits(a):
    return np.asarray(a).tobytes()


def apart(a, b, at):
    """|a - b| in fp32 spacings at |at|; 0 where both are NaN"""
    return R.distance(a, b) if math.isnan(at) or math.isnan(b) else abs(float(a) - float(b)) / R.spacing(at)


def within_one_spacing(got, want, what):
    dist = [R.distance(g, w) for g, w in zip(got, want)]
    print(what, "kernel to referee in fp32 spacings", [round(d, 3) for d in dist])
    assert max(dist) <= 1.0, (what, got, want, dist)


@pytest.mark.parametrize("key", R.case_names())
def test_fixture_cases_against_the_referee_and_the_reference(fx, key):
    name, scale = key.split("/")[0], float(fx[key + "/scale"])
    case = R.build(name)
    want, K = R.referee(case, scale)
    got, count, _ = run(case, scale)
    assert count.tolist() == [K]
    within_one_spacing(got, want, key)
    ref = fx[key + "/ref"]
    for g, r, w in zip(got, ref, want):
        d_got_ref, d_ref = apart(g, r, w), apart(r, w, w)          # both in spacings at the referee's value
        print(key, "kernel to reference", round(d_got_ref, 3), " reference to referee", round(d_ref, 3))
        assert d_got_ref <= d_ref + 1.0, (key, g, r, w)


@pytest.mark.parametrize("shape", R.EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_chunk_edges_on_full_images(shape):
    """4096 rows: the last one-launch size; 4097: the first two-launch size; 8710: three chunks, the last one partial"""
    B, h, w = shape
    case = R.build_edge(B, h, w)
    for scale in R.SCALES:
        want, K = R.referee(case, scale)
        got, count, _ = run(case, scale)
        assert count.tolist() == [K] and 0 < K < B * h * w
        within_one_spacing(got, want, f"{shape} s{scale}")


def test_no_valid_row_and_one_valid_row():
    case = R.build("per_image")
    none = dict(case, valid=np.zeros_like(case["valid"]))
    got, count, res = run(none)
    assert count.tolist() == [0] and int(res.n_valid) == 0
    assert got[0] == 0.0 and math.isnan(got[1]) and got[2] == 0.0 and math.isnan(got[3])
    one = dict(none, valid=none["valid"].copy())
    p = int(case["ray_idx"][2, 11])
    one["valid"].reshape(3, -1)[2, p] = True
    want, K = R.referee(one, 1.7)
    got, count, _ = run(one, 1.7)
    assert K == int((case["ray_idx"][2] == p).sum()) == 1 and count.tolist() == [1]
    within_one_spacing(got, want, "one valid row")
    # no row at all: the same (0, NaN), and no input is read
    empty = metrics.depth_error_on_rays(D(case["depth_gt"]), D(case["valid"]), torch.zeros(1, 0, 1, device=dev()), torch.zeros(1, 0, 1, device=dev()),
                                        ray_idx=torch.zeros(0, dtype=torch.int64, device=dev()))
    v = empty.vector.cpu().numpy()
    assert v[0] == 0.0 and math.isnan(v[1]) and v[2] == 0.0 and math.isnan(v[3]) and int(empty.n_valid) == 0


@pytest.mark.parametrize("name", ["per_image", "edge"])
def test_fine_head_scale_forms_and_determinism(name):
    case = R.build(name) if name != "edge" else R.build_edge(2, 65, 67)
    both, count, res = run(case, 1.7)
    assert set(res) == {"vector", "count", "abs_e", "rmse", "abs_e_fine", "rmse_fine", "n_valid"}
    # the fine pair is a second call's coarse pair given the fine depth; without a fine head the pair is 0
    alone, _, res1 = run(dict(case, depth=case["depth_fine"]), 1.7, fine=False)
    assert bits(both[2:]) == bits(alone[:2]) and alone[2:].tolist() == [0.0, 0.0] and "abs_e_fine" not in res1
    coarse, _, _ = run(case, 1.7, fine=False)
    assert bits(coarse[:2]) == bits(both[:2])
    # the scale as a float, as a 0-dim device tensor and as a float64 one on the device
    for s in (torch.tensor(1.7, device=dev()), torch.tensor([1.7], device=dev(), dtype=torch.float64), np.float32(1.7)):
        got, c, _ = run(case, s)
        assert bits(got) == bits(both) and bits(c) == bits(count)
    # a second call
    again, c, _ = run(case, 1.7)
    assert bits(again) == bits(both) and bits(c) == bits(count)
    # without a workspace the one-workgroup path serves any size, to the same bound
    if name == "edge":
        from sparf_amd import lib as L, ops
        real = L.workspace
        L.workspace = lambda nbytes, device, dtype: None
        try:
            v, c = ops.ray_depth_err(D(case["depth_gt"]), D(case["valid"]), D(case["depth"]), D(case["depth_fine"]), scale=1.7)
        finally:
            L.workspace = real
        within_one_spacing(v.cpu().numpy(), R.referee(case, 1.7)[0], "one workgroup, 8710 rows")
        assert bits(c.cpu().numpy()) == bits(count)


@pytest.mark.parametrize("name", ["subset", "full2"])
def test_image_index_equals_the_indexed_copies(name):
    """img_idx = [2, 0] on the device against a call on the maps' indexed copies, bit for bit"""
    if name == "subset":
        case = R.build("subset")
    else:
        case = dict(R.build("full"), idx=np.array([2, 0], dtype=np.int64))
        case["depth"], case["depth_fine"] = case["depth"][:2], case["depth_fine"][:2]
    assert case["idx"].tolist() == [2, 0]
    got, count, _ = run(case, 1.7)
    copies = dict(case, depth_gt=case["depth_gt"][case["idx"]], valid=case["valid"][case["idx"]], idx=None)
    want, want_count, _ = run(copies, 1.7)
    assert bits(got) == bits(want) and bits(count) == bits(want_count) and count[0] > 0
    plain, _, _ = run(dict(case, idx=None), 1.7)          # and the index matters
    assert bits(plain) != bits(got)


def test_installed_function_behind_a_real_render():
    """2 images x 64 rays, 16 + 16 samples, fp32, train mode: compute_depth_error_on_rays under the reference's name, on both heads, against
    depth_error_on_rays_torch and the referee on the same render outputs"""
    from sparf_amd.renderer import Graph
    from tests.golden.recipe import make_state_dict, ring_cameras, small_opt
    H, W, B, n = 12, 16, 2, 64
    opt = small_opt(nerf=dict(rand_rays=B * n, sample_intvs=16, sample_intvs_fine=16, sample_stratified=False))
    g = Graph(opt, dev())
    g.nerf.load_state_dict(make_state_dict(opt, 5))
    g.nerf_fine.load_state_dict(make_state_dict(opt, 6))
    g.train()
    pose, intr = ring_cameras(B, H=H, W=W)
    rs = np.random.RandomState(3)
    depth_gt, valid = R.maps_of(B, H, W)
    data = edict(idx=torch.arange(B), image=D(rs.random_sample((B, 3, H, W)).astype(np.float32)), intr=intr.to(dev()), pose=pose.to(dev()),
                 depth_range=torch.tensor([[1.2, 5.2]] * B, device=dev()), depth_gt=D(depth_gt), valid_depth_gt=D(valid))
    idx = D(rs.permutation(H * W)[:n].astype(np.int64))
    torch.manual_seed(2)
    ret = g.render_image_at_specific_rays(opt, data, iter=10, ray_idx=idx, mode="train")
    ret.ray_idx = idx
    ret.idx_img_rendered = torch.arange(B, device=dev())
    core, trainer = types.SimpleNamespace(compute_depth_error_on_rays=None), types.SimpleNamespace(compute_depth_error_on_rays=None)
    metrics.install_depth_error_on_rays(core, trainer)
    try:
        with torch.no_grad():
            got = [float(v) for head in (ret.depth, ret.depth_fine) for v in trainer.compute_depth_error_on_rays(data, ret, head, 1.7)]
            rest = metrics.depth_error_on_rays_torch(data.depth_gt, data.valid_depth_gt, ret.depth, ret.depth_fine, ray_idx=idx, img_idx=ret.idx_img_rendered,
                                                     scale=1.7).vector.tolist()
    finally:
        metrics.uninstall_depth_error_on_rays()
    case = dict(depth_gt=depth_gt, valid=valid, idx=None, ray_idx=idx.cpu().numpy(), depth=ret.depth.detach().cpu().numpy().reshape(B, n, 1),
                depth_fine=ret.depth_fine.detach().cpu().numpy().reshape(B, n, 1))
    want, K = R.referee(case, 1.7)
    assert K > 0 and all(math.isfinite(v) for v in got)
    within_one_spacing(got, want, "installed, real render")
    for a, r, w in zip(got, rest, want):
        d, d_rest = apart(a, r, w), apart(r, w, w)
        print("installed to restatement", round(d, 3), " restatement to referee", round(d_rest, 3))
        assert d <= d_rest + 1.0


@pytest.mark.parametrize("shape", [(1, 64, 64), (2, 65, 67)], ids=["4096", "8710"])
def test_graph_replay_gives_the_eager_bits(shape):
    """one capture on a single stream of the one-launch size and of the two-launch size, replayed once"""
    case = R.build_edge(*shape)
    args = [D(case[k]) for k in ("depth_gt", "valid", "depth", "depth_fine")]
    scale = torch.tensor(1.7, device=dev())
    call = lambda: metrics.depth_error_on_rays(*args, scale=scale)
    eager = call()
    eager = (eager.vector.clone(), eager.count.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = call()
    static.vector.zero_()
    static.count.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static.count, eager[1]) and bits(static.vector.cpu().numpy()) == bits(eager[0].cpu().numpy()) and int(eager[1]) > 0
