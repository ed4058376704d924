"""The evaluation-metrics kernel on the GPU (csrc/metrics.hip behind sparf_amd.metrics.image_metrics): every case of
tests/metrics_referee.py against the float64 referee -- one fp32 spacing of the referee's value per finite output, NaN / inf in the same
places, the counts exact -- and against the reference's own recorded values; the strided forms, one head or two, repeated calls and
replays of a captured graph bit for bit; Graph.evaluate_metrics behind a real render.  Run with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

from sparf_amd import metrics
from tests import metrics_referee as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def D(a):
    return torch.from_numpy(np.array(a)).to(dev()) if a is not None else None


def trainer_form(a):
    """[B,3,H,W] -> the trainer's prediction: a channel-last buffer under a permuted view (nerf_trainer.py:391)"""
    B, _, H, W = a.shape
    return D(a).permute(0, 2, 3, 1).contiguous().view(-1, H, W, 3).permute(0, 3, 1, 2)


def operands(x, form=trainer_form):
    B = x["B"]
    d3 = lambda a: D(a).reshape(B, -1, 1) if a is not None else None
    return dict(pred=form(x["pred"]), gt=D(x["gt"]), pred_fine=form(x["fine"]) if x["fine"] is not None else None,
                fg_mask=D(x["mask"]).reshape(B, 1, x["H"], x["W"]) if x["mask"] is not None else None, depth=d3(x["depth"]), depth_fine=d3(x["depth_fine"]),
                depth_gt=d3(x["depth_gt"]), valid_depth_gt=D(x["valid"]), depth_scale=x["scale"])


def run(ops_):
    ops_ = dict(ops_)
    return metrics.image_metrics(ops_.pop("pred"), ops_.pop("gt"), **ops_)


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def results(fx):
    """per case, computed once: the inputs, the referee's values and the kernel's (vector and counts on the host)"""
    cache = {}

    def get(name):
        if name not in cache:
            x = R.inputs(name)
            res = run(operands(x))
            assert res.vector.is_cuda and res.vector.dtype == torch.float32 and res.counts.dtype == torch.int32
            cache[name] = (x, R.want(x, fx["window"]), res.vector.cpu().numpy(), res.counts.cpu().numpy())
        return cache[name]
    return get


@pytest.mark.parametrize("name", R.CASES)
def test_kernel_against_the_referee(results, name):
    x, w, got, counts = results(name)
    heads = w["out"].shape[0]
    assert R.same_pattern(got[:heads], w["out"]) and (heads == 2 or np.isnan(got[1]).all())
    assert np.array_equal(counts, w["counts"])
    d = R.spacings(got[:heads], w["out"])
    print(name, "kernel to float64, worst output:", np.nanmax(d), "fp32 spacings")
    assert np.nanmax(d) <= R.BOUND, d
    c = R.CASES[name]
    if c["content"] == "identical":
        assert (got[:heads, 0] == 0).all() and np.isposinf(got[:heads, 1]).all() and (got[:heads, 2] == 1.0).all() and (got[:heads, 5] == 1.0).all()
    if c["mask"] == "none":
        assert np.isnan(got[:heads, 3:5]).all() and (got[:heads, 5] == 1.0).all()
    if c["depth"] == "none":
        assert (got[:heads, 6] == 0).all() and np.isnan(got[:heads, 7]).all() and (got[:heads, 8] == 0).all()


@pytest.mark.parametrize("name", R.CASES)
def test_kernel_against_the_references_recorded_values(fx, results, name):
    """no farther from the reference's value than the reference's own distance from float64 plus the kernel's bound"""
    x, w, got, _ = results(name)
    ref, refdist = fx[f"ref_{name}"], fx[f"refdist_{name}"]
    heads = ref.shape[0]
    assert R.same_pattern(got[:heads], ref)
    fin = np.isfinite(w["out"])
    sp = np.spacing(np.abs(np.where(fin, w["out"], 1.0)).astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):                  # (inf - inf where both are +inf: not a finite output)
        d = np.abs(got[:heads].astype(np.float64) - ref.astype(np.float64)) / sp
    assert (d[fin] <= refdist[fin] + R.BOUND).all(), (d, refdist)


def bits(res):
    return res.vector.cpu().numpy().view(np.uint32).copy(), res.counts.cpu().numpy().copy()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["s17x65", "big", "s5x7"])
def test_strided_forms_give_the_contiguous_bits(name):
    x = R.inputs(name)
    B, H, W = x["B"], x["H"], x["W"]
    dense = bits(run(operands(x, form=D)))
    assert same(bits(run(operands(x, form=trainer_form))), dense)                            # the permuted view of a channel-last buffer

    def offset(a):                                                                          # a storage offset
        buf = torch.zeros(a.size + 7, device=dev())
        buf[7:] = D(a).reshape(-1)
        return buf[7:].view(a.shape)

    def pitched(a):                                                                         # a row pitch and a batch of a larger one
        big = torch.full((B + 1, 3, H + 2, W + 5), 9.0, device=dev())
        big[1:, :, 1:H + 1, 3:W + 3] = D(a)
        return big[1:, :, 1:H + 1, 3:W + 3]

    def reshaped(a):                                                                        # reshape(-1, 3, H, W) of a stack of views
        return D(a)[None].reshape(-1, 3, H, W)

    for form in (offset, pitched, reshaped):
        o = operands(x, form=form)
        o["gt"] = form(x["gt"])
        assert same(bits(run(o)), dense), form.__name__
    o = operands(x, form=D)
    o["fg_mask"] = D(x["mask"])                                                             # [B,H,W]
    o["valid_depth_gt"] = D(x["valid"]).reshape(B, 1, H, W)
    assert same(bits(run(o)), dense)


@pytest.mark.parametrize("name", ["s17x65", "big", "const37x38"])
def test_two_heads_against_two_one_head_calls_and_two_calls(name):
    x = R.inputs(name)
    o = operands(x)
    both = bits(run(o))
    assert same(bits(run(o)), both)                                                         # two eager calls
    coarse = bits(run(dict(o, pred_fine=None, depth_fine=None)))
    fine = bits(run(dict(o, pred=o["pred_fine"], depth=o["depth_fine"], pred_fine=None, depth_fine=None)))
    assert np.array_equal(coarse[0][0], both[0][0]) and np.array_equal(fine[0][0], both[0][1])
    assert np.array_equal(coarse[1], both[1]) and np.isnan(coarse[0].view(np.float32)[1]).all()


def test_graph_replays_give_the_eager_bits():
    """a capture of image_metrics alone: no readback inside"""
    x = R.inputs("s37x38")
    o = operands(x)
    eager = bits(run(o))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(o)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run(o)
    for _ in range(2):
        static.vector.zero_()
        static.counts.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same(bits(static), eager)


def test_ssim_and_the_installed_functions_on_the_device():
    x = R.inputs("s17x65")
    o = operands(x)
    res = run(o)
    assert float(metrics.ssim(o["pred"], o["gt"])) == float(res.ssim)
    from sparf_amd.edict import EasyDict as edict
    B, H, W = x["B"], x["H"], x["W"]
    data = edict(idx=torch.arange(B, device=dev()), fg_mask=o["fg_mask"], depth_gt=o["depth_gt"].reshape(B, 1, H, W), valid_depth_gt=o["valid_depth_gt"].reshape(B, 1, H, W))
    output = edict(idx_img_rendered=torch.arange(B, device=dev()))
    got = metrics.compute_metrics(data, output, o["pred"], o["depth"], o["gt"], lambda a, b: torch.tensor(R.LPIPS), x["scale"], suffix="_x")
    v = res.vector[0].tolist()
    assert all(type(val) is float for val in got.values()) and list(got) == [k + "_x" for k in R.DICT_KEYS]
    assert (got.psnr_x, got.ssim_x, got.psnr_masked_x, got.ssim_masked_x) == (v[1], v[2], v[4], v[5])
    assert (got.abse_depth_x, got.rmse_depth_x) == (min(v[6], v[8]), min(v[7], v[9])) and got.lpips_x == got.lpips_masked_x == R.LPIPS


def test_evaluate_metrics_behind_a_real_render():
    """a tiny Graph (fp32, 8 + 8 samples, 16 x 16): evaluate_metrics against the restatement on the same render_by_slices outputs,
    and its psnr against evaluate_psnr"""
    from sparf_amd.renderer import Graph
    from tests.golden.recipe import make_state_dict, ring_cameras, small_opt
    opt = small_opt(nerf=dict(rand_rays=64))
    g = Graph(opt, dev())
    g.nerf.load_state_dict(make_state_dict(opt, 3))
    g.nerf_fine.load_state_dict(make_state_dict(opt, 4))
    H, W, B = 16, 16, 2
    pose, intr = ring_cameras(B, H=H, W=W)
    pose, intr = pose.to(dev()), intr.to(dev())
    rs = np.random.RandomState(7)
    image = D(rs.random_sample((B, 3, H, W)).astype(np.float32))
    mask = D(R.blob(B, H, W)).reshape(B, 1, H, W)
    depth_gt = D((1.5 + 3 * rs.random_sample((B, 1, H, W))).astype(np.float32))
    valid = D(rs.random_sample((B, 1, H, W)) < 0.6)
    kw = dict(H=H, W=W, intr=intr, depth_range=[1.2, 5.2])
    ev = g.evaluate_metrics(opt, pose, image=image, fg_mask=mask, depth_gt=depth_gt, valid_depth_gt=valid, depth_scale=1.37, **kw)
    with torch.no_grad():
        full = g.render_by_slices(opt, pose, iter=None, mode="val", **kw)
    as_image = lambda rgb: rgb.view(B, H, W, 3).permute(0, 3, 1, 2)
    want = metrics.image_metrics_torch(as_image(full.rgb).double(), image.double(), pred_fine=as_image(full.rgb_fine).double(), fg_mask=mask,
                                       depth=full.depth.double(), depth_fine=full.depth_fine.double(), depth_gt=depth_gt.double(), valid_depth_gt=valid,
                                       depth_scale=float(np.float32(1.37)))
    assert set(ev) == set(want) and not any(torch.is_tensor(v) and v.requires_grad for v in ev.values())
    got, w64 = ev.vector.cpu().numpy(), want.vector.cpu().numpy()
    # (the restatement's vector is rounded to float32 after float64 arithmetic: half a spacing of its own on top of the kernel's one)
    assert np.isfinite(w64).all() and np.nanmax(R.spacings(got, w64)) <= R.BOUND + 0.5
    assert torch.equal(ev.counts.cpu(), want.counts.cpu()) and int(ev.n_fg) == int(mask.sum()) and int(ev.n_valid) == int(valid.sum())
    ps = g.evaluate_psnr(opt, pose, image=image, **kw)
    assert abs(float(ev.psnr) - float(ps.psnr)) < 1e-4 and abs(float(ev.psnr_fine) - float(ps.psnr_fine)) < 1e-4
    plain = g.evaluate_metrics(opt, pose, image=image, **kw)
    assert set(plain) == {"vector", "counts", "mse", "psnr", "ssim", "mse_fine", "psnr_fine", "ssim_fine"} and float(plain.ssim) == float(ev.ssim)
