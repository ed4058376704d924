"""The correspondence sampler on the device: select_matches through the compact and gather kernels against the
fixture (tests/golden/matches.npz: what the reference's own chain did), the numpy referee (tests/matches_referee.py) and the torch
restatement on the same device -- bit for bit, there is no tolerance -- at every shape x mask pattern x window of the referee; the forms
of the permutation and the generator's state; the empty cases; determinism; and the installed method behind real renders."""
import contextlib
import types

import numpy as np
import pytest
import torch

from sparf_amd import losses, ops
from tests import matches_referee as R

pytestmark = pytest.mark.gpu
RESULTS = ("pixels_self", "ray_self", "pixels_other", "ray_other", "conf")
DTYPES = (torch.float32, torch.int64, torch.float32, torch.int64, torch.float32)


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def D(a):
    return torch.from_numpy(np.array(a)).to(dev()) if a is not None else None


def N(t):
    return t.detach().cpu().numpy()


def stored(mask, corres, conf):
    """the maps as the reference stores and hands them over: pair 1 of [M,1,H,W] / [M,2,H,W] / [M,1,H,W] tensors (the mask then starts
    H W bytes into its allocation), as the permuted views of sample_valid_image_pair"""
    H, W = mask.shape
    m, c, f = torch.zeros(3, 1, H, W, dtype=torch.bool), torch.full((3, 2, H, W), -7.0), torch.full((3, 1, H, W), -7.0)
    m[1, 0], c[1], f[1] = torch.from_numpy(mask), torch.from_numpy(corres), torch.from_numpy(conf)
    m, c, f = m.to(dev()), c.to(dev()), f.to(dev())
    return m[1].permute(1, 2, 0), c[1].permute(1, 2, 0)[:, :, :2], f[1].permute(1, 2, 0)


@contextlib.contextmanager
def kernel_calls():
    """counts the library calls of the sampler: [compact, gather]"""
    seen = [0, 0]
    real = ops.match_compact, ops.match_gather

    def compact(*a, **k):
        seen[0] += 1
        return real[0](*a, **k)

    def gather(*a, **k):
        seen[1] += int(a[3] > 0)
        return real[1](*a, **k)
    ops.match_compact, ops.match_gather = compact, gather
    try:
        yield seen
    finally:
        ops.match_compact, ops.match_gather = real


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), what


def same_results(a, b, what):
    assert a[5] == b[5], (what, a[5], b[5])
    for key, x, y, dtype in zip(RESULTS, a[:5], b[:5], DTYPES):
        assert x.dtype == y.dtype == dtype and x.shape == y.shape and x.device == y.device, (what, key)
        same_bits(N(x), N(y), (what, key))
    same_bits(N(a[6]), N(b[6]), (what, "perc"))


@pytest.mark.parametrize("name", list(R.FIXTURE_CASES))
def test_fixture_cases(fx, name):
    """what the reference's chain recorded, through the kernels"""
    case = R.fixture_case(fx, name)
    min_nbr = R.FIXTURE_CASES[name][4]
    mask, corres, conf = stored(case["mask"], case["corres"], case["conf"])
    with kernel_calls() as seen:
        out = losses.select_matches(mask, corres, conf, R.MAX_MATCHES, window=case["window"], perm=D(case["perm"]), min_matches=min_nbr)
    if int(case["rendered"]) == 0:
        assert seen == [1, 0] and out[5] < min_nbr and out[0].shape == (0, 2)
        return
    assert seen == [1, 1], "the kernel route was not taken"
    for key, got, ref in zip(RESULTS, out[:5], ("pixels_self", "ray_self", "pixels_other", "ray_other", "conf_values")):
        same_bits(N(got), case[ref], key)
    same_bits(N(out[6]), case["perc"], "perc")


@pytest.mark.parametrize("window", R.WINDOWS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_generated_cases(shape, window):
    """every pattern: the seven results equal the restatement's on the same device and the referee's; the index list is the referee's
    and strictly increasing"""
    H, W = shape
    corres, conf = R.maps_of(H, W)
    win = R.window_of(H, W, window)
    for pattern in R.PATTERNS:
        mask = R.mask_of(H, W, pattern)
        count = int(R.window_mask(mask, win).sum())
        perm = R.perm_of(count)
        want = R.select_np(mask, corres, conf, R.MAX_MATCHES, win, perm)
        m, c, f = stored(mask, corres, conf)
        with kernel_calls() as seen:
            out = losses.select_matches(m, c, f, R.MAX_MATCHES, window=win, perm=D(perm))
        assert seen == [1, int(count > 0)], (pattern, seen)
        same_results(out, losses.select_matches_torch(m, c, f, R.MAX_MATCHES, window=win, perm=D(perm)), pattern)
        assert out[5] == want["count"] == count
        for key, got in zip(RESULTS, out[:5]):
            same_bits(N(got), want[key], (pattern, key))
        same_bits(N(out[6]), want["perc"], (pattern, "perc"))
        index, count_dev, _ = ops.match_compact(m, win, want_perc=False)
        index = N(index)[:int(count_dev.item())]
        same_bits(index, want["index"], (pattern, "index"))
        assert np.all(np.diff(index.astype(np.int64)) > 0)
        # channel-first maps and a plain mask: the same rows
        same_results(out, losses.select_matches(D(mask), D(corres), D(conf), R.MAX_MATCHES, window=win, perm=D(perm)), (pattern, "channel-first"))


def test_perm_forms_and_the_generator():
    H, W = 64, 65
    corres, conf = R.maps_of(H, W)
    m, c, f = stored(R.mask_of(H, W, "bernoulli"), corres, conf)
    count = int(R.mask_of(H, W, "bernoulli").sum())
    # given
    perm = D(R.perm_of(count, 3))
    same_results(losses.select_matches(m, c, f, 100, perm=perm), losses.select_matches_torch(m, c, f, 100, perm=perm), "perm given")
    # none needed: the identity, nothing drawn, a given one ignored
    state = torch.cuda.get_rng_state(dev())
    a = losses.select_matches(m, c, f, count)
    assert torch.equal(torch.cuda.get_rng_state(dev()), state) and a[0].shape == (count, 2)
    same_results(a, losses.select_matches(m, c, f, count + 5, perm=perm), "perm ignored")
    same_results(a, losses.select_matches_torch(m, c, f, count), "identity")
    # drawn: the same seed draws the same matches as the restatement and leaves the generator in the same state
    for seed in (0, 7):
        torch.manual_seed(seed)
        with kernel_calls() as seen:
            a = losses.select_matches(m, c, f, 100)
        state = torch.cuda.get_rng_state(dev())
        torch.manual_seed(seed)
        with losses.unfused(), kernel_calls() as seen_unfused:
            b = losses.select_matches(m, c, f, 100)
        assert seen == [1, 1] and seen_unfused == [0, 0]
        same_results(a, b, ("drawn", seed))
        assert torch.equal(torch.cuda.get_rng_state(dev()), state)
        torch.manual_seed(seed)
        same_bits(N(a[1]), R.select_np(R.mask_of(H, W, "bernoulli"), corres, conf, 100, None, N(torch.randperm(count, device=dev())))["ray_self"],
                  "torch.randperm(count, device)")


def test_empty_cases():
    """legal inputs: an all-false mask, an empty window, max_matches = 0, an image of no pixels"""
    H, W = 16, 16
    corres, conf = R.maps_of(H, W)
    shapes = [(0, 2), (0,), (0, 2), (0,), (0, 1)]
    for mask, window, max_matches in ((R.mask_of(H, W, "none"), None, 10), (R.mask_of(H, W, "all"), R.window_of(H, W, "empty"), 10),
                                      (R.mask_of(H, W, "all"), None, 0)):
        m, c, f = stored(mask, corres, conf)
        with kernel_calls() as seen:
            out = losses.select_matches(m, c, f, max_matches, window=window, perm=torch.arange(H * W, device=dev()))
        assert seen == [1, 0]
        assert [tuple(t.shape) for t in out[:5]] == shapes and tuple(t.dtype for t in out[:5]) == DTYPES and all(t.device == m.device for t in out[:5])
        assert out[5] == (H * W if max_matches == 0 else 0) and float(out[6]) == float(np.float32(out[5]) / np.float32(H * W + 1e-6))
    out = losses.select_matches(torch.zeros(0, 5, dtype=torch.bool, device=dev()), torch.zeros(2, 0, 5, device=dev()), torch.zeros(1, 0, 5, device=dev()), 10)
    assert out[5] == 0 and [tuple(t.shape) for t in out[:5]] == shapes and float(out[6]) == 0.0
    rows = ops.match_gather(torch.zeros(4, dtype=torch.int32, device=dev()), torch.zeros(1, dtype=torch.int32, device=dev()), None, 0, 2, 2,
                            torch.zeros(2, 2, 2, device=dev()), torch.zeros(2, 2, device=dev()))
    assert [tuple(t.shape) for t in rows] == shapes and tuple(t.dtype for t in rows) == DTYPES


def test_two_calls_give_the_same_bits():
    H, W = 96, 128
    m, c, f = stored(R.mask_of(H, W, "bernoulli"), *R.maps_of(H, W))
    perm = D(R.perm_of(int(R.mask_of(H, W, "bernoulli").sum())))
    a = losses.select_matches(m, c, f, 1024, perm=perm)
    b = losses.select_matches(m, c, f, 1024, perm=perm)
    same_results(a, b, "two calls")
    i1, i2 = ops.match_compact(m)[0], ops.match_compact(m)[0]
    assert torch.equal(i1[:a[5]], i2[:a[5]])


def test_installed_method_behind_real_renders():
    """A real Graph at fp32 with 8 + 8 samples and a 16 x 16 scene: compute_loss_on_image_pair on a stand-in, once with the kernels
    and once with ONLY the sampler switched to its restatement, from the same seed.  The selected tensors are identical; both legs then
    run the same renders and the same loss kernel on the same inputs, so the loss and the gradients to the poses and the networks are
    demanded bit for bit."""
    from sparf_amd.edict import EasyDict as edict
    from sparf_amd.renderer import Graph
    from tests.golden.recipe import small_opt
    H = W = 16
    corres, conf = R.maps_of(H, W)
    mask, corres, conf = stored(R.mask_of(H, W, "bernoulli"), corres, conf)
    intr = torch.tensor([[20.0, 0, W / 2], [0, 20.0, H / 2], [0, 0, 1]], device=dev())
    intrs = torch.stack([intr, intr])
    poses0 = torch.tensor([[[1.0, 0, 0, 0.1], [0, 1, 0, 0], [0, 0, 1, 3.0]], [[1.0, 0, 0, -0.1], [0, 1, 0, 0.05], [0, 0, 1, 3.05]]], device=dev())
    image = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(2)).to(dev())

    def run(sampler_restated):
        opt = small_opt(hip=dict(lazy_batch=True), nerf=dict(rand_rays=64))
        torch.manual_seed(0)
        g = Graph(opt, dev())
        g.train()
        poses = poses0.clone().requires_grad_()
        obj = types.SimpleNamespace(net=g, device=dev(), opt=edict(opt))
        obj.opt.update(min_nbr_matches=10, compute_photo_on_matches=False, diff_loss_type="huber", use_gt_correspondences=False,
                       renderrepro_do_pixel_reprojection_check=False, renderrepro_do_depth_reprojection_check=False,
                       renderrepro_pixel_reprojection_thresh=10.0, renderrepro_depth_reprojection_thresh=0.1)
        data = edict(image=image, intr=intrs, poses_w2c=poses, depth_range=torch.tensor([[1.5, 4.5]] * 2, device=dev()), iter=10)
        picked = []
        real = losses.select_matches
        losses.select_matches = lambda *a, **k: (picked.append(real(*a, **k)), picked[-1])[1]
        torch.manual_seed(3)
        try:
            with losses.unfused_sampler() if sampler_restated else contextlib.nullcontext(), kernel_calls() as seen:
                loss_dict, stats, plots = losses.compute_loss_on_image_pair(
                    obj, data, image.permute(0, 2, 3, 1), poses, intrs, 0, 1, corres, None, conf, mask.squeeze(-1), losses._to_4x4(poses[0]),
                    losses._to_4x4(poses[1]), intr, intr, {"corres": torch.zeros((), device=dev())}, {}, {})
        finally:
            losses.select_matches = real
        assert seen == ([0, 0] if sampler_restated else [1, 1])
        assert type(loss_dict["corres"].grad_fn).__name__.startswith("ReprojPairLoss"), "the loss kernel was not taken"
        loss_dict["corres"].backward()
        params = {k: p.grad for k, p in g.named_parameters() if not k.endswith("progress")}
        return dict(loss=loss_dict["corres"].detach(), stats=stats, picked=picked[0], d_poses=poses.grad, params=params)

    a, b = run(False), run(True)
    assert a["picked"][5] > 32 and a["picked"][0].shape == (32, 2)
    same_results(a["picked"], b["picked"], "selected")
    assert set(a["stats"]) == set(b["stats"]) == {"perc_valid_corr_mask", "depth_in_corr_loss"}
    print("loss", float(a["loss"]), float(b["loss"]), "pose gradient max", float(a["d_poses"].abs().max()))
    assert torch.isfinite(a["loss"]) and float(a["loss"]) > 0 and float(a["d_poses"].abs().max()) > 0
    assert torch.equal(a["loss"], b["loss"]) and all(torch.equal(a["stats"][k], b["stats"][k]) for k in a["stats"])
    assert torch.equal(a["d_poses"], b["d_poses"])
    assert a["params"] and all(v is not None and torch.isfinite(v).all() for v in a["params"].values())
    for k, v in a["params"].items():
        assert torch.equal(v, b["params"][k]), k
