"""The depth-consistency front end and the ray sampler on the GPU: the kernels of csrc/pick.hip against the fixture
(tests/golden/pick.npz: what the reference's own functions did) -- pixels, rays and id_other exact, every pose entry within the bound
tests/pick_referee.py derives from the float32 roundings; partial last workgroups, clamped permutation entries, the output-NULL variants,
the same bits from call to call; the installed RaySamplingStrategy.__call__ on the recorded draws; the installed compute_loss around a
real render against the restatements on the same draws; and the copies of the installed front end between entry and the first render."""
import types

import numpy as np
import pytest
import torch

from sparf_amd import losses, ops
from sparf_amd.edict import EasyDict as edict
from tests import pick_referee as R

pytestmark = pytest.mark.gpu
PIXEL_CASES, STRATEGY_CASES = R.pixel_cases(), R.strategy_cases()
DRAWN = [n for n, c in PIXEL_CASES.items() if c["nbr"] is not None]


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(autouse=True)
def nothing_stays_installed():
    yield
    losses.uninstall_depth_consistency_sampler()
    losses.uninstall_ray_sampler()
    losses.uninstall_depth_consistency()


def D(a):
    return torch.from_numpy(np.array(a)).to(dev()) if a is not None else None


def get(fx, key):
    return fx[key] if key in fx.files else None


def same_bits(got, want):
    got = got.detach().cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def pixel_kwargs(case):
    return dict(nbr=case["nbr"], precrop_frac=R.PRECROP, fraction_in_center=case["fraction"], patch_size=case["patch"])


@pytest.mark.parametrize("name", DRAWN)
def test_pixels_and_rays_equal_the_fixture(fx, name):
    """every case, the 300-row and the patch-3 ones among them: their last workgroup is partial"""
    case = PIXEL_CASES[name]
    perm, perm_center = fx[f"{name}/perm"], get(fx, f"{name}/perm_center")
    pixels, rays = losses.sample_pixels(case["H"], case["W"], perm=D(perm), perm_center=D(perm_center), **pixel_kwargs(case))
    assert pixels.is_cuda and rays.is_cuda and same_bits(pixels, fx[f"{name}/pixels"]) and same_bits(rays, fx[f"{name}/rays"])
    # prefixes in host memory travel in one copy; the result is the same
    host = losses.sample_pixels(case["H"], case["W"], perm=torch.from_numpy(perm), perm_center=None if perm_center is None else torch.from_numpy(perm_center),
                                device=dev(), **pixel_kwargs(case))
    assert same_bits(host[0], fx[f"{name}/pixels"]) and same_bits(host[1], fx[f"{name}/rays"])
    # its own draws on the CPU generator, as the reference makes them
    torch.manual_seed(case["seed"])
    own = losses.sample_pixels(case["H"], case["W"], device=dev(), **pixel_kwargs(case))
    assert same_bits(own[0], fx[f"{name}/pixels"]) and same_bits(own[1], fx[f"{name}/rays"])


def test_partial_workgroups_are_among_the_cases(fx):
    rows = {n: fx[f"{n}/rays"].size for n in DRAWN}
    assert rows[f"px_19x21_n{R.BLOCK + 44}_f0.0_pNone"] == R.BLOCK + 44 and rows["px_12x10_n300_f0.0_p3"] == 720 and rows["px_12x10_n300_f0.4_p2"] % R.BLOCK


def test_output_null_variants_and_the_same_bits_from_call_to_call(fx):
    name = "px_12x10_n300_f0.4_p3"
    case = PIXEL_CASES[name]
    args = (D(fx[f"{name}/perm"]), D(fx[f"{name}/perm_center"]), R.pool_of(case), R.centre_box(12, 10), 10, 3)
    both = ops.pick_pixels(*args)
    only_pixels, only_rays = ops.pick_pixels(*args, rays=False), ops.pick_pixels(*args, pixels=False)
    assert only_pixels[1] is None and only_rays[0] is None and torch.equal(only_pixels[0], both[0]) and torch.equal(only_rays[1], both[1])
    assert same_bits(both[0].reshape(-1, 9, 2), fx[f"{name}/pixels"]) and same_bits(both[1].reshape(-1, 9), fx[f"{name}/rays"])
    again = ops.pick_pixels(*args)
    assert torch.equal(again[0], both[0]) and torch.equal(again[1], both[1])
    # one pool alone, either one
    a_only = ops.pick_pixels(args[0], None, args[2], None, 10, 3)
    b_only = ops.pick_pixels(None, args[1], None, args[3], 10, 3)
    n_a = len(fx[f"{name}/perm"]) * 9
    assert torch.equal(a_only[1], both[1][:n_a]) and torch.equal(b_only[1], both[1][n_a:]) and torch.equal(b_only[0], both[0][n_a:])
    empty = ops.pick_pixels(None, None, args[2], args[3], 10, 3, device=dev())
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,)


def test_wild_permutation_entries_are_clamped_into_their_pools():
    """the inputs are valid memory; only the values are wild"""
    H, W, patch = 7, 9, 2
    wild = torch.tensor([-1, 48, torch.iinfo(torch.int64).max, torch.iinfo(torch.int64).min, 5], device=dev())
    pixels, rays = ops.pick_pixels(wild, wild[:3].clone(), (W - 1, H - 1), R.centre_box(H, W), W, patch)
    torch.cuda.synchronize()
    assert float(pixels[:, 0].min()) >= 0 and float(pixels[:, 0].max()) <= W - 1 and float(pixels[:, 1].min()) >= 0 and float(pixels[:, 1].max()) <= H - 1
    assert rays.reshape(-1, 4)[:, 0].tolist() == [0, 5 * W + 7, 5 * W + 7, 0, 5, 2 * W + 2, 3 * W + 5, 3 * W + 5]


@pytest.mark.parametrize("name", R.POSE_CASES)
def test_unseen_pose_against_the_fixture_and_the_referee(fx, name):
    poses, id_self, w = fx[f"{name}/poses_w2c"], int(fx[f"{name}/id_self"]), float(fx[f"{name}/w"])
    got = losses.sample_unseen_pose(D(poses), id_self, w)
    assert got.id_other.is_cuda and got.id_other.dim() == 0 and got.id_other.dtype == torch.int32 and int(got.id_other) == int(fx[f"{name}/id_other"])
    ref = R.referee_pose(poses, id_self, w, int(got.id_other))
    for k in R.POSE_OUTS:
        assert got[k].shape == (4, 4) and got[k].dtype == torch.float32
        ok, ratio = R.within(got[k].cpu().numpy(), *ref[k])
        far = float(np.abs(got[k].cpu().numpy().astype(np.float64) - fx[f"{name}/{k}"]).max())
        print(name, k, "worst |error| / bound", round(ratio, 3), "largest distance to the reference's value", far)
        assert ok, (name, k, ratio)
    assert same_bits(got.pose_w2c_ref, fx[f"{name}/pose_w2c_ref"])
    again = losses.sample_unseen_pose(D(poses), id_self, w)
    assert all(torch.equal(again[k], got[k]) for k in R.POSE_OUTS) and torch.equal(again.id_other, got.id_other)


def test_two_cameras_at_one_centre_give_the_lowest_index():
    poses = R.poses_of(70, 41)
    for twins in ((1, 3), (5, 69), (64, 66)):            # in one lane's stride, across the strides, both in the second stride
        p = poses.copy()
        p[twins[0]] = p[twins[1]] = poses[0]             # the direction of camera 0: the nearest there is
        got = losses.sample_unseen_pose(D(p), 0, 0.25)
        want = losses.sample_unseen_pose_torch(torch.from_numpy(p), 0, 0.25)
        assert int(got.id_other) == int(want.id_other) == twins[0]
    assert int(losses.sample_unseen_pose(D(R.poses_of(1, 42)), 0, 0.5).id_other) == 0


class Replay:
    """torch.randperm answers with the recorded draws, in order and on the device asked for, while it is open"""

    def __init__(self, draws):
        self.draws, self.real = list(draws), torch.randperm

    def __enter__(self):
        def randperm(n, **kw):
            v = self.draws.pop(0)
            assert len(v) == n, (len(v), n)
            return v.to(kw.get("device", "cpu"))
        torch.randperm = randperm
        return self

    def __exit__(self, *exc):
        torch.randperm = self.real


class Sampler:
    """what RaySamplingStrategy.__call__ reads of its instance, for a strategy case"""

    def __init__(self, case, device=None):
        self.opt = edict(sample_fraction_in_fg_mask=0., sampled_fraction_in_center=case["fraction"], precrop_frac=R.PRECROP,
                         depth_regu_patch_size=case["patch"] or 2, loss_weight=edict(depth_patch=None if case["patch"] is None else 1.0))
        self.device, self.nbr_images, self.H, self.W = dev() if device is None else device, case["B"], case["H"], case["W"]
        a_w, a_h = R.strategy_pool(case)
        box = R.centre_box(case["H"], case["W"])
        self.all_possible_pixels = torch.zeros(a_w * a_h, 2, dtype=torch.long, device=dev())
        self.all_center_pixels = torch.zeros(box[2] * box[3], 2, dtype=torch.long, device=dev())

    def __call__(self, *a, **k):
        raise AssertionError("handed to the original")


@pytest.mark.parametrize("name", STRATEGY_CASES)
def test_installed_ray_sampler_equals_the_fixture(fx, name):
    case = STRATEGY_CASES[name]
    module = types.SimpleNamespace(RaySamplingStrategy=type("RaySamplingStrategy", (Sampler,), {}))
    losses.install_ray_sampler(module)
    draws = [torch.from_numpy(fx[f"{name}/draw{i}"]) for i in range(2) if f"{name}/draw{i}" in fx.files]
    with Replay(draws) as tape:
        rays = module.RaySamplingStrategy(case)(case["nbr_pixels"], sample_in_center=case["in_center"], idx_imgs=case["idx_imgs"])
    assert not tape.draws and rays.is_cuda and same_bits(rays, fx[f"{name}/rays"])


# ---- the installed front end around a real render
H, W, B = 40, 60, 3


def scene():
    intr = torch.tensor([[50.0, 0, W / 2], [0, 50.0, H / 2], [0, 0, 1]], device=dev()).repeat(B, 1, 1)
    poses = torch.eye(4, device=dev())[:3].repeat(B, 1, 1)
    poses[:, :, 3] = torch.tensor([[0.1 - 0.1 * b, 0.02 * b, 3.0 + 0.02 * b] for b in range(B)], device=dev())
    return edict(image=torch.zeros(B, 3, H, W, device=dev()), poses_w2c=poses, intr=intr, depth_range=torch.tensor([[1.5, 4.5]] * B, device=dev()), iter=10)


def loss_object(graph, opt):
    """an object with what DepthConsistencyLoss holds, its core method the package's (install_depth_consistency) and its front end installed"""
    module = types.SimpleNamespace(DepthConsistencyLoss=type("Theirs", (), {}))
    losses.install_depth_consistency(module)
    losses.install_depth_consistency_sampler(module)
    obj = module.DepthConsistencyLoss()
    obj.net, obj.device = graph, dev()
    obj.opt = edict(opt)
    obj.opt.update(diff_loss_type="huber", gradually_decrease_depth_cons_loss=False, depth_cons_loss_reduct_at_x_iter=5, sampled_fraction_in_center=0.4,
                   start_ratio=edict(depth_cons=None), start_iter=edict(depth_cons=0), max_iter=100)
    return obj


def test_installed_compute_loss_around_a_real_render():
    """The installed compute_loss on a tiny Graph against the restatements on the same draws: the pixels into the first render are
    identical; the loss agrees within the bound tests/test_dcons_gpu.py holds its own kernels to behind real renders (1e-3 of the loss:
    the unseen pose differs from torch's in its last bits, and so do the projected pixels that are rendered)."""
    from sparf_amd.renderer import Graph
    from tests.golden.recipe import small_opt
    opt = small_opt(hip=dict(lazy_batch=True))
    torch.manual_seed(0)
    g = Graph(opt, dev())
    g.train()
    obj = loss_object(g, opt)
    data = scene()
    seen = []
    render = g.render_image_at_specific_pose_and_rays
    g.render_image_at_specific_pose_and_rays = lambda *a, **k: (seen.append(k["pixels"].detach().clone()), render(*a, **k))[1]

    def seeded():
        np.random.seed(5)
        torch.manual_seed(5)
    seeded()
    loss, stats, _ = obj.compute_loss(obj.opt, data, {}, 10, mode="train")
    value = float(loss["depth_cons"].detach())
    assert np.isfinite(value) and value > 0 and stats["nbr_px_sampling"] == 1024 and len(seen) == 2
    loss["depth_cons"].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for k, p in g.named_parameters() if not k.endswith("progress"))
    # by hand on the same draws: randint, the two permutations, the render, rand -- everything in front of the renders in torch
    seeded()
    id_self = np.random.randint(B)
    pixels, _ = losses.sample_pixels_torch(H, W, nbr=1024, fraction_in_center=0.4, device=dev())
    assert torch.equal(seen[0], pixels)
    ret = render(obj.opt, data, pose=data.poses_w2c[id_self], intr=data.intr[id_self], H=H, W=W, pixels=pixels, mode="train", iter=10)
    prep = losses.sample_unseen_pose_torch(data.poses_w2c, id_self, np.random.rand())
    points = losses.backproject_to_3d_torch(pixels, ret.depth_fine.squeeze(0).squeeze(-1), data.intr[id_self], prep.pose_c2w_ref)
    want, _, _ = obj.compute_loss_at_sampled_pose(data, prep.pose_w2c_at_unseen, data.intr[id_self].clone(), points, H, W, pixels)
    by_hand = float(want["depth_cons"].detach())
    print("installed", value, "by hand", by_hand)
    assert abs(value - by_hand) <= 1e-3 * by_hand


class Stop(Exception):
    pass


class StopAtTheFirstRender:
    def render_image_at_specific_pose_and_rays(self, *a, **k):
        raise Stop


def test_front_end_copies_between_entry_and_the_first_render():
    """no device-to-host copy, and exactly one host-to-device copy -- the permutation prefix -- from the entry of the installed
    compute_loss to its first render; the call behind the render (the unseen pose) copies nothing either way"""
    from torch.profiler import ProfilerActivity, profile
    obj = loss_object(StopAtTheFirstRender(), edict(nerf=edict(rand_rays=2048)))
    data = scene()

    def front():
        with pytest.raises(Stop):
            obj.compute_loss(obj.opt, data, {}, 10, mode="train")
        return losses.sample_unseen_pose(data.poses_w2c, 1, 0.3)
    front()                                                                   # (the first call loads the kernels)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with pytest.raises(Stop):
            obj.compute_loss(obj.opt, data, {}, 10, mode="train")
        torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof_pose:
        losses.sample_unseen_pose(data.poses_w2c, 1, 0.3)
        torch.cuda.synchronize()

    def device_events(p):
        names = [e.name for e in p.events() if str(e.device_type).endswith("CUDA")]
        copies = [x for x in names if x.lower().startswith("memcpy")]
        return names, copies
    names, copies = device_events(prof)
    print("entry to the first render:", names)
    assert sum("HtoD" in x for x in copies) == 1 and not any("DtoH" in x for x in copies), copies
    assert len(names) - len(copies) == 1                                      # one kernel: the pixels
    host = [e.name for e in prof.events() if not str(e.device_type).endswith("CUDA")]
    assert not any(x in ("aten::nonzero", "aten::_local_scalar_dense", "aten::item") for x in host)
    names, copies = device_events(prof_pose)
    print("the unseen pose:", names)
    assert not copies and len(names) == 1


# ---- the device as the reference trainer holds it: the string 'cuda', without an index (base_trainer.py:109)
DEVICE_FORMS = {"string": lambda: "cuda", "bare": lambda: torch.device("cuda"), "indexed string": lambda: "cuda:0"}


@pytest.mark.parametrize("form", DEVICE_FORMS)
@pytest.mark.parametrize("name", ["st_12x10_f0.4_p3_c0", "st_7x9_f0.4_pNone_c1", "st_12x10_f0.0_p2_c0"])
def test_installed_ray_sampler_with_a_device_without_an_index(fx, name, form):
    case = STRATEGY_CASES[name]
    module = types.SimpleNamespace(RaySamplingStrategy=type("RaySamplingStrategy", (Sampler,), {}))
    losses.install_ray_sampler(module)
    draws = [torch.from_numpy(fx[f"{name}/draw{i}"]) for i in range(2) if f"{name}/draw{i}" in fx.files]
    with Replay(draws) as tape:
        rays = module.RaySamplingStrategy(case, DEVICE_FORMS[form]())(case["nbr_pixels"], sample_in_center=case["in_center"], idx_imgs=case["idx_imgs"])
    assert not tape.draws and rays.is_cuda and same_bits(rays, fx[f"{name}/rays"])
    # with torch's own draws on that device, as the trainer makes them
    rays = module.RaySamplingStrategy(case, DEVICE_FORMS[form]())(case["nbr_pixels"], sample_in_center=case["in_center"], idx_imgs=case["idx_imgs"])
    assert rays.is_cuda and rays.shape == fx[f"{name}/rays"].shape


class PlaneNet:
    """the two render methods DepthConsistencyLoss calls: a plane at depth 3 in front of every camera, half visible"""

    def render_image_at_specific_pose_and_rays(self, opt, data_dict, pose, intr, H, W, pixels=None, mode=None, iter=None):
        n = pixels.shape[0]
        return edict(depth=torch.full((1, n, 1), 3.0, device=dev(), requires_grad=True), opacity=torch.full((1, n, 1), 0.9, device=dev()))

    def render_up_to_maxdepth_at_specific_pose_and_rays(self, opt, data_dict, pose, intr, H, W, depth_max=None, pixels=None, mode=None, iter=None):
        return edict(all_cumulated=torch.full((1, pixels.shape[0]), 0.5, device=dev()))


def test_installed_compute_loss_with_a_device_without_an_index():
    """the installed compute_loss and compute_loss_from_existing_pixels of a loss whose `device` is 'cuda' or torch.device('cuda'):
    the same pixels, the same unseen pose and the same loss as with cuda:0, from the kernels (poses that want a gradient included)"""
    data = scene()
    data.poses_w2c = data.poses_w2c.clone().requires_grad_(True)         # joint pose training: detached on the way in, as the reference does
    seen = {}

    def run(device):
        obj = loss_object(PlaneNet(), edict(nerf=edict(rand_rays=2048)))
        obj.device = device
        core, kept = obj.compute_loss_at_sampled_pose, []
        obj.compute_loss_at_sampled_pose = lambda d, **kw: (kept.append(kw), core(d, **kw))[1]
        calls = []
        real = ops.L.call
        ops.L.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        try:
            np.random.seed(9)
            torch.manual_seed(9)
            loss = obj.compute_loss(obj.opt, data, {}, 10, mode="train")[0]["depth_cons"]
            np.random.seed(9)
            existing = obj.compute_loss_from_existing_pixels(obj.opt, data, 10, kept[0]["pixels_in_ref"][:33], 1, torch.full((33,), 3.0, device=dev()))
        finally:
            ops.L.call = real
            losses.uninstall_depth_consistency_sampler()
            losses.uninstall_depth_consistency()
        assert calls.count("sparf_pick_pixels") == 1 and calls.count("sparf_unseen_pose") == 2
        return loss.detach(), existing[0]["depth_cons"].detach(), kept[0]["pixels_in_ref"], kept[0]["pose_w2c_at_unseen"], kept[1]["pose_w2c_at_unseen"]
    want = run(dev())
    assert want[2].shape == (1229 + 600, 2) and float(want[0]) > 0       # 2048 - int(2048 * 0.4) picks of the pool, the whole centre box of 20 x 30
    for form, make in DEVICE_FORMS.items():
        got = run(make())
        assert all(torch.equal(a, b) for a, b in zip(got, want)), form


def test_prefixes_on_the_device_are_used_where_they_are():
    perm = torch.arange(5, device=dev())
    for form, make in DEVICE_FORMS.items():
        assert losses._prefixes_to(ops._resolve(make()), perm, None)[0] is perm
        pixels, rays = losses.sample_pixels(7, 9, nbr=5, perm=perm, device=make())
        assert rays.tolist() == [0, 1, 2, 3, 4] and pixels.device == perm.device
        assert ops.pick_pixels(perm, None, (8, 6), None, 9, device=make())[1].tolist() == [0, 1, 2, 3, 4]
