"""The depth-consistency front end and the ray sampler without a GPU: the torch restatements of sparf_amd.losses
against the fixture (tests/golden/pick.npz: what the reference's own sample_rays, sample_rays_for_patch, RaySamplingStrategy.__call__ and
DepthConsistencyLoss.sample_pose did); csrc/pick.h built for the host over every fixture case -- pixels, rays and id_other exact, every
pose entry within the bound tests/pick_referee.py derives; the argument checks of both ops wrappers and of both entry points; what the
glue hands the library, over a stand-in that records calls (tests/pick_fake.py); both installs; where the reference tree is present, the
generators after the reference's compute_loss and after the installed one; and build.py's lists."""
import ctypes
import types

import numpy as np
import pytest
import torch

from sparf_amd import build as BUILD, lib as L, losses, ops
from sparf_amd.edict import EasyDict as edict
from tests import pick_fake, pick_referee as R, ref_harness

PIXEL_CASES, STRATEGY_CASES = R.pixel_cases(), R.strategy_cases()


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return pick_fake.build_host(tmp_path_factory.mktemp("pick_host"))


@pytest.fixture
def fake():
    with pick_fake.installed() as lib:
        yield lib


@pytest.fixture
def fake_host(host):
    with pick_fake.installed(host) as lib:
        yield lib


@pytest.fixture(autouse=True)
def nothing_stays_installed():
    yield
    losses.uninstall_depth_consistency_sampler()
    losses.uninstall_ray_sampler()
    losses.uninstall_depth_consistency()


def T(a):
    return None if a is None else torch.from_numpy(np.array(a))


def get(fx, key):
    return fx[key] if key in fx.files else None


def same_bits(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def pixel_kwargs(case):
    return dict(nbr=case["nbr"], precrop_frac=R.PRECROP, fraction_in_center=case["fraction"], patch_size=case["patch"])


def test_the_fixture_holds_every_case(fx):
    names = {k.split("/")[0] for k in fx.files}
    assert names == set(PIXEL_CASES) | set(STRATEGY_CASES) | set(R.POSE_CASES)
    # what the issue asks of the cases: two images that are not square, more rows than one workgroup, a pose set as [B,3,4]
    assert fx[f"px_19x21_n{R.BLOCK + 44}_f0.0_pNone/rays"].shape == (R.BLOCK + 44,) and fx["px_12x10_n300_f0.0_p3/rays"].shape == (80, 9)
    assert fx["st_12x10_f0.4_p3_c0/rays"].shape[0] > R.BLOCK and fx["pose_b3_3x4/poses_w2c"].shape == (3, 3, 4)
    for name, (B, id_self, three, seed) in R.POSE_CASES.items():
        assert same_bits(R.poses_of(B, seed, three), fx[f"{name}/poses_w2c"]) and int(fx[f"{name}/id_self"]) == id_self
        # the smallest and the second-smallest distance lie apart: the first-index rule decides no fixture case
        assert R.gap(R.centres32(fx[f"{name}/poses_w2c"]), id_self) >= R.MIN_GAP
        d = R.angular_dists(R.centres32(fx[f"{name}/poses_w2c"]), id_self)
        assert int(np.argmin(d)) == int(fx[f"{name}/id_other"])


# ---- the restatements against the fixture
@pytest.mark.parametrize("name", PIXEL_CASES)
def test_pixel_restatement_reproduces_the_fixture(fx, name):
    case = PIXEL_CASES[name]
    perm, perm_center = T(get(fx, f"{name}/perm")), T(get(fx, f"{name}/perm_center"))
    for fn in (losses.sample_pixels_torch, losses.sample_pixels):            # CPU tensors: the public function is the restatement
        pixels, rays = fn(case["H"], case["W"], perm=perm, perm_center=perm_center, **pixel_kwargs(case))
        assert same_bits(pixels, fx[f"{name}/pixels"]) and same_bits(rays, fx[f"{name}/rays"]), name
    # its own draws are the reference's: the same generator, the same calls in the same order
    torch.manual_seed(case["seed"])
    pixels, rays = losses.sample_pixels(case["H"], case["W"], **pixel_kwargs(case))
    assert same_bits(pixels, fx[f"{name}/pixels"]) and same_bits(rays, fx[f"{name}/rays"]), name


@pytest.mark.parametrize("name", R.POSE_CASES)
def test_pose_restatement_reproduces_the_fixture(fx, name):
    """the reference's operations in the reference's order on the CPU: the same bits"""
    got = losses.sample_unseen_pose_torch(T(fx[f"{name}/poses_w2c"]), int(fx[f"{name}/id_self"]), float(fx[f"{name}/w"]))
    assert set(got) == set(R.POSE_OUTS) | {"id_other"}
    assert got.id_other.dim() == 0 and got.id_other.dtype == torch.int32 and int(got.id_other) == int(fx[f"{name}/id_other"])
    for k in R.POSE_OUTS:
        assert same_bits(got[k], fx[f"{name}/{k}"]), (name, k)
    pub = losses.sample_unseen_pose(T(fx[f"{name}/poses_w2c"]), int(fx[f"{name}/id_self"]), float(fx[f"{name}/w"]))
    assert all(same_bits(pub[k], fx[f"{name}/{k}"]) for k in R.POSE_OUTS)


@pytest.mark.parametrize("name", R.POSE_CASES)
def test_the_reference_lies_within_the_referees_bound(fx, name):
    ref = R.referee_pose(fx[f"{name}/poses_w2c"], int(fx[f"{name}/id_self"]), float(fx[f"{name}/w"]), int(fx[f"{name}/id_other"]))
    for k, (want, bound) in ref.items():
        ok, ratio = R.within(fx[f"{name}/{k}"], want, bound)
        print(name, k, "worst |error| / bound of the reference", round(ratio, 3))
        assert ok, (name, k, ratio)


# ---- csrc/pick.h as host C++
def host_pixels(host, perm_a, perm_b, pool_a, pool_b, W, patch):
    pa, pb = (np.ascontiguousarray(p, dtype=np.int64) if p is not None else np.zeros(0, dtype=np.int64) for p in (perm_a, perm_b))
    rows = (len(pa) + len(pb)) * patch * patch
    pixels, rays = np.full((rows, 2), -7, dtype=np.float32), np.full(rows, -7, dtype=np.int64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None
    assert host.host_pick_pixels(p(pa), len(pa), p(pb), len(pb), *pool_a, *pool_b, W, patch, p(pixels), p(rays)) == 0
    return pixels, rays


@pytest.mark.parametrize("name", [n for n, c in PIXEL_CASES.items() if c["nbr"] is not None])
def test_host_build_of_pick_h_reproduces_the_pixel_cases(fx, host, name):
    case = PIXEL_CASES[name]
    patch = case["patch"] or 1
    pixels, rays = host_pixels(host, fx[f"{name}/perm"], get(fx, f"{name}/perm_center"), R.pool_of(case), R.centre_box(case["H"], case["W"]), case["W"], patch)
    assert same_bits(pixels.reshape(fx[f"{name}/pixels"].shape), fx[f"{name}/pixels"]) and same_bits(rays.reshape(fx[f"{name}/rays"].shape), fx[f"{name}/rays"])


def host_pose(host, poses, id_self, w):
    poses = np.ascontiguousarray(poses, dtype=np.float32)
    out, id_other = np.full((4, 4, 4), np.nan, dtype=np.float32), np.full(1, -1, dtype=np.int32)
    p = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)
    assert host.host_unseen_pose(p(poses), poses.shape[1] * 4, len(poses), id_self, w, 1.0 - w, p(out), p(out, 64), p(out, 128), p(out, 192), p(id_other)) == 0
    return out, int(id_other[0])


@pytest.mark.parametrize("name", R.POSE_CASES)
def test_host_build_of_pick_h_against_the_referee(fx, host, name):
    poses, id_self, w = fx[f"{name}/poses_w2c"], int(fx[f"{name}/id_self"]), float(fx[f"{name}/w"])
    out, id_other = host_pose(host, poses, id_self, w)
    assert id_other == int(fx[f"{name}/id_other"])
    for k, (want, bound) in zip(R.POSE_OUTS, (R.referee_pose(poses, id_self, w, id_other)[k] for k in R.POSE_OUTS)):
        ok, ratio = R.within(out[R.POSE_OUTS.index(k)], want, bound)
        print(name, k, "worst |error| / bound", round(ratio, 3))
        assert ok, (name, k, ratio)
    assert same_bits(out[0], fx[f"{name}/pose_w2c_ref"])


def test_two_cameras_at_one_centre_give_the_lowest_index(host):
    """numpy's argsort leaves ties to the implementation; here the first index of the minimum is the rule, on both routes"""
    poses = R.poses_of(5, 41)
    for id_self in (0, 2, 4):
        twins = poses.copy()
        twins[1] = twins[3] = poses[id_self]             # both where camera id_self is: the nearest there is, and equally near
        d = R.angular_dists(R.centres32(twins), id_self)
        assert d[1] == d[3] == d.min()
        got = losses.sample_unseen_pose_torch(T(twins), id_self, 0.25)
        assert int(got.id_other) == 1 and host_pose(host, twins, id_self, 0.25)[1] == 1
    one = R.poses_of(1, 42)
    assert int(losses.sample_unseen_pose_torch(T(one), 0, 0.5).id_other) == 0 and host_pose(host, one, 0, 0.5)[1] == 0


def test_host_build_clamps_wild_permutation_entries(host):
    H, W, patch = 7, 9, 2
    wild = np.array([-1, 48, np.iinfo(np.int64).max, np.iinfo(np.int64).min, 5], dtype=np.int64)
    pixels, rays = host_pixels(host, wild, wild[:3], (W - 1, H - 1), R.centre_box(H, W), W, patch)
    assert pixels[:, 0].min() >= 0 and pixels[:, 0].max() <= W - 1 and pixels[:, 1].min() >= 0 and pixels[:, 1].max() <= H - 1
    assert rays.reshape(-1, 4)[:, 0].tolist() == [0, 5 * W + 7, 5 * W + 7, 0, 5, 2 * W + 2, 3 * W + 5, 3 * W + 5]


# ---- the entry points' argument checks: every one returns before a launch
PIX_ARGS = dict(perm_a=1, n_a=5, perm_b=1, n_b=3, a_w=8, a_h=6, b_x0=2, b_y0=2, b_w=4, b_h=2, W=9, patch=1, pixels=1, rays=1)
PIX_MALFORMED = {
    "negative n_a": dict(n_a=-1), "negative n_b": dict(n_b=-1), "no width": dict(W=0), "patch 0": dict(patch=0), "patch 1025": dict(patch=1025),
    "rows above 2^30": dict(n_a=1 << 29, n_b=(1 << 29) + 1), "no perm_a": dict(perm_a=None), "no perm_b": dict(perm_b=None), "empty pool A": dict(a_w=0),
    "pool A of no height": dict(a_h=0), "negative pool B": dict(b_w=-4), "negative origin": dict(b_x0=-1), "pool A wider than the image": dict(a_w=10),
    "pool A plus the patch wider than the image": dict(patch=3), "pool B past the image": dict(b_x0=6), "pool above 2^30": dict(a_w=9, a_h=1 << 28, W=1 << 20),
}
POSE_ARGS = dict(poses_w2c=1, row_floats=12, B=3, id_self=1, w=0.25, one_minus_w=0.75, pose_w2c_ref=1, pose_c2w_ref=1, pose_c2w_other=1,
                 pose_w2c_at_unseen=1, id_other=1)
POSE_MALFORMED = {
    "row_floats 9": dict(row_floats=9), "no pose": dict(B=0), "negative B": dict(B=-2), "B above 2^20": dict(B=(1 << 20) + 1), "id_self -1": dict(id_self=-1),
    "id_self B": dict(id_self=3), **{f"no {k}": {k: None} for k in ("poses_w2c", "pose_w2c_ref", "pose_c2w_ref", "pose_c2w_other", "pose_w2c_at_unseen", "id_other")},
}


def entry(name, defaults, **kw):
    assert tuple(defaults) == pick_fake.CALLS[name] and set(kw) <= set(defaults)
    buf = np.zeros(64, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)         # host memory: never dereferenced, every call here returns before a launch
    pointers = {k for k, t in zip(defaults, L.EXPORTS[name][1]) if t is ctypes.c_void_p}
    args = [(p if v is not None else None) if k in pointers else v for k, v in dict(defaults, **kw).items()]
    return getattr(L.load(), name)(*args, None)


@pytest.mark.parametrize("name", PIX_MALFORMED)
def test_malformed_pixel_calls_return_1_without_a_device(name):
    assert entry("sparf_pick_pixels", PIX_ARGS, **PIX_MALFORMED[name]) == 1


@pytest.mark.parametrize("name", POSE_MALFORMED)
def test_malformed_pose_calls_return_1_without_a_device(name):
    assert entry("sparf_unseen_pose", POSE_ARGS, **POSE_MALFORMED[name]) == 1


def test_nothing_to_write_is_no_launch():
    assert entry("sparf_pick_pixels", PIX_ARGS, n_a=0, n_b=0, perm_a=None, perm_b=None) == 0
    assert entry("sparf_pick_pixels", PIX_ARGS, pixels=None, rays=None) == 0
    assert L.ABI_VERSION == 7 and L.load().sparf_abi_version() == 7


# ---- the ops wrappers over the recording stand-in
def test_pick_pixels_hands_over_pools_counts_and_outputs(fake):
    pa, pb = torch.arange(5), torch.arange(3)
    pixels, rays = ops.pick_pixels(pa, pb, (8, 6), (2, 2, 4, 2), 9, 2)
    assert fake.names() == ["sparf_pick_pixels"]
    rec, raw = fake.calls[0][1], fake.raw[0][1]
    assert rec == dict(perm_a=True, n_a=5, perm_b=True, n_b=3, a_w=8, a_h=6, b_x0=2, b_y0=2, b_w=4, b_h=2, W=9, patch=2, pixels=True, rays=True)
    assert raw["perm_a"] == pa.data_ptr() and raw["perm_b"] == pb.data_ptr() and raw["pixels"] == pixels.data_ptr() and raw["rays"] == rays.data_ptr()
    assert pixels.shape == (32, 2) and pixels.dtype == torch.float32 and rays.shape == (32,) and rays.dtype == torch.int64
    # output-NULL variants, an empty prefix, and no row at all
    assert ops.pick_pixels(pa, None, (8, 6), None, 9, pixels=False)[0] is None and fake.calls[1][1]["pixels"] is False and fake.calls[1][1]["perm_b"] is False
    assert ops.pick_pixels(pa, pb[:0], (8, 6), (2, 2, 4, 2), 9, rays=False)[1] is None and fake.calls[2][1]["rays"] is False and fake.calls[2][1]["n_b"] == 0
    px, ry = ops.pick_pixels(None, None, (8, 6), None, 9, device="cpu")
    assert px.shape == (0, 2) and ry.shape == (0,) and len(fake.calls) == 3
    assert ops.pick_pixels(pa, None, (8, 6), None, 9, pixels=False, rays=False) == (None, None) and len(fake.calls) == 3


@pytest.mark.parametrize("kw, text", [
    (dict(perm_a=torch.arange(5, dtype=torch.int32)), "perm_a must be int64"), (dict(perm_b=torch.arange(6).reshape(2, 3)), "perm_b must be int64"),
    (dict(W=0), "W must be positive"), (dict(patch=0), "patch in"), (dict(pool_a=(0, 6)), "pool A"), (dict(pool_a=(10, 6)), "pool A"), (dict(patch=3), "pool A"),
    (dict(pool_b=(6, 2, 4, 2)), "pool B"), (dict(pool_b=(-1, 2, 4, 2)), "pool B"), (dict(perm_a=None, perm_b=None), "no permutation and no device"),
])
def test_pick_pixels_argument_checks(fake, kw, text):
    args = dict(perm_a=torch.arange(5), perm_b=torch.arange(3), pool_a=(8, 6), pool_b=(2, 2, 4, 2), W=9, patch=1)
    args.update(kw)
    with pytest.raises(ValueError, match=text):
        ops.pick_pixels(**args)
    assert not fake.calls


def test_unseen_pose_hands_over_the_scalars_and_one_output_block(fake):
    poses = T(R.poses_of(6, 3))
    out, id_other = ops.unseen_pose(poses, 4, 0.3)
    rec, raw = fake.calls[0][1], fake.raw[0][1]
    assert fake.names() == ["sparf_unseen_pose"] and rec["row_floats"] == 16 and rec["B"] == 6 and rec["id_self"] == 4
    # 1 - w is taken in double; ctypes rounds each of the two to float32 once (the recorder sees them before that)
    assert rec["w"] == 0.3 and rec["one_minus_w"] == 1.0 - 0.3
    assert raw["poses_w2c"] == poses.data_ptr() and [raw[k] for k in pick_fake.POSE_OUTS] == [out.data_ptr() + 64 * k for k in range(4)]
    assert out.shape == (4, 4, 4) and [float(out[k, 0, 0]) for k in range(4)] == [1.0, 2.0, 3.0, 4.0]
    assert id_other.dtype == torch.int32 and id_other.tolist() == [pick_fake.ID_OTHER]
    ops.unseen_pose(poses[:, :3], 0, 0.5)
    assert fake.calls[1][1]["row_floats"] == 12
    sliced = torch.cat([poses, poses], dim=1)[:, :4]                        # not dense: copied, the values unchanged
    ops.unseen_pose(sliced, 0, 0.5)
    assert fake.raw[2][1]["poses_w2c"] != sliced.data_ptr()


@pytest.mark.parametrize("poses, id_self, text", [
    (torch.zeros(3, 4, 4, dtype=torch.float64), 0, "float32"), (torch.zeros(3, 2, 4), 0, r"\[B,3,4\]"), (torch.zeros(4, 4), 0, r"\[B,3,4\]"),
    (torch.zeros(0, 4, 4), 0, "at least one pose"), (torch.zeros(3, 4, 4), 3, "id_self 3"), (torch.zeros(3, 4, 4), -1, "id_self -1"),
])
def test_unseen_pose_argument_checks(fake, poses, id_self, text):
    with pytest.raises(ValueError, match=text):
        ops.unseen_pose(poses, id_self, 0.5)
    assert not fake.calls


# ---- the public functions over the stand-in that answers with pick.h
@pytest.mark.parametrize("name", [n for n, c in PIXEL_CASES.items() if c["nbr"] is not None])
def test_sample_pixels_through_the_library_route(fx, fake_host, name):
    case = PIXEL_CASES[name]
    torch.manual_seed(case["seed"])                                           # its own draws, as the reference makes them
    pixels, rays = losses.sample_pixels(case["H"], case["W"], device="cpu", **pixel_kwargs(case))
    assert fake_host.names() == ["sparf_pick_pixels"]
    assert same_bits(pixels, fx[f"{name}/pixels"]) and same_bits(rays, fx[f"{name}/rays"])
    rec = fake_host.calls[0][1]
    assert (rec["a_w"], rec["a_h"]) == R.pool_of(case) and rec["patch"] == (case["patch"] or 1)
    assert rec["n_a"] == len(fx[f"{name}/perm"]) and rec["n_b"] == (len(fx[f"{name}/perm_center"]) if case["fraction"] > 0 else 0)
    given = losses.sample_pixels(case["H"], case["W"], perm=T(fx[f"{name}/perm"]), perm_center=T(get(fx, f"{name}/perm_center")), **pixel_kwargs(case))
    assert same_bits(given[0], fx[f"{name}/pixels"]) and same_bits(given[1], fx[f"{name}/rays"])


def test_sample_pixels_routes_to_the_restatement(fx, fake_host):
    name = "px_7x9_nNone_f0.4_p2"                                             # nothing is drawn: the whole pool, no centre pick
    state = torch.get_rng_state()
    pixels, rays = losses.sample_pixels(7, 9, device="cpu", **pixel_kwargs(PIXEL_CASES[name]))
    assert same_bits(pixels, fx[f"{name}/pixels"]) and same_bits(rays, fx[f"{name}/rays"]) and torch.equal(state, torch.get_rng_state())
    with losses.unfused():
        losses.sample_pixels(7, 9, nbr=5, device="cpu")
    losses.sample_pixels(7, 9, nbr=5, perm=torch.arange(5, dtype=torch.int32))                     # a foreign dtype
    losses.sample_pixels(12, 10, nbr=5, precrop_frac=1.0, fraction_in_center=0.4, patch_size=3)   # the centre box's patches leave the image
    assert not fake_host.calls


@pytest.mark.parametrize("name", R.POSE_CASES)
def test_sample_unseen_pose_through_the_library_route(fx, fake_host, name):
    poses, id_self, w = T(fx[f"{name}/poses_w2c"]), int(fx[f"{name}/id_self"]), float(fx[f"{name}/w"])
    got = losses.sample_unseen_pose(poses, id_self, w)
    assert fake_host.names() == ["sparf_unseen_pose"] and got.id_other.dim() == 0 and int(got.id_other) == int(fx[f"{name}/id_other"])
    ref = R.referee_pose(fx[f"{name}/poses_w2c"], id_self, w, int(got.id_other))
    assert all(R.within(got[k].numpy(), *ref[k])[0] and got[k].shape == (4, 4) for k in R.POSE_OUTS)
    # a gradient asked of the poses, another dtype and unfused() go to the restatement
    for p in (poses.clone().requires_grad_(True), poses.double()):
        losses.sample_unseen_pose(p, id_self, w)
    with losses.unfused():
        losses.sample_unseen_pose(poses, id_self, w)
    assert len(fake_host.calls) == 1


# ---- the installs
def strategy_opt(case, mask_fraction=0.):
    return edict(sample_fraction_in_fg_mask=mask_fraction, sampled_fraction_in_center=case["fraction"], precrop_frac=R.PRECROP,
                 depth_regu_patch_size=case["patch"] or 2, loss_weight=edict(depth_patch=None if case["patch"] is None else 1.0))


class Sampler:
    """what RaySamplingStrategy.__call__ reads of its instance, for a case: the original method returns a mark"""

    def __init__(self, case, mask_fraction=0.):
        self.opt, self.device, self.nbr_images, self.H, self.W = strategy_opt(case, mask_fraction), torch.device("cpu"), case["B"], case["H"], case["W"]
        a_w, a_h = R.strategy_pool(case)
        box = R.centre_box(case["H"], case["W"])
        self.all_possible_pixels, self.all_center_pixels = torch.zeros(a_w * a_h, 2, dtype=torch.long), torch.zeros(box[2] * box[3], 2, dtype=torch.long)

    def __call__(self, nbr_pixels, sample_in_center=False, idx_imgs=None):
        return ("original", nbr_pixels, sample_in_center, idx_imgs)


class Replay:
    """torch.randperm answers with the recorded draws, in order, while it is open"""

    def __init__(self, draws):
        self.draws, self.real = list(draws), torch.randperm

    def __enter__(self):
        def randperm(n, **kw):
            v = self.draws.pop(0)
            assert len(v) == n, (len(v), n)
            return v.clone()
        torch.randperm = randperm
        return self

    def __exit__(self, *exc):
        torch.randperm = self.real


def draws_of(fx, name):
    return [T(fx[f"{name}/draw{i}"]) for i in range(2) if f"{name}/draw{i}" in fx.files]


@pytest.mark.parametrize("name", STRATEGY_CASES)
def test_installed_ray_sampler_reproduces_the_fixture(fx, fake_host, name):
    case = STRATEGY_CASES[name]
    module = types.SimpleNamespace(RaySamplingStrategy=type("RaySamplingStrategy", (Sampler,), {}))
    losses.install_ray_sampler(module)
    try:
        with Replay(draws_of(fx, name)) as tape:
            rays = module.RaySamplingStrategy(case)(case["nbr_pixels"], sample_in_center=case["in_center"], idx_imgs=case["idx_imgs"])
        assert not tape.draws                                                 # as many draws as the reference made, of the same pools
    finally:
        losses.uninstall_ray_sampler()
    assert fake_host.names() == ["sparf_pick_pixels"] and fake_host.calls[0][1]["pixels"] is False
    assert same_bits(rays, fx[f"{name}/rays"]), name


def test_ray_sampler_install_put_restore_and_hand_over(fake_host):
    case = STRATEGY_CASES["st_7x9_f0.4_p2_c0"]
    cls = type("RaySamplingStrategy", (Sampler,), {})
    module = types.SimpleNamespace(RaySamplingStrategy=cls)
    losses.install_ray_sampler(module)
    assert cls.__call__ is losses.ray_sampler_call and "__call__" in vars(cls)
    with pytest.raises(RuntimeError, match="already installed"):
        losses.install_ray_sampler(module)
    # the mask-fraction config, and pools that are not their rectangles, reach the original
    assert cls(case, mask_fraction=0.5)(37, True, [0]) == ("original", 37, True, [0])
    odd = cls(case)
    odd.all_possible_pixels = odd.all_possible_pixels[:-1]
    assert odd(37)[0] == "original" and not fake_host.calls
    losses.uninstall_ray_sampler()
    assert "__call__" not in vars(cls) and cls(case)(37)[0] == "original"
    losses.install_ray_sampler(module)                                        # repeatable
    losses.uninstall_ray_sampler()
    losses.uninstall_ray_sampler()


class StubNet:
    """the two render methods DepthConsistencyLoss calls: a plane at depth 3 in front of every camera, half visible"""

    def __init__(self):
        self.calls = []

    def render_image_at_specific_pose_and_rays(self, opt, data_dict, pose, intr, H, W, pixels=None, mode=None, iter=None):
        self.calls.append(("render", tuple(pose.shape), pixels.detach().clone()))
        n = pixels.shape[0]
        return edict(depth=torch.full((1, n, 1), 3.0), opacity=torch.full((1, n, 1), 0.9))

    def render_up_to_maxdepth_at_specific_pose_and_rays(self, opt, data_dict, pose, intr, H, W, depth_max=None, pixels=None, mode=None, iter=None):
        self.calls.append(("render_to_max", tuple(pose.shape), pixels.detach().clone()))
        return edict(all_cumulated=torch.full((1, pixels.shape[0]), 0.5))


def dcons_opt(fraction=0.4):
    return edict(nerf=edict(rand_rays=64), sampled_fraction_in_center=fraction, start_ratio=edict(depth_cons=None), start_iter=edict(depth_cons=0), max_iter=100,
                 diff_loss_type="huber", gradually_decrease_depth_cons_loss=False, depth_cons_loss_reduct_at_x_iter=1000)


def dcons_data(B=3, H=12, W=10):
    intr = torch.tensor([[12.0, 0.0, W / 2], [0.0, 12.0, H / 2], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    poses = torch.eye(4)[:3].repeat(B, 1, 1)                 # cameras side by side that look the same way: the pseudo points stay in view
    poses[:, :, 3] = -torch.tensor([[0.2 * b - 0.2, 0.1 * b, 0.1 * b - 4.0] for b in range(B)])
    return edict(image=torch.zeros(B, 3, H, W), poses_w2c=poses, intr=intr, depth_range=torch.tensor([[0.1, 10.0]] * B), iter=5)


class Loss:
    """what the installed methods read of a DepthConsistencyLoss"""

    def __init__(self):
        self.opt, self.net, self.device, self.seen = dcons_opt(), StubNet(), torch.device("cpu"), []

    def compute_loss_at_sampled_pose(self, data_dict, **kw):
        self.seen.append(kw)
        return {"depth_cons": torch.tensor(1.5)}, {}, {}

    def sample_pose(self, *a):
        return "original"


def test_depth_consistency_sampler_install_put_restore():
    cls = type("DepthConsistencyLoss", (Loss,), {})
    module = types.SimpleNamespace(DepthConsistencyLoss=cls)
    losses.install_depth_consistency_sampler(module)
    assert all(vars(cls)[n] is fn for n, fn in losses.DCONS_SAMPLER_METHODS.items()) and set(losses.DCONS_SAMPLER_METHODS) == {
        "sample_pose", "compute_loss", "compute_loss_from_existing_pixels"}
    with pytest.raises(RuntimeError, match="already installed"):
        losses.install_depth_consistency_sampler(module)
    # independent of install_depth_consistency(), in either order, and the method of the moment is the one that is called
    losses.install_depth_consistency(module)
    assert cls.compute_loss_at_sampled_pose is losses.compute_loss_at_sampled_pose
    losses.uninstall_depth_consistency()
    loss = cls()
    assert loss.compute_loss(loss.opt, dcons_data(), {}, 5, mode="val") == ({}, {}, {})
    assert loss.compute_loss(edict(loss.opt, start_iter=edict(depth_cons=9)), dcons_data(), {}, 5, mode="train") == ({}, {}, {}) and not loss.net.calls
    np.random.seed(3)
    torch.manual_seed(3)
    out = loss.compute_loss(loss.opt, dcons_data(), {}, 5, mode="train")
    assert float(out[0]["depth_cons"]) == 1.5 and len(loss.seen) == 1 and [c[:2] for c in loss.net.calls] == [("render", (3, 4))]
    kw = loss.seen[0]
    assert set(kw) == {"pose_w2c_at_unseen", "intr_at_unseen", "pseudo_gt_3dpts_in_w", "H", "W", "pixels_in_ref"} and kw["pose_w2c_at_unseen"].shape == (4, 4)
    assert kw["pixels_in_ref"].shape == (99 + 24, 2) and kw["pseudo_gt_3dpts_in_w"].shape == (123, 3) and (kw["H"], kw["W"]) == (12, 10)
    # the same draws by hand: randint, the two permutations, then rand
    np.random.seed(3)
    torch.manual_seed(3)
    id_self = np.random.randint(3)
    pixels, _ = losses.sample_pixels_torch(12, 10, nbr=1024, fraction_in_center=0.4)
    want = losses.sample_unseen_pose_torch(dcons_data().poses_w2c, id_self, np.random.rand())
    assert torch.equal(kw["pixels_in_ref"], pixels) and torch.equal(kw["pose_w2c_at_unseen"], want.pose_w2c_at_unseen)
    assert torch.equal(loss.net.calls[0][2], pixels)
    # from existing pixels: one rand
    np.random.seed(4)
    loss.compute_loss_from_existing_pixels(loss.opt, dcons_data(), 5, pixels[:7], 2, torch.full((7,), 3.0))
    np.random.seed(4)
    want = losses.sample_unseen_pose_torch(dcons_data().poses_w2c, 2, np.random.rand())
    assert torch.equal(loss.seen[1]["pose_w2c_at_unseen"], want.pose_w2c_at_unseen) and loss.seen[1]["pixels_in_ref"].shape == (7, 2)
    assert torch.equal(loss.seen[1]["pseudo_gt_3dpts_in_w"], losses.backproject_to_3d_torch(pixels[:7], torch.full((7,), 3.0), dcons_data().intr[2], want.pose_c2w_ref))
    # sample_pose under the reference's signature
    np.random.seed(5)
    poses = want.pose_w2c_ref.new_zeros(3, 4, 4)
    full = torch.cat((dcons_data().poses_w2c, torch.tensor([0., 0., 0., 1.]).reshape(1, 1, 4).repeat(3, 1, 1)), dim=1)
    c2w = losses._pose_inverse_batched_torch(full)
    got = loss.sample_pose(c2w, 2, full[2])
    np.random.seed(5)
    assert torch.equal(got, losses.sample_unseen_pose_torch(full, 2, np.random.rand()).pose_w2c_at_unseen) and poses.shape == (3, 4, 4)
    losses.uninstall_depth_consistency_sampler()
    assert not set(losses.DCONS_SAMPLER_METHODS) & set(vars(cls)) and cls().sample_pose() == "original"
    losses.install_depth_consistency_sampler(module)                         # repeatable
    losses.uninstall_depth_consistency_sampler()
    losses.uninstall_depth_consistency_sampler()


@pytest.mark.skipif(ref_harness.reference_root() is None, reason="the reference tree is not present")
@pytest.mark.parametrize("fraction", (0.0, 0.4))
def test_generators_after_the_reference_and_after_the_install(fraction):
    """the parity contract with an unmodified trainer: np.random and torch's CPU generator are left in the same state, and on the CPU
    route -- the reference's operations -- the loss is the same"""
    assert ref_harness.install_reference()
    import source.training.core.depth_cons_loss as ref_dcons

    def run():
        np.random.seed(11)
        torch.manual_seed(11)
        loss = ref_dcons.DepthConsistencyLoss(dcons_opt(fraction), StubNet(), torch.device("cpu"))
        out = loss.compute_loss(loss.opt, dcons_data(), {}, 5, mode="train")
        return out, loss.net.calls, np.random.get_state(), torch.get_rng_state()
    ref = run()
    losses.install_depth_consistency_sampler(ref_dcons)
    try:
        got = run()
    finally:
        losses.uninstall_depth_consistency_sampler()
    assert "compute_loss" in vars(ref_dcons.DepthConsistencyLoss) and vars(ref_dcons.DepthConsistencyLoss)["compute_loss"] is not losses.dcons_compute_loss
    for a, b in zip(ref[2], got[2]):
        assert np.array_equal(a, b)
    assert torch.equal(ref[3], got[3])
    assert [c[:2] for c in ref[1]] == [c[:2] for c in got[1]] and len(ref[1]) == 3
    assert all(torch.equal(a[2], b[2]) for a, b in zip(ref[1], got[1]))     # the same pixels into every render
    assert torch.equal(ref[0][0]["depth_cons"], got[0][0]["depth_cons"]) and ref[0][1].keys() == got[0][1].keys()


def test_build_lists_the_unit():
    assert "pick.hip" in BUILD.SOURCES and "pick.h" in BUILD.HEADERS
    deps = {d.rsplit("/", 1)[-1] for d in BUILD._deps(BUILD.CSRC + "/pick.hip")}
    assert {"pick.h", "ordered.h", "sparf_hip.h"} <= deps
    # the unit needs no LDS tile, no atomic and no inline assembly: all its writes are plain stores
    src = open(BUILD.CSRC + "/pick.hip").read() + open(BUILD.CSRC + "/pick.h").read()
    assert "__shared__" not in src and "atomic" not in src.replace("no atomic", "") and "asm" not in src
