"""The correspondence sampler without a GPU: the torch restatement of sparf_amd.losses against the fixture
(tests/golden/matches.npz: what the reference's own chain did) and the numpy referee (tests/matches_referee.py), bit for bit; the
argument checks of the C-ABI entry points; what select_matches hands the library, over a stand-in that records calls
(tests/matches_fake.py); the early returns; install_sampler() / uninstall_sampler(); the hand-over of the debug configurations; and,
where the reference tree is present, its unmodified chain before and after the installation, from the same seed."""
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
from tests import matches_fake, matches_referee as R, ref_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULTS = ("pixels_self", "ray_self", "pixels_other", "ray_other", "conf")
DTYPES = dict(pixels_self=torch.float32, ray_self=torch.int64, pixels_other=torch.float32, ray_other=torch.int64, conf=torch.float32)


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def T(a):
    return torch.from_numpy(np.array(a)) if a is not None else None


def reference_views(mask, corres, conf):
    """the forms sample_valid_image_pair hands over: permuted views of [1,H,W] / [2,H,W] / [1,H,W] storage"""
    return T(mask)[None].permute(1, 2, 0), T(corres).permute(1, 2, 0)[:, :, :2], T(conf).permute(1, 2, 0)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("name", list(R.FIXTURE_CASES))
def test_restatement_reproduces_the_fixture(fx, name):
    """every array the reference's chain left, bit for bit; the referee agrees with both"""
    case = R.fixture_case(fx, name)
    H, W, _, _, min_nbr = R.FIXTURE_CASES[name]
    mask, corres, conf = reference_views(case["mask"], case["corres"], case["conf"])
    out = losses.select_matches_torch(mask, corres, conf, R.MAX_MATCHES, window=case["window"], perm=T(case["perm"]), min_matches=min_nbr)
    want = R.select_np(case["mask"], case["corres"], case["conf"], R.MAX_MATCHES, case["window"], case["perm"])
    assert out[5] == want["count"] and isinstance(out[5], int)
    if int(case["rendered"]) == 0:
        assert out[5] < min_nbr and all(t.shape[0] == 0 for t in out[:5])
        return
    for key, got, ref in zip(RESULTS, out[:5], ("pixels_self", "ray_self", "pixels_other", "ray_other", "conf_values")):
        same_bits(got.numpy(), case[ref], key)
        same_bits(want[key], case[ref], "referee " + key)
    same_bits(out[6].numpy(), case["perc"], "perc")
    same_bits(want["perc"], case["perc"], "referee perc")
    assert (want["count"] > R.MAX_MATCHES) == (case["perm"] is not None)


@pytest.mark.parametrize("window", R.WINDOWS)
@pytest.mark.parametrize("shape", R.SHAPES[:3], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_against_the_referee_on_generated_cases(shape, window):
    """every pattern; the channel-first and the dense forms of the maps give the same rows"""
    H, W = shape
    corres, conf = R.maps_of(H, W)
    win = R.window_of(H, W, window)
    for pattern in R.PATTERNS:
        mask = R.mask_of(H, W, pattern)
        want = R.select_np(mask, corres, conf, R.MAX_MATCHES, win, R.perm_of(int(R.window_mask(mask, win).sum())))
        perm = T(R.perm_of(want["count"]))
        for m, c, f in (reference_views(mask, corres, conf), (T(mask), T(corres), T(conf)), (T(mask)[..., None], T(corres), T(conf)[0])):
            out = losses.select_matches(m, c, f, R.MAX_MATCHES, window=win, perm=perm)
            assert out[5] == want["count"]
            for key, got in zip(RESULTS, out[:5]):
                same_bits(got.numpy(), want[key], (pattern, key))
            same_bits(out[6].numpy(), want["perc"], (pattern, "perc"))
    if window == "empty":
        assert want["count"] == 0


def test_round_is_half_to_even_and_the_share_is_a_float32_division():
    assert torch.round(torch.tensor([0.5, 1.5, 2.5, -0.0, -0.5])).tolist() == [0.0, 2.0, 2.0, 0.0, 0.0]
    m = torch.ones(7, 9, dtype=torch.bool)
    share = m.sum() / (m.nelement() + 1e-6)
    assert share.dtype == torch.float32 and float(share) == float(np.float32(63) / np.float32(63 + 1e-6))
    assert ops.match_window((3, 2, 0, 5), 7, 9) == (3, 2, 0, 5) and ops.match_window(None, 7, 9) == (0, 7, 0, 9)
    assert ops.match_window((-2, 100, 1, -1), 7, 9) == (5, 7, 1, 8)          # as Python reads the slices


def test_entry_points_check_their_arguments_without_a_device():
    lib = L.load()
    buf = np.zeros(64, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)         # host memory: never dereferenced, every call below returns before a launch

    def call(name, defaults, **kw):
        assert tuple(defaults) == matches_fake.MATCH_CALLS[name] and set(kw) <= set(defaults), name
        return getattr(lib, name)(*dict(defaults, **kw).values(), None)

    compact = lambda **kw: call("sparf_match_compact", dict(mask=p, H=4, W=4, y0=0, y1=4, x0=0, x1=4, index=p, count=p, perc=None, workspace=None), **kw)
    gather = lambda **kw: call("sparf_match_gather", dict(index=p, count=p, sel=None, k=2, H=4, W=4, corres=p, corres_channel_stride=16, conf=p,
                                                          pixels_self=p, ray_self=p, pixels_other=p, ray_other=p, conf_out=p), **kw)
    assert compact(H=-1) == 1 and compact(W=-1) == 1 and compact(H=1 << 16, W=1 << 16) == 1
    for name in ("mask", "index", "count"):
        assert compact(**{name: None}) == 1, name
    assert gather(k=-1) == 1 and gather(H=-1) == 1 and gather(corres_channel_stride=-1) == 1 and gather(H=0) == 1
    for name in ("index", "count", "corres", "conf", "pixels_self", "ray_self", "pixels_other", "ray_other", "conf_out"):
        assert gather(**{name: None}) == 1, name
    assert gather(k=0) == 0 and gather(k=0, index=None, corres=None) == 0           # nothing to launch, no pointer looked at
    wb = lib.sparf_match_workspace_bytes
    assert wb(0) == 0 and wb(-3) == 0 and wb(4096) == 0 and wb(4097) == matches_fake.workspace_bytes(4097) == 8 and wb(12288) == 12


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(losses, "_takes_kernel", lambda values, constants: not losses._unfused)     # CPU tensors down the fused route
    with matches_fake.installed() as lib:
        yield lib


def test_one_compact_one_gather_one_readback(fake):
    H, W = 65, 65
    mask_store = torch.ones(3, 1, H, W, dtype=torch.bool)            # mask_valid_corr: pair 1 starts at byte H W, no alignment
    corres_store, conf_store = torch.zeros(3, 2, H, W), torch.ones(3, 1, H, W)
    mask, corres, conf = mask_store[1].permute(1, 2, 0), corres_store[1].permute(1, 2, 0)[:, :, :2], conf_store[1].permute(1, 2, 0)
    reads = []
    real_item = torch.Tensor.item
    fake.keep = 300
    torch.manual_seed(5)
    torch.Tensor.item = lambda t: (reads.append(t.dtype), real_item(t))[1]
    try:
        out = losses.select_matches(mask, corres, conf, 128, window=(16, 47, 16, 47))
    finally:
        torch.Tensor.item = real_item
    given = dict(mask=True, H=H, W=W, y0=16, y1=47, x0=16, x1=47, index=True, count=True, perc=True, workspace=True)
    rows = dict(index=True, count=True, sel=True, k=128, H=H, W=W, corres=True, corres_channel_stride=H * W, conf=True, pixels_self=True,
                ray_self=True, pixels_other=True, ray_other=True, conf_out=True)
    assert fake.calls == [("sparf_match_compact", given), ("sparf_match_gather", rows)]
    assert reads == [torch.int32]                                   # the one readback: the count
    # the reference's views are read in place: the pointers are the stored tensors' own
    assert fake.raw[0][1]["mask"] == mask_store[1].data_ptr() and mask_store[1].data_ptr() % 4 != 0
    assert fake.raw[1][1]["corres"] == corres_store[1].data_ptr() and fake.raw[1][1]["conf"] == conf_store[1].data_ptr()
    assert fake.raw[1][1]["index"] == fake.raw[0][1]["index"] and fake.raw[1][1]["count"] == fake.raw[0][1]["count"]
    assert out[5] == 300 and [tuple(t.shape) for t in out[:5]] == [(128, 2), (128,), (128, 2), (128,), (128, 1)]
    assert [t.dtype for t in out[:5]] == [DTYPES[k] for k in RESULTS] and out[6].dim() == 0 and out[6].dtype == torch.float32
    torch.manual_seed(5)
    torch.randperm(300)
    state = torch.get_rng_state()
    torch.manual_seed(5)
    losses.select_matches(mask, corres, conf, 128)
    assert torch.equal(torch.get_rng_state(), state)                 # one randperm(count), as the reference draws it
    # count <= max_matches: nothing drawn, no selection; the first three channels of a [3,H,W] map: stride H W all the same; up to 4096
    # pixels no workspace; channel-first maps and a plain [H,W] mask
    fake.calls.clear(), fake.raw.clear()
    state = torch.get_rng_state()
    small = torch.zeros(3, 16, 16)
    out = losses.select_matches(torch.ones(16, 16, dtype=torch.bool), small[:2], torch.ones(16, 16), 500, perm=torch.arange(256))
    assert torch.equal(torch.get_rng_state(), state)
    assert fake.calls == [("sparf_match_compact", dict(given, H=16, W=16, y0=0, y1=16, x0=0, x1=16, workspace=False)),
                          ("sparf_match_gather", dict(rows, sel=False, k=256, H=16, W=16, corres_channel_stride=256))]
    assert fake.raw[1][1]["corres"] == small.data_ptr() and out[0].shape == (256, 2)
    # a map in another layout is made dense once: a copy, and the pointer is no longer the caller's
    fake.calls.clear(), fake.raw.clear()
    hwc = torch.zeros(16, 16, 2)                                    # pixel-interleaved storage
    losses.select_matches(torch.ones(16, 16, dtype=torch.bool), hwc, torch.ones(16, 16), 500)
    assert fake.raw[1][1]["corres"] != hwc.data_ptr() and fake.calls[1][1]["corres_channel_stride"] == 256
    losses.select_matches(torch.ones(16, 32, dtype=torch.bool)[:, ::2], small[:2], torch.ones(16, 16), 500)
    assert fake.names() == ["sparf_match_compact", "sparf_match_gather"] * 2
    with pytest.raises(ValueError, match="correspondence map must be"):
        losses.select_matches(torch.ones(16, 16, dtype=torch.bool), torch.zeros(16, 16, 3), torch.ones(16, 16), 500)
    with pytest.raises(ValueError, match="confidence map must be"):
        losses.select_matches(torch.ones(16, 16, dtype=torch.bool), small[:2], torch.ones(16, 15), 500)


def test_early_returns_make_no_gather_call(fake):
    mask, corres, conf = torch.ones(32, 32, dtype=torch.bool), torch.zeros(2, 32, 32), torch.ones(1, 32, 32)
    state = torch.get_rng_state()
    for keep, min_matches in ((0, 0), (0, 500), (499, 500)):
        fake.calls.clear()
        fake.keep = keep
        out = losses.select_matches(mask, corres, conf, 100, min_matches=min_matches)
        assert fake.names() == ["sparf_match_compact"] and out[5] == keep
        assert [tuple(t.shape) for t in out[:5]] == [(0, 2), (0,), (0, 2), (0,), (0, 1)] and [t.dtype for t in out[:5]] == [DTYPES[k] for k in RESULTS]
    assert torch.equal(torch.get_rng_state(), state)                 # nothing drawn below the threshold, as in the reference
    fake.calls.clear()
    fake.keep = 500
    assert losses.select_matches(mask, corres, conf, 100, min_matches=500)[0].shape == (100, 2) and fake.names()[-1] == "sparf_match_gather"
    # the restatement takes CPU tensors (here: inside unfused()), non-bool masks, other dtypes
    fake.calls.clear()
    with losses.unfused():
        losses.select_matches(mask, corres, conf, 100)
    with losses.unfused_sampler():
        losses.select_matches(mask, corres, conf, 100)
    losses.select_matches(mask.to(torch.uint8), corres, conf, 100)
    losses.select_matches(mask, corres.double(), conf.double(), 100)
    assert fake.calls == []
    assert ops.match_gather(torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), None, 0, 2, 2, corres, conf)[1].dtype == torch.int64
    assert fake.calls == []                                         # k == 0: empty tensors, no call


class _Net:
    """a render that is a deterministic function of its pixel list"""

    def __init__(self):
        self.calls = []

    def render_image_at_specific_pose_and_rays(self, opt, data_dict, pose, intr, H, W, pixels=None, mode=None, iter=None):
        from sparf_amd.edict import EasyDict as edict
        assert pose.shape == (3, 4) and mode == "train"
        self.calls.append(pixels.clone())
        d = 3.0 + 0.1 * torch.sin(pixels[:, 0] * 0.37) + 0.05 * torch.cos(pixels[:, 1] * 0.11)
        return edict(rgb=torch.zeros(1, pixels.shape[0], 3), depth=d[None, :, None], opacity=torch.ones(1, pixels.shape[0], 1),
                     depth_fine=(d * 1.01)[None, :, None])


def _classes():
    class Base:
        def compute_loss_pairwise(self, *a, **k):
            return ("theirs", "pairwise", a, k)

        def compute_loss_at_given_img_indexes(self, *a, **k):
            return ("theirs", "given", a, k)

    class Pair(Base):
        def compute_loss_on_image_pair(self, *a, **k):
            return ("theirs", "pair", a, k)

    return Base, Pair


def _module(Pair, H, W, pattern="bernoulli", **opt):
    from sparf_amd.edict import EasyDict as edict
    obj = Pair()
    corres, conf = R.maps_of(H, W)
    obj.corres_maps, obj.conf_maps, obj.mask_valid_corr = T(corres)[None], T(conf)[None], T(R.mask_of(H, W, pattern))[None, None]
    obj.filtered_flow_pairs = [(0, 0, 1)]
    obj.net, obj.device = _Net(), torch.device("cpu")
    obj.sample_valid_image_pair = lambda: (0, 1, obj.corres_maps[0].permute(1, 2, 0)[:, :, :2], obj.conf_maps[0].permute(1, 2, 0), None,
                                           obj.mask_valid_corr[0].permute(1, 2, 0))
    obj.opt = edict(dict(dict(min_nbr_matches=10, precrop_iters=100, precrop_frac=R.PRECROP_FRAC, start_iter=edict(corres=0),
                         nerf=edict(rand_rays=2 * R.MAX_MATCHES), compute_photo_on_matches=False, diff_loss_type="huber",
                         renderrepro_do_pixel_reprojection_check=True, renderrepro_do_depth_reprojection_check=False,
                         renderrepro_pixel_reprojection_thresh=10.0, renderrepro_depth_reprojection_thresh=0.1, use_gt_correspondences=False), **opt))
    f = 1.2 * min(H, W)
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    poses = torch.eye(4)[:3].repeat(2, 1, 1)
    poses[1, 0, 3] = 0.2
    data = edict(image=torch.zeros(2, 3, H, W), intr=torch.stack([K, K]), poses_w2c=poses.requires_grad_(), iter=0)
    return obj, data


def test_install_patches_and_uninstall_restores():
    Base, Pair = _classes()
    base_mod, pair_mod = types.SimpleNamespace(CorrespondenceBasedLoss=Base), types.SimpleNamespace(CorrespondencesPairRenderDepthAndGet3DPtsAndReproject=Pair)
    H, W = 64, 65
    obj, data = _module(Pair, H, W)
    losses.install_sampler(pair_mod, base_mod)
    try:
        with pytest.raises(RuntimeError):
            losses.install_sampler(pair_mod, base_mod)
        losses.install(pair_mod)                                    # independent of the other installs
        losses.uninstall()
        torch.manual_seed(3)
        loss, stats, plots = obj.compute_loss_pairwise(obj.opt, data, {}, 0, mode="train")          # the pre-crop phase
        win = R.precrop_window(H, W)
        mask = R.mask_of(H, W, "bernoulli")
        count = int(R.window_mask(mask, win).sum())
        torch.manual_seed(3)
        want = R.select_np(mask, *R.maps_of(H, W), R.MAX_MATCHES, win, torch.randperm(count).numpy())
        assert count > R.MAX_MATCHES and len(obj.net.calls) == 2
        same_bits(obj.net.calls[0].numpy(), want["pixels_self"], "pixels_self")
        same_bits(obj.net.calls[1].numpy(), want["pixels_other"], "pixels_other")
        assert set(stats) == {"perc_valid_corr_mask", "depth_in_corr_loss", "perc_val_pix_rep"} and plots == {}
        same_bits(stats["perc_valid_corr_mask"].numpy(), want["perc"], "perc")
        # the loss of those rows through the public function, by hand
        ret =[obj.net.render_image_at_specific_pose_and_rays(None, None, torch.eye(4)[:3], None, H, W, pixels=T(want[k]), mode="train")
               for k in ("pixels_self", "pixels_other")]
        by_hand, _ = losses.correspondence_pair_loss(T(want["pixels_self"]), T(want["pixels_other"]), ret[0].depth[0, :, 0], ret[1].depth[0, :, 0],
                                                     data.intr[0], data.intr[1], data.poses_w2c[0], data.poses_w2c[1], T(want["conf"]),
                                                     ret[0].depth_fine[0, :, 0], ret[1].depth_fine[0, :, 0], loss_type="huber", pixel_thresh=10.0)
        assert torch.equal(loss["corres"], by_hand) and float(loss["render_matches"].detach()) == 0.0
        loss["corres"].backward()
        assert data.poses_w2c.grad is not None and float(data.poses_w2c.grad.abs().max()) > 0
        # below min_nbr_matches: the dictionaries untouched, no render, nothing drawn
        few, data = _module(Pair, H, W, "seams")
        state = torch.get_rng_state()
        loss, stats, plots = few.compute_loss_pairwise(few.opt, data, {}, 200, mode="train")
        assert stats == {} and plots == {} and few.net.calls == [] and float(loss["corres"].detach()) == 0.0 and loss["corres"].requires_grad
        assert torch.equal(torch.get_rng_state(), state)
        assert few.compute_loss_pairwise(few.opt, data, {}, 200, mode="val")[1] == {}
    finally:
        losses.uninstall_sampler()
    assert Pair().compute_loss_pairwise()[:2] == ("theirs", "pairwise") and Pair().compute_loss_on_image_pair()[:2] == ("theirs", "pair")
    assert "compute_loss_on_image_pair" in vars(Pair) and "compute_loss_pairwise" not in vars(Pair)
    losses.install_sampler(pair_mod, base_mod)                      # and again after an uninstall
    losses.uninstall_sampler()


def test_debug_configurations_reach_the_original_methods():
    Base, Pair = _classes()
    base_mod, pair_mod = types.SimpleNamespace(CorrespondenceBasedLoss=Base), types.SimpleNamespace(CorrespondencesPairRenderDepthAndGet3DPtsAndReproject=Pair)
    obj, data = _module(Pair, 16, 16, use_gt_correspondences=True)
    _, corres, conf, _, mask = obj.sample_valid_image_pair()[1:]
    with pytest.raises(RuntimeError, match="no original method"):
        losses.compute_loss_on_image_pair(obj, data, None, None, None, 0, 1, corres, None, conf, mask[..., 0], None, None, None, None, {}, {}, {})
    losses.install_sampler(pair_mod, base_mod)
    try:
        out = obj.compute_loss_pairwise(obj.opt, data, {}, 0, mode="train")
        assert out[:2] == ("theirs", "pairwise") and out[2] == (obj.opt, data, {}, 0, "train", False)
        out = obj.compute_loss_at_given_img_indexes(obj.opt, data, 0, 1, corres, conf, None, mask, {}, {}, {})
        assert out[:2] == ("theirs", "given") and out[2][7] is mask and out[2][-1] is True
        out = obj.compute_loss_on_image_pair(data, None, None, None, 0, 1, corres, "rounded", conf, mask[..., 0], None, None, None, None, {}, {}, {})
        assert out[:2] == ("theirs", "pair") and out[2][7] == "rounded" and out[3] == {}
        obj.opt.use_gt_correspondences = False
        out = obj.compute_loss_at_given_img_indexes(obj.opt, data, 0, 1, corres, conf, None, mask, {}, {}, {}, False, False)         # skip_verif=False
        assert out[:2] == ("theirs", "given") and out[2][-1] is False and obj.net.calls == []
        # with a window the original gets the mask the reference would have built
        out = obj.compute_loss_at_given_img_indexes(obj.opt, data, 0, 1, corres, conf, None, mask, {}, {}, {}, skip_verif=False, window=(4, 11, 4, 11))
        same_bits(out[2][7][..., 0].numpy(), R.window_mask(R.mask_of(16, 16, "bernoulli"), (4, 11, 4, 11)), "windowed mask")
    finally:
        losses.uninstall_sampler()


@pytest.mark.skipif(ref_harness.reference_root() is None, reason="reference tree not present")
def test_reference_chain_after_install():
    """The reference's unmodified compute_loss_pairwise chain on CPU tensors (the restatement leg), constructed by its own __init__ on the
    fixture's cases, with a `net` whose render is a deterministic function of the pixel list: after install_sampler() against before,
    from the same seed -- identical loss_dict / stats_dict keys and values, identical render requests, and torch's generator left in
    the same state.  In a process of its own: the reference's `source` package must not meet dropin/source here."""
    code = """
        import json, numpy as np, torch
        from tests import matches_referee as R
        from tests.golden import make_matches_golden as M
        from tests.test_matches_cpu import _Net
        import source.training.core.corres_loss as cl, source.training.core.base_corres_loss as bcl
        import sparf_amd.losses as losses
        def run(name, seed):
            net = _Net()
            obj, data = M.build_case(name, net, compute_photo=False)
            data.poses_w2c = data.poses_w2c.clone().requires_grad_()
            torch.manual_seed(seed)
            loss, stats, plots = obj.compute_loss_pairwise(obj.opt, data, {}, data.iter, mode="train")
            state = torch.get_rng_state()
            g = torch.autograd.grad(loss["corres"], data.poses_w2c)[0] if net.calls else torch.zeros(1)
            return loss, stats, plots, state, net.calls, g
        res = {}
        for i, name in enumerate(R.FIXTURE_CASES):
            before = run(name, 100 + i)
            losses.install_sampler(cl, bcl)
            try:
                after = run(name, 100 + i)
            finally:
                losses.uninstall_sampler()
            restored = run(name, 100 + i)
            same = lambda a, b: sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
            res[name] = dict(loss=same(after[0], before[0]), stats=same(after[1], before[1]), plots=after[2] == before[2] == {},
                             state=bool(torch.equal(after[3], before[3])), renders=len(after[4]) == len(before[4]) and
                             all(torch.equal(a, b) for a, b in zip(after[4], before[4])), grad=bool(torch.equal(after[5], before[5])),
                             restored=same(restored[0], before[0]), keys=sorted(after[1]), nrender=len(after[4]))
        print(json.dumps(res))
    """
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "compat")])
    p = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(res) == set(R.FIXTURE_CASES)
    for name, r in res.items():
        assert all(r[k] for k in ("loss", "stats", "plots", "state", "renders", "grad", "restored")), (name, r)
        assert r["nrender"] == (0 if name.startswith("too_few") else 2), (name, r)
        assert r["keys"] == ([] if name.startswith("too_few") else ["depth_in_corr_loss", "perc_valid_corr_mask"]), (name, r)
