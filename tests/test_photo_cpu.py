"""The photometric / mask / depth-patch loss without a GPU: the float64 referee (tests/photo_referee.py, which states
the kernel's bounds) against the fixture (tests/golden/photo_regu.npz: the reference's own fp32 values); the torch restatements of
sparf_amd.losses against both; what ops.PhotoReguLoss hands the library, over a stand-in that records calls (tests/photo_fake.py); the
routes; the argument checks of the C-ABI entry point; install_photometric() / uninstall_photometric()."""
import ctypes
import types

import numpy as np
import pytest
import torch

from sparf_amd import lib as L, losses, ops
from sparf_amd.edict import EasyDict as edict
from tests import photo_fake, photo_referee as R

# The reference's own fp32 distance from the float64 value.  Every term is a sum of non-negative fp32 elements, each the result of at
# most 5 roundings (difference, square or product, the Charbonnier root), added by torch's cascaded sum (error growing with log2 of the
# count, at most 14 levels here) and divided once: (5 + 14 + 1) half-spacings in the worst case.
REF_OUT_SPACINGS = 10.0
# its gradients: a colour or mask seed is a difference, a constant factor and a division (<= 4 roundings: 4 x 2^-24 elementwise, so also
# in relative L2); a depth seed adds up to 64 quotients of mixed sign, each with the roundings of the square, the sum, the root and the
# division behind it ((64 + 8) x 2^-24 in the worst case)
REF_SEED_L2 = dict(rgb=2.0 ** -22, rgb_fine=2.0 ** -22, opacity=2.0 ** -22, opacity_fine=2.0 ** -22, depth=72 * 2.0 ** -24, depth_fine=72 * 2.0 ** -24)


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def wants(fx):
    cache = {}

    def get(name):
        if name not in cache:
            x = R.inputs(fx, name)
            cache[name] = (x, R.want(x))
        return cache[name]
    return get


def T(a, grad=False):
    return torch.from_numpy(np.array(a)).requires_grad_(grad) if a is not None else None


def tensors(x, grad=True):
    return {k: T(x[k], grad) for k in R.TENSORS}


def call(fn, x, t, **kw):
    return fn(T(x["image"]), T(x["ray_idx"]), t["rgb"], t["rgb_fine"], fg_mask=T(x["fg_mask"]), opacity=t["opacity"], opacity_fine=t["opacity_fine"],
              depth=t["depth"], depth_fine=t["depth_fine"], huber=x["kind"] == "huber", patch_size=x["patch"] or None, **kw)


def out5(loss, mse):
    return np.array([float(loss[k].detach()) if k in loss else 0.0 for k in R.OUT_KEYS[:3]] + [float(mse["mse"]), float(mse["mse_fine"]) if mse["mse_fine"] is not None else 0.0])


def test_the_row_pools_are_the_generators(fx):
    assert np.array_equal(R.pool_check(), fx["pool_check"])
    assert set(fx) == {"image", "fg_mask", "pool_check"} | {f"ref_{c}" for c in R.CASES} | {f"seed_{c}_{k}" for c, v in R.CASES.items() for k in v["seeds"]
                                                                                          if R.inputs(fx, c)[k] is not None}
    assert 0.3 < fx["fg_mask"].mean() < 0.5 and fx["image"].shape == (3, 3, R.H, R.W) and fx["fg_mask"].dtype == np.bool_


@pytest.mark.parametrize("name", R.CASES)
def test_referee_against_the_references_values(fx, wants, name):
    x, w = wants(name)
    ref = fx[f"ref_{name}"]
    on = w["out"] != 0
    assert np.array_equal(ref != 0, on)
    excess = R.fwd_excess(ref[on], w["out"][on])
    print(name, "reference to float64:", excess, "fp32 spacings")
    assert excess <= REF_OUT_SPACINGS
    for key in R.CASES[name]["seeds"]:
        if x[key] is None:
            continue
        d = R.rel_l2(fx[f"seed_{name}_{key}"], w["seeds"][key])
        print(name, key, d)
        assert d <= REF_SEED_L2[key], (key, d)
    s32, s64, ab = R.kink_sides(x)
    assert np.array_equal(s32, s64) and (np.abs(ab - R.DELTA) >= R.KINK_MARGIN).all()
    if x["patch"]:
        const = R.constant_rows(x)
        assert const.any() and (w["seeds"]["depth"].reshape(-1)[const] == 0).all()
        assert (x["opacity"] is None) or (np.abs(x["opacity"]) > 0).all()


def held(got, ref32, want64, measure, what):
    """the restatement within 4x the reference's own distance from the referee (the project's rule, tests/dcons_referee.py)"""
    d_ref, d_got = measure(ref32, want64), measure(got, want64)
    print(f"{what}: reference {d_ref:.3e}  restatement {d_got:.3e}")
    assert d_got <= 4 * d_ref, (what, d_got, d_ref)


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_within_the_references_distance(fx, wants, name):
    x, w = wants(name)
    t = tensors(x)
    loss, mse = call(losses.photo_and_regu_loss, x, t)            # CPU tensors: the restatement
    assert set(loss) == {"render"} | ({"fg_mask"} if x["fg_mask"] is not None else set()) | ({"depth_patch"} if x["patch"] else set())
    assert all(v.dim() == 0 for v in loss.values()) and not mse["mse"].requires_grad and (mse["mse_fine"] is None) == (x["rgb_fine"] is None)
    got, ref = out5(loss, mse), fx[f"ref_{name}"]
    for i, key in enumerate(R.OUT_KEYS):
        held(got[i], ref[i], w["out"][i], lambda a, b: abs(float(a) - float(b)), key)
    for key in R.CASES[name]["seeds"]:
        if x[key] is not None:
            g, = torch.autograd.grad(loss[R.TERM_OF[key]], t[key], retain_graph=True)
            held(g, fx[f"seed_{name}_{key}"], w["seeds"][key], R.rel_l2, key)


def _modules():
    class Theirs:
        def compute_loss(self, opt, data_dict, output_dict, iteration, mode=None, plot=False, **kwargs):
            return "theirs", iteration, mode

    return types.SimpleNamespace(BasePhotoandReguLoss=Theirs), types.SimpleNamespace(compute_mse_on_rays=lambda d, o: "their mse", other=1)


def _trainer_args(x, t, distortion=None, start=0):
    B, P = x["B"], x["patch"]
    opt = edict(start_iter=edict(photometric=start), huber_loss_for_photometric=x["kind"] == "huber", depth_regu_patch_size=P or 2,
                loss_weight=edict(fg_mask=-1 if x["fg_mask"] is not None else None, depth_patch=-3 if P else None, distortion=distortion),
                nerf=edict(rand_rays=x["N"] if x["ray_idx"] is not None else None))
    data = edict(idx=torch.arange(B), image=T(x["image"]), fg_mask=T(x["fg_mask"]))
    output = edict(idx_img_rendered=torch.arange(B), **{k: v for k, v in t.items() if v is not None})
    if x["ray_idx"] is not None:
        output.ray_idx = T(x["ray_idx"])
    return opt, data, output


@pytest.mark.parametrize("name", ["shared64_huber", "per_image64_mse", "full3_huber", "colour_mse", "p3_63"])
def test_installed_method_and_mse_give_the_references_values(fx, wants, name):
    """compute_loss and mse_on_rays under the trainer's names, on CPU tensors (the restatement): the reference's keys and, its
    operation order being restated, its values to 4x its own distance from float64"""
    x, w = wants(name)
    base, trainer = _modules()
    losses.install_photometric(base, trainer)
    try:
        obj = base.BasePhotoandReguLoss()
        t = tensors(x)
        opt, data, output = _trainer_args(x, t)
        obj.opt, obj.device = opt, torch.device("cpu")
        loss, stats, plots = obj.compute_loss(opt, data, output, iteration=3, mode="train")
        mse, mse_fine = trainer.compute_mse_on_rays(data, output)
    finally:
        losses.uninstall_photometric()
    assert stats == {} and plots == {} and (mse_fine is None) == (x["rgb_fine"] is None)
    assert set(loss.keys()) == {"render"} | ({"fg_mask"} if x["fg_mask"] is not None else set()) | ({"depth_patch"} if x["patch"] else set())
    got, ref = out5(loss, dict(mse=mse, mse_fine=mse_fine)), fx[f"ref_{name}"]
    for i, key in enumerate(R.OUT_KEYS):
        held(got[i], ref[i], w["out"][i], lambda a, b: abs(float(a) - float(b)), key)
    loss.render.backward()
    assert t["rgb"].grad is not None


def test_method_before_the_start_iteration_and_with_distortion(fx, wants):
    x, _ = wants("shared64_huber")
    base, trainer = _modules()
    t = tensors(x)
    with pytest.raises(RuntimeError, match="no original method"):
        opt, data, output = _trainer_args(x, t, distortion=1e-3)
        losses.compute_loss(types.SimpleNamespace(opt=opt, device=torch.device("cpu")), opt, data, output, 3, mode="train")
    losses.install_photometric(base, trainer)
    try:
        with pytest.raises(RuntimeError, match="already installed"):
            losses.install_photometric(base)
        losses.install(types.SimpleNamespace(CorrespondencesPairRenderDepthAndGet3DPtsAndReproject=type("C", (), {})))       # independent of the others
        losses.install_depth_consistency(types.SimpleNamespace(DepthConsistencyLoss=type("D", (), {})))
        losses.uninstall()
        losses.uninstall_depth_consistency()
        assert trainer.compute_mse_on_rays is losses.mse_on_rays and base.BasePhotoandReguLoss.compute_loss is losses.compute_loss
        obj = base.BasePhotoandReguLoss()
        opt, data, output = _trainer_args(x, t, start=10)
        obj.opt, obj.device = opt, torch.device("cpu")
        loss, stats, plots = obj.compute_loss(opt, data, output, iteration=9, mode="train")
        assert list(loss.keys()) == ["render"] and loss.render.item() == 0.0 and loss.render.requires_grad and stats == {} and plots == {}
        # the distortion loss is not built: the saved original is called with what the trainer passed, and its return is returned
        opt, data, output = _trainer_args(x, t, distortion=1e-3)
        obj.opt = opt
        assert obj.compute_loss(opt, data, output, 7, mode="val") == ("theirs", 7, "val")
        # mode outside train / test-optim: the whole images (here: as many rays as pixels are needed)
        opt, data, output = _trainer_args(x, t)
        obj.opt = opt
        with pytest.raises((RuntimeError, ValueError)):
            obj.compute_loss(opt, data, output, 7, mode="val")
    finally:
        losses.uninstall_photometric()
    assert base.BasePhotoandReguLoss().compute_loss(None, None, None, 1) == ("theirs", 1, None)
    assert trainer.compute_mse_on_rays(None, None) == "their mse" and trainer.other == 1 and not losses._photo.originals
    # a module that had no such name loses it again
    bare = types.SimpleNamespace()
    losses.install_photometric(base, bare)
    assert bare.compute_mse_on_rays is losses.mse_on_rays
    losses.uninstall_photometric()
    assert not hasattr(bare, "compute_mse_on_rays")


# ---------------------------------------------------------------------------------------------- the glue over a recording stand-in
@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(losses, "_takes_kernel", lambda values, constants: not losses._unfused)     # CPU tensors down the fused route
    with photo_fake.installed() as lib:
        yield lib


GIVEN = dict(image=True, fg_mask=False, ray_idx=True, per_image=0, B=2, HW=12, N=8, rgb=True, rgb_fine=False, opacity=False, opacity_fine=False,
             depth=False, depth_fine=False, kind=0, delta=0.5, patch=0, charbonnier=pytest.approx(0.001), out=True, d_rgb=False, d_rgb_fine=False,
             d_opacity=False, d_opacity_fine=False, d_depth=False, d_depth_fine=False, workspace=False)


def _small(B=2, N=8, grad=()):
    t = dict(rgb=torch.rand(B, N, 3), rgb_fine=torch.rand(B, N, 3), opacity=torch.rand(B, N, 1), opacity_fine=torch.rand(B, N, 1),
             depth=torch.rand(B, N, 1), depth_fine=torch.rand(B, N, 1))
    for k in grad:
        t[k].requires_grad_()
    return torch.rand(B, 3, 3, 4), torch.rand(B, 1, 3, 4) > 0.5, torch.arange(N), t


def test_pointers_for_every_combination_of_terms_and_gradients(fake):
    for fine in (False, True):
        for mask in (False, True):
            for patch in (None, 2):
                for grad in ((), ("rgb",), ("rgb_fine", "opacity"), ("opacity_fine", "depth", "depth_fine"), R.TENSORS):
                    image, fg, idx, t = _small(grad=grad)
                    fake.calls.clear()
                    loss, mse = losses.photo_and_regu_loss(image, idx, t["rgb"], t["rgb_fine"] if fine else None, fg_mask=fg if mask else None,
                                                           opacity=t["opacity"], opacity_fine=t["opacity_fine"] if fine else None, depth=t["depth"],
                                                           depth_fine=t["depth_fine"] if fine else None, huber=fine, patch_size=patch)
                    present = dict(rgb=True, rgb_fine=fine, opacity=mask, opacity_fine=mask and fine, depth=bool(patch), depth_fine=bool(patch) and fine)
                    want = dict(GIVEN, fg_mask=mask, kind=int(fine), patch=patch or 0, **present, **{"d_" + k: present[k] and k in grad for k in R.TENSORS})
                    assert fake.calls == [("sparf_photo_regu_loss", want)], (fine, mask, patch, grad)
                    assert set(loss) == {"render"} | ({"fg_mask"} if mask else set()) | ({"depth_patch"} if patch else set())
                    assert [float(loss.get(k, i + 1.0)) for i, k in enumerate(R.OUT_KEYS[:3])] == [1.0, 2.0, 3.0] and float(mse["mse"]) == 4.0
                    assert (float(mse["mse_fine"]) == 5.0) if fine else mse["mse_fine"] is None
                    assert not mse["mse"].requires_grad and all(v.dim() == 0 for v in loss.values())
                    live = [k for k in grad if present[k]]
                    if live:
                        assert loss["render"].grad_fn is not None and type(loss["render"].grad_fn).__name__.startswith("PhotoReguLoss")
                        sum(R.UPSTREAM[k] * v for k, v in loss.items()).backward()
                        assert fake.names() == ["sparf_photo_regu_loss"]            # the backward makes no call
                        for k in R.TENSORS:
                            assert (t[k].grad is not None and t[k].grad.shape == t[k].shape) == (k in live), k
                    else:
                        assert not any(v.requires_grad for v in loss.values())


def test_backward_scales_each_seed_by_its_own_upstream(fake, monkeypatch):
    image, fg, idx, t = _small(grad=R.TENSORS)
    with monkeypatch.context() as m:
        m.setattr(torch, "empty_like", torch.ones_like)              # the seeds, which the stand-in never writes
        loss, _ = losses.photo_and_regu_loss(image, idx, t["rgb"], t["rgb_fine"], fg_mask=fg, opacity=t["opacity"], opacity_fine=t["opacity_fine"],
                                             depth=t["depth"], depth_fine=t["depth_fine"], patch_size=2)
    sum(R.UPSTREAM[k] * v for k, v in loss.items()).backward()
    for k in R.TENSORS:
        assert torch.equal(t[k].grad, torch.full_like(t[k], R.UPSTREAM[R.TERM_OF[k]])), k
    # a term that is not used downstream gives None, not zeros
    image, fg, idx, t = _small(grad=R.TENSORS)
    loss, _ = losses.photo_and_regu_loss(image, idx, t["rgb"], fg_mask=fg, opacity=t["opacity"], depth=t["depth"], patch_size=2)
    loss["fg_mask"].backward()
    assert t["rgb"].grad is None and t["depth"].grad is None and t["opacity"].grad is not None


def test_ray_idx_forms_sizes_and_empty(fake):
    image, fg, idx, t = _small()
    losses.photo_and_regu_loss(image, torch.arange(16).reshape(2, 8) % 12, t["rgb"])
    assert fake.calls[-1][1] == dict(GIVEN, per_image=1)
    full = torch.rand(2, 12, 3)
    losses.photo_and_regu_loss(image, None, full)
    assert fake.calls[-1][1] == dict(GIVEN, ray_idx=False, N=12)
    losses.photo_and_regu_loss(image.reshape(2, 3, 12), idx, t["rgb"].reshape(16, 3))           # [B,3,H*W], rows flat
    assert fake.calls[-1][1] == GIVEN
    for bad in (torch.arange(7), torch.arange(16).reshape(1, 16), torch.arange(24).reshape(3, 8)):
        with pytest.raises(ValueError, match="ray_idx must be int64"):
            losses.photo_and_regu_loss(image, bad, t["rgb"])
    with pytest.raises(ValueError, match="full images"):
        losses.photo_and_regu_loss(image, None, t["rgb"])
    with pytest.raises(ValueError, match="no whole number"):
        losses.photo_and_regu_loss(image, torch.arange(6), torch.rand(2, 6, 3), depth=torch.rand(2, 6, 1), patch_size=2)
    with pytest.raises(ValueError, match="needs opacity"):
        losses.photo_and_regu_loss(image, idx, t["rgb"], fg_mask=fg)
    with pytest.raises(ValueError, match="needs depth"):
        losses.photo_and_regu_loss(image, idx, t["rgb"], patch_size=2)
    with pytest.raises(ValueError, match="opacity has 8 elements for 16 rays"):
        losses.photo_and_regu_loss(image, idx, t["rgb"], fg_mask=fg, opacity=torch.rand(8))
    # above the one-workgroup limit: a workspace; rows == 0: one call that launches nothing
    n = photo_fake.CHUNK + 1
    losses.photo_and_regu_loss(torch.rand(1, 3, 3, 4), torch.zeros(n, dtype=torch.int64), torch.rand(1, n, 3))
    assert fake.calls[-1][1] == dict(GIVEN, B=1, N=n, workspace=True)
    fake.calls.clear()
    loss, mse = losses.photo_and_regu_loss(torch.rand(1, 3, 3, 4), torch.zeros(0, dtype=torch.int64), torch.rand(1, 0, 3))
    assert fake.calls == [("sparf_photo_regu_loss", dict(GIVEN, B=1, N=0, rgb=False, ray_idx=False))] and loss["render"].dim() == 0


def test_routes(fake, monkeypatch):
    """the kernel's rule is _takes_kernel's; whatever it does not cover takes the restatement"""
    image, fg, idx, t = _small()
    kw = dict(fg_mask=fg, opacity=t["opacity"])
    with losses.unfused():
        losses.photo_and_regu_loss(image, idx, t["rgb"], **kw)
    losses.photo_and_regu_loss(image, idx, t["rgb"], fg_mask=fg.float(), opacity=t["opacity"])              # a float mask
    losses.photo_and_regu_loss(image.double(), idx, t["rgb"].double())                                       # float64 (the image's dtype)
    losses.photo_and_regu_loss(image, idx.int(), t["rgb"])                                                   # int32 indices
    d = torch.rand(2, 81, 1)
    losses.photo_and_regu_loss(image, torch.zeros(81, dtype=torch.int64), torch.rand(2, 81, 3), depth=d, patch_size=9)       # P > 8
    assert fake.calls == []
    monkeypatch.undo()                                                                                       # the real _takes_kernel
    with photo_fake.installed() as lib:
        losses.photo_and_regu_loss(image, idx, t["rgb"], **kw)                                               # CPU tensors
        g = image.clone().requires_grad_()
        loss, _ = losses.photo_and_regu_loss(g, idx, t["rgb"])
        assert lib.calls == [] and loss["render"].requires_grad
        seen = []
        real_ok = losses._takes_kernel
        monkeypatch.setattr(losses, "_takes_kernel", lambda values, constants: seen.append((values, constants)) or real_ok(values, constants))
        losses.photo_and_regu_loss(g, idx, t["rgb"], t["rgb_fine"], **kw)
        (values, constants), = seen
        assert values[0] is t["rgb"] and values[1] is t["rgb_fine"] and values[2] is t["opacity"] and values[3:] == (None, None, None)
        assert constants[0] is g and constants[1] is idx and constants[2] is fg                              # no gradient asked of the image
        assert lib.calls == []


def test_mse_on_rays_calls_the_kernel_without_seeds(fake):
    image, fg, idx, t = _small(grad=("rgb", "rgb_fine"))
    data = edict(idx=torch.arange(2), image=image)
    out = edict(idx_img_rendered=torch.arange(2), ray_idx=idx, rgb=t["rgb"], rgb_fine=t["rgb_fine"])
    mse, mse_fine = losses.mse_on_rays(data, out)
    assert fake.calls == [("sparf_photo_regu_loss", dict(GIVEN, rgb_fine=True))] and float(mse) == 4.0 and float(mse_fine) == 5.0
    assert not mse.requires_grad
    del out["rgb_fine"], out["ray_idx"]
    out.rgb = torch.rand(1, 12, 3)
    out.idx_img_rendered = [1]                                       # a subset of the images, full renders
    mse, mse_fine = losses.mse_on_rays(data, out)
    assert fake.calls[-1][1] == dict(GIVEN, B=1, N=12, ray_idx=False) and mse_fine is None
    with losses.unfused():
        a, b = losses.mse_on_rays(data, out)
    assert b is None and torch.equal(a, ((out.rgb - image[1].reshape(1, 3, 12).permute(0, 2, 1)) ** 2).mean()) and len(fake.calls) == 2


# ---------------------------------------------------------------------------------------------- the real library, no device
def test_entry_point_checks_its_arguments_without_a_device():
    """every refusal is decided before any HIP call"""
    lib = L.load()
    buf = np.zeros(64, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)         # host memory: never dereferenced, every call below returns before a launch
    base = dict(image=p, fg_mask=p, ray_idx=p, per_image=0, B=2, HW=12, N=8, rgb=p, rgb_fine=p, opacity=p, opacity_fine=p, depth=p, depth_fine=p,
                kind=1, delta=0.5, patch=2, charbonnier=0.001, out=p, d_rgb=p, d_rgb_fine=p, d_opacity=p, d_opacity_fine=p, d_depth=p,
                d_depth_fine=p, workspace=None)
    assert tuple(base) == photo_fake.PHOTO_CALLS["sparf_photo_regu_loss"]

    def call(**kw):
        assert set(kw) <= set(base)
        return lib.sparf_photo_regu_loss(*dict(base, **kw).values(), None)
    assert call(B=-1) == 1 and call(HW=-1) == 1 and call(N=-8) == 1                      # a negative size
    assert call(kind=2) == 1 and call(kind=-1) == 1
    assert call(patch=-1) == 1 and call(patch=9) == 1
    assert call(patch=3) == 1 and call(N=6) == 1                                          # N % P^2 != 0
    assert call(depth=None, depth_fine=None, d_depth=None, d_depth_fine=None) == 1        # a patch term without depth
    assert call(rgb_fine=None) == 1 and call(opacity_fine=None) == 1 and call(depth_fine=None) == 1        # a fine seed without its tensor
    assert call(opacity=None, opacity_fine=None, d_opacity=None, d_opacity_fine=None) == 1                 # fg_mask without opacity
    assert call(fg_mask=None, opacity=None, d_opacity_fine=None, opacity_fine=None) == 1                   # a seed without its tensor
    assert call(ray_idx=None) == 1                                                        # the identity is a full image
    for name in ("image", "rgb", "out"):
        assert call(**{name: None}) == 1, name
    assert call(N=0, out=None) == 1
    wb = lib.sparf_photo_regu_workspace_bytes
    assert wb(0) == 0 and wb(-3) == 0 and wb(4096) == 0 and wb(4097) == photo_fake.workspace_bytes(4097) == 128 and wb(8200) == 192
