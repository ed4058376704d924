"""sparf_amd.patcher.Patcher on stand-in classes and modules, and every public install / uninstall pair of the package on stand-in
targets: after install then uninstall every target holds what it held before, the same objects under the same names."""
import types

import pytest

from sparf_amd import camera, losses, metrics, pose_eval
from sparf_amd.patcher import Patcher


class _Base:
    def method(self):
        return "base"


class _Sub(_Base):
    def own(self):
        return "own"


def test_patcher_restores_what_each_object_itself_held():
    p = Patcher("pkg.mod.install", "uninstall")
    own, new = _Sub.__dict__["own"], lambda self: "new"
    module = types.SimpleNamespace(fn=len, other=1)
    obj = _Sub()
    assert p.original("method") is None
    p.guard()                                                    # nothing installed: no error
    p.put(_Sub, "own", new)
    p.put(_Sub, "method", new)                                   # inherited
    p.put(module, "fn", max)
    p.put(obj, "fresh", 3)                                       # shadowed nothing
    p.save("method", _Base.method)
    p.save("method", "a later one")                              # the first one saved stays
    assert obj.own() == obj.method() == "new" and module.fn is max and obj.fresh == 3 and p.original("method") is _Base.method
    with pytest.raises(RuntimeError) as e:
        p.guard()
    assert str(e.value) == "pkg.mod.install: already installed; call uninstall() first"
    p.restore()
    assert _Sub.__dict__["own"] is own and module.fn is len and vars(module) == dict(fn=len, other=1)
    assert "method" not in vars(_Sub) and _Sub.method is _Base.method and obj.method() == "base"
    assert "fresh" not in vars(obj) and not hasattr(obj, "fresh")
    assert p.originals == {} and p.patched == [] and p.original("method") is None
    p.restore()                                                  # a second one does nothing
    p.guard()
    assert _Sub.__dict__["own"] is own and "method" not in vars(_Sub)
    p.put(_Sub, "method", new)                                   # install, uninstall, install again
    p.restore()
    assert "method" not in vars(_Sub)


def test_patcher_restores_in_reverse_order():
    p = Patcher("pkg.mod.install", "uninstall")
    module = types.SimpleNamespace(fn=1)
    p.put(module, "fn", 2)
    p.put(module, "fn", 3)                                       # remembers the 2: only the reverse order brings the 1 back
    p.restore()
    assert module.fn == 1


def _cls(name, *bases, **attrs):
    return type(name, bases, {k: (lambda self, *a, _v=v, **kw: _v) for k, v in attrs.items()})


def _camera():
    lie, pose = _cls("Lie", se3_to_SE3=1)(), _cls("Pose", compose_pair_b_at_a=2, compose=3)()
    two = types.SimpleNamespace(r6d2mat=len, other=0)
    return (types.SimpleNamespace(lie=lie, pose=pose), two), (lie, pose, type(lie), type(pose), two)


def _corres():
    base = _cls("Base", compute_render_and_repro_loss_w_repro_thres=1)                      # the method is inherited
    cls = _cls("CorrespondencesPairRenderDepthAndGet3DPtsAndReproject", base, other=2)
    return (types.SimpleNamespace(CorrespondencesPairRenderDepthAndGet3DPtsAndReproject=cls),), (cls, base)


def _dcons():
    cls = _cls("DepthConsistencyLoss", compute_loss_at_sampled_pose=1)
    return (types.SimpleNamespace(DepthConsistencyLoss=cls),), (cls,)


def _photo():
    cls = _cls("BasePhotoandReguLoss", compute_loss=1)
    trainer, bare = types.SimpleNamespace(compute_mse_on_rays=len, other=1), types.SimpleNamespace()
    return (types.SimpleNamespace(BasePhotoandReguLoss=cls), trainer), (cls, trainer, bare)


def _photo_bare():
    (base, _), (cls, _, bare) = _photo()
    return (base, bare), (cls, bare)                                                        # a module without the name loses it again


def _sampler():
    base = _cls("CorrespondenceBasedLoss", compute_loss_pairwise=1, compute_loss_at_given_img_indexes=2, compute_loss_on_image_pair=3)
    pair = _cls("CorrespondencesPairRenderDepthAndGet3DPtsAndReproject", base)              # inherits all three
    return ((types.SimpleNamespace(CorrespondencesPairRenderDepthAndGet3DPtsAndReproject=pair), types.SimpleNamespace(CorrespondenceBasedLoss=base)),
            (base, pair))


def _colmap():
    cls = _cls("SparseCOLMAPDepthLoss", _cls("Parent", compute_loss=1))
    return (types.SimpleNamespace(SparseCOLMAPDepthLoss=cls),), (cls, cls.__mro__[1])


def _metrics():
    mod = types.SimpleNamespace(compute_metrics=len, compute_metrics_masked=max, ssim_loss=min, other=1)
    importing, unrelated = types.SimpleNamespace(compute_metrics=len, ssim_loss=min), types.SimpleNamespace(x=1)
    return (mod, importing, unrelated), (mod, importing, unrelated)


def _pose_eval():
    base = _cls("CommonPoseEvaluation", evaluate_camera_alignment=1, evaluate_any_poses=2)
    cls = _cls("Trainer", base, prealign_w2c_small_camera_systems=3)                        # one of its own, two inherited
    mods = (types.SimpleNamespace(backtrack_from_aligning_the_trajectory=len), types.SimpleNamespace(backtrack_from_aligning_the_trajectory=len, y=2),
            types.SimpleNamespace(x=1))
    return (cls, *mods), (cls, base, *mods)


PAIRS = {
    "camera": (camera.install, camera.uninstall, camera._installer, _camera),
    "losses": (losses.install, losses.uninstall, losses._corres, _corres),
    "depth_consistency": (losses.install_depth_consistency, losses.uninstall_depth_consistency, losses._dcons, _dcons),
    "photometric": (losses.install_photometric, losses.uninstall_photometric, losses._photo, _photo),
    "photometric_bare_module": (losses.install_photometric, losses.uninstall_photometric, losses._photo, _photo_bare),
    "sampler": (losses.install_sampler, losses.uninstall_sampler, losses._sampler, _sampler),
    "colmap_depth": (losses.install_colmap_depth, losses.uninstall_colmap_depth, losses._colmap, _colmap),
    "metrics": (metrics.install, metrics.uninstall, metrics._installer, _metrics),
    "pose_eval": (pose_eval.install, pose_eval.uninstall, pose_eval._installer, _pose_eval),
}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_install_then_uninstall_leaves_every_target_as_it_was(pair):
    install, uninstall, patcher, make = PAIRS[pair]
    args, targets = make()
    before = [dict(vars(t)) for t in targets]
    install(*args)
    try:
        assert [dict(vars(t)) for t in targets] != before and patcher.patched
        with pytest.raises(RuntimeError, match=r"^sparf_amd\.\w+\.%s: already installed; call %s\(\) first$" % (install.__name__, uninstall.__name__)):
            install(*args)
    finally:
        uninstall()
    for t, was in zip(targets, before):
        now = dict(vars(t))
        assert now.keys() == was.keys() and all(now[k] is was[k] for k in was), (pair, t)
    assert patcher.patched == [] and patcher.originals == {}
    uninstall()                                                  # a second one does nothing
    install(*args)                                               # and the pair can be used again
    uninstall()
    assert all(dict(vars(t)) == was for t, was in zip(targets, before))
