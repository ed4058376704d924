"""The opt.hip keys that have an environment variable, through the public readers (frequency_nerf.precision_name / pass_precision,
Graph's deferral of render calls): which of option, environment and default wins.  Precedence is behaviour: for precision,
inverse_depth_precision, far_samples and far_depth a truthy option wins, else a truthy environment value, else the default (far_samples = 0
falls through); $SPARF_LAZY_BATCH, read once when the Graph is constructed, overrides opt.hip.lazy_batch."""
import itertools

import pytest
import torch

from sparf_amd import lib as L
from sparf_amd.config import default_opt
from sparf_amd.frequency_nerf import DEFAULT_FAR_DEPTH, DEFAULT_FAR_SAMPLES, DEFAULT_PRECISION, pass_precision, precision_name
from tests.glue_fake import fake  # noqa: F401  (the stand-in library, as a fixture)

ENV = ("SPARF_PRECISION", "SPARF_INVERSE_DEPTH_PRECISION", "SPARF_FAR_SAMPLES", "SPARF_FAR_DEPTH", "SPARF_LAZY_BATCH")
ABSENT = object()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _opt(**hip):
    """inverse depth (what the three routing keys are read under); keys given as ABSENT are left out of opt.hip"""
    return default_opt(nerf=dict(depth=dict(param="inverse")), hip={k: v for k, v in hip.items() if v is not ABSENT})


def _cross(monkeypatch, var, options, env_value):
    for option, env in itertools.product(options, (None, env_value)):
        if env is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, env)
        yield option, env


def test_no_opt_hip_at_all_is_every_default():
    opt = default_opt(nerf=dict(depth=dict(param="inverse")))
    assert "hip" not in opt and precision_name(opt) == DEFAULT_PRECISION == "bf16x3"
    assert pass_precision(opt, 64) == (L.PREC_X3, (DEFAULT_FAR_SAMPLES, L.PREC_FP32))
    with torch.no_grad():
        assert pass_precision(opt, None, to_max_samples=64) == (L.PREC_X3, (DEFAULT_FAR_DEPTH, L.PREC_FP32))


def test_precision(monkeypatch):
    for option, env in _cross(monkeypatch, "SPARF_PRECISION", (ABSENT, None, "", "fp32"), "bf16"):
        assert precision_name(_opt(precision=option)) == ("fp32" if option == "fp32" else env or "bf16x3"), (option, env)
    monkeypatch.setenv("SPARF_PRECISION", "fp64")
    with pytest.raises(ValueError, match=r"unknown precision 'fp64' \(choose from \['bf16', 'bf16\+q8', 'bf16x3', 'bf16x3\+q8', 'fp32'\]\)"):
        precision_name(_opt())
    with pytest.raises(ValueError, match="unknown precision 'half'"):
        precision_name(_opt(precision="half"))


def test_inverse_depth_precision(monkeypatch):
    routed = (L.PREC_X3, (8, L.PREC_FP32))
    want = {"fp32": (L.PREC_FP32, None), "bf16x3": (L.PREC_X3, None), None: routed}
    for option, env in _cross(monkeypatch, "SPARF_INVERSE_DEPTH_PRECISION", (ABSENT, None, "", "fp32"), "bf16x3"):
        assert pass_precision(_opt(inverse_depth_precision=option), 64) == want[option if option == "fp32" else env], (option, env)
    monkeypatch.setenv("SPARF_INVERSE_DEPTH_PRECISION", "exact")
    with pytest.raises(ValueError, match=r"opt.hip.inverse_depth_precision must be 'routed', 'fp32' or 'bf16x3', not 'exact'"):
        pass_precision(_opt(), 64)


def test_far_samples(monkeypatch):
    for option, env in _cross(monkeypatch, "SPARF_FAR_SAMPLES", (ABSENT, None, 0, 3), "5"):
        K = 3 if option == 3 else 5 if env else 8             # (0 is falsy: it falls through)
        assert pass_precision(_opt(far_samples=option), 64) == (L.PREC_X3, (K, L.PREC_FP32)), (option, env)
    assert pass_precision(_opt(far_samples=3), 3) == (L.PREC_X3, (2, L.PREC_FP32))           # at most the coarse sample count - 1


def test_far_depth(monkeypatch):
    with torch.no_grad():
        for option, env in _cross(monkeypatch, "SPARF_FAR_DEPTH", (ABSENT, None, 0, 4.0), "6.5"):
            thr = 4.0 if option == 4.0 else 6.5 if env else 8.0
            got = pass_precision(_opt(far_depth=option), None, to_max_samples=64)
            assert got == (L.PREC_X3, (thr, L.PREC_FP32)) and isinstance(got[1][0], float), (option, env)


def test_lazy_batch_environment_beats_the_option_and_is_read_at_construction(fake, monkeypatch):
    """a train-mode call on an explicit ray list under autograd is deferred (a PendingRender) or not"""
    from sparf_amd import frequency_nerf, renderer
    from sparf_amd.edict import EasyDict as edict
    from tests.golden.recipe import ring_cameras, small_opt
    for mod in (renderer, frequency_nerf):
        monkeypatch.setattr(mod, "max_rows_per_call", lambda prec=None, device=None, need=None, far=None: 1 << 20)
    H, W = 6, 8
    pose, intr = ring_cameras(1, H=H, W=W)
    data = edict(depth_range=torch.tensor([[1.2, 5.2]]))

    def deferred(opt, graph):
        ret = graph.render_image_at_specific_pose_and_rays(opt, data, pose[0], intr[0], H, W, iter=0, ray_idx=torch.arange(6), mode="train")
        graph._pending = None                            # (dropped unread: nothing is to be launched here)
        return isinstance(ret, renderer.PendingRender)

    for option, env in itertools.product((ABSENT, True, False), (None, "0", "1", "yes")):
        if env is None:
            monkeypatch.delenv("SPARF_LAZY_BATCH", raising=False)
        else:
            monkeypatch.setenv("SPARF_LAZY_BATCH", env)
        opt = small_opt(hip={} if option is ABSENT else dict(lazy_batch=option))
        graph = renderer.Graph(opt, torch.device("cpu"))
        want = (option is not False) if env is None else env != "0"
        assert deferred(opt, graph) == want, (option, env)
        # the variable was read when the Graph was constructed: changing it now changes nothing
        monkeypatch.setenv("SPARF_LAZY_BATCH", "0" if want else "1")
        assert deferred(opt, graph) == want, (option, env)
