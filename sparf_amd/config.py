"""Option tree for the renderer hot path.

Mirrors the keys the reference renderer reads, with the
defaults of /root/reference/train_settings/default_config.py:88-127 (LLFF-type)
and :247-272 (360-type data: metric depth, 1024 rays).  Reference
`train_settings/*` configs can be passed to `Graph` unchanged; this module only
exists so tests/bench/smoke can build an `opt` without the reference tree.
"""
import os
from collections import namedtuple

from .edict import EasyDict as edict, opt_get

DEFAULT_PRECISION = "bf16x3"         # the ONE default: what an unmodified run_trainval.py gets, and what bench.py measures
DEFAULT_FAR_SAMPLES = 8
DEFAULT_FAR_DEPTH = 8.0


# default; env: the environment variable that also sets the key; parse: what turns the option's / the variable's value into the key's
# type; env_wins: the variable overrides the option (A/B runs of an unmodified trainer)
HipKey = namedtuple("HipKey", "default env parse env_wins", defaults=(None, None, False))


# The opt.hip.* keys of this renderer: everything that changes what a render computes or leaves behind (the reference's settings files
# have no opt.hip: an absent key is its default).  hip_option is their one reader; what they mean is said where they are read.
#   precision, inverse_depth_precision, far_samples, far_depth: frequency_nerf.precision_name / pass_precision
#   fused_rays, fused_render, lazy_batch, device_rng: renderer.Graph (_rays, _render_fused, _render_deferred, _grid_midpoints)
#   test_optim_rays_only: renders with mode == "test-optim" (the reference's test-time pose optimisation, joint_pose_nerf_trainer.py:381-406,
#       whose optimiser holds nothing but the pose refinement) treat both networks as frozen: ray-gradient-only passes (ops.save_kind),
#       no weight gradient.  Off by default: the unmodified loop never freezes the networks, and with the option on their `.grad` no longer
#       receive what that loop accumulates into them (nothing in it reads them).
HIP_KEYS = dict(
    precision=HipKey(DEFAULT_PRECISION, "SPARF_PRECISION"),
    inverse_depth_precision=HipKey("routed", "SPARF_INVERSE_DEPTH_PRECISION"),
    far_samples=HipKey(DEFAULT_FAR_SAMPLES, "SPARF_FAR_SAMPLES", int),
    far_depth=HipKey(DEFAULT_FAR_DEPTH, "SPARF_FAR_DEPTH", float),
    fused_rays=HipKey(True),
    fused_render=HipKey(True),
    lazy_batch=HipKey(True, "SPARF_LAZY_BATCH", lambda s: s != "0", env_wins=True),
    device_rng=HipKey(False),
    test_optim_rays_only=HipKey(False),
)
HIP_DEFAULTS = {k: v.default for k, v in HIP_KEYS.items()}


def hip_env(*keys):
    """the environment variables of `keys` as they are set now, for a reader that must not see later changes (hip_option(env=))"""
    return {v: os.environ[v] for v in (HIP_KEYS[k].env for k in keys) if v in os.environ}


def hip_option(opt, key, env=os.environ):
    """The value of opt.hip.<key> (HIP_KEYS).  A key without an environment variable: the option if the tree has it, else the default.
    One with a variable: the option if it is truthy, else the variable if it is truthy, else the default (far_samples = 0 falls
    through), parsed -- unless the variable wins: then the variable if it is set, else the option if the tree has it, else the default."""
    k = HIP_KEYS[key]
    hip = opt_get(opt, "hip") or {}
    raw = env.get(k.env) if k.env is not None else None
    if k.env is None or k.env_wins:
        return opt_get(hip, key, k.default) if raw is None else k.parse(raw)
    val = opt_get(hip, key) or raw or k.default
    return val if k.parse is None else k.parse(val)


def default_opt(**over):
    o = edict()
    o.max_iter = 200000
    o.mask_img = False
    o.barf_c2f = None
    o.arch = edict(
        layers_feat=[None, 256, 256, 256, 256, 256, 256, 256, 256],
        layers_feat_fine=None,
        layers_rgb=[None, 128, 3],
        skip=[4],
        density_activ="softplus",
        tf_init=True,
        posenc=edict(include_pi_in_posenc=True, add_raw_3D_points=True, add_raw_rays=True,
                     log_sampling=True, L_3D=10, L_view=4),
    )
    o.nerf = edict(
        view_dep=True,
        depth=edict(param="metric", range=[1, 0]),
        sample_intvs=128,
        sample_stratified=True,
        fine_sampling=False,
        sample_intvs_fine=128,
        rand_rays=1024,
        density_noise_reg=False,
        setbg_opaque=False,
    )
    o.camera = edict(model="perspective", ndc=False)
    _merge(o, over)
    return o


def _merge(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            dst[k] = v


def baseline_opt(config=1, **over):
    """BASELINE.json configs: 0 = 256 rays / 64 coarse (+128 fine) CPU case,
    1 = 4096 rays x (64+128), both `nerf_training_w_gt_poses/dtu/nerf.py`
    (fine_sampling, density_noise_reg=True, metric depth, no c2f);
    2 = joint pose/BARF c2f [0.4, 0.7] (`joint_pose_nerf_training/dtu/barf.py`)."""
    base = dict(nerf=dict(fine_sampling=True, sample_intvs=64, sample_intvs_fine=128,
                          density_noise_reg=True, depth=dict(param="metric")))
    if config == 0:
        base["nerf"]["rand_rays"] = 256
    elif config == 1:
        base["nerf"]["rand_rays"] = 4096
    elif config == 2:
        base["nerf"]["rand_rays"] = 4096
        base["nerf"]["density_noise_reg"] = False
        base["barf_c2f"] = [0.4, 0.7]
    else:
        raise ValueError(config)
    o = default_opt(**base)
    _merge(o, over)
    return o
