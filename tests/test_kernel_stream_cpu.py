"""The compiled instruction stream of the two config-1 kernels of the bf16x3 mode (no GPU: code-object notes + disassembly of the
built translation units, tools/kernel_stream.py; a unit without a current object is compiled first, ~2 min each).

What is pinned, and where the numbers come from (DESIGN 3.2 "instruction stream"):
  * no scalar parked in VGPR lanes: .sgpr_spill_count = 0 and no v_readlane_b32 / v_writelane_b32 (before the weight-DMA offsets
    became literals: 502 / 185 spilled scalars, one reload in front of every DMA piece);
  * the work itself unchanged: MFMA count, LDS bytes, no scratch, no more registers than before, the same occupancy
    (forward: one wave per SIMD, all 512 registers; data gradient: two waves per SIMD, i.e. at most 256);
  * the non-MFMA instruction total and the s_nop count reached, as upper bounds (before: 16 251 / 1 111 and 8 330 / 999, counted the same way on the objects of the commit before; the data gradient keeps the wait state between a mask pop and its select).
The tile body is fully unrolled, so the static counts are per tile and wave."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FWD = "_ZN5sparf14mlp_fwd_kernelILi2ELi1EEEvNS_10MlpFwdArgsE"                                  # mlp_fwd_kernel<PREC_X3, 1>
DGRAD = "_ZN5sparf14mlp_bwd_kernelILi2ELb0ENS_14PolicyX3DgradTILi8EEELb0EEEvNS_10MlpBwdArgsE"  # mlp_bwd_kernel<PREC_X3, false, PolicyX3DgradT<8>, false>
DGRAD_POSE = "_ZN5sparf14mlp_bwd_kernelILi2ELb1ENS_14PolicyX3DgradTILi8EEELb0EEEvNS_10MlpBwdArgsE"


@pytest.fixture(scope="module")
def stream():
    spec = importlib.util.spec_from_file_location("kernel_stream", os.path.join(ROOT, "tools", "kernel_stream.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def figs(stream):
    m = stream
    out = {}
    for unit in m.MLP_UNITS:
        for k, f in m.figures(unit).items():
            out[k] = out[(unit, k)] = f          # (mlp_bwd_q8.hip and mlp_bwd_x3.hip hold kernels of the same template: keyed by unit too)
            print(unit, k, f)
    return out


def _no_parked_scalars(f):
    assert f["sgpr_spill_count"] == 0, f
    assert f["v_readlane_b32"] == 0 and f["v_writelane_b32"] == 0, f
    assert f["private_segment_fixed_size"] == 0, f


def test_forward_stream(figs):
    f = figs[FWD]
    _no_parked_scalars(f)
    assert f["mfma"] == 3168, f
    assert f["group_segment_fixed_size"] == 131904, f
    assert f["vgpr_count"] <= 367 and f["vgpr_count"] > 256, f        # (arch + accumulator registers; one wave per SIMD either way)
    assert f["other"] <= 14174, f
    assert f["s_nop"] <= 200, f


def test_dgrad_stream(figs):
    f = figs[DGRAD]
    _no_parked_scalars(f)
    assert f["mfma"] == 1944, f
    assert f["group_segment_fixed_size"] == 65600, f
    assert f["vgpr_count"] <= 238 and f["agpr_count"] == 0, f         # two waves per SIMD
    assert f["other"] <= 7692, f
    assert f["s_nop"] <= 746, f


def test_pose_dgrad_stream(figs):
    """the other kernel of the unit (8 waves at the 256-register limit): no parked scalars, no scratch, not more registers than before (250)"""
    f = figs[DGRAD_POSE]
    _no_parked_scalars(f)
    assert f["mfma"] == 2088, f
    assert f["group_segment_fixed_size"] == 131136, f
    assert f["vgpr_count"] <= 250 and f["agpr_count"] == 0, f
    assert f["other"] <= 8665, f                                      # (before: 9 362 / 1 188)
    assert f["s_nop"] <= 973, f


# Every kernel built from mlp_dev.h + mlp_fwd_impl.h / mlp_bwd_impl.h: (registers before, registers allowed, scratch bytes allowed,
# parked scalars allowed).  "Allowed" registers = the figure before, except for three 8-wave kernels which the register allocator
# gives 1-3 more once their 76-189 parked scalars are gone: pinned at the figure reached, below the 256 that two
# waves per SIMD need.  Scratch: the figure reached (before: 24 / 24 / 0 everywhere else).  Parked scalars: none, except 22 that
# the fp32 training forward keeps (505 before).
_FWD = "_ZN5sparf14mlp_fwd_kernelILi%dELi%dEEEvNS_10MlpFwdArgsE"
_BWD = "_ZN5sparf14mlp_bwd_kernelILi%dELb%dENS_6PolicyILi%dEEELb%dEEEvNS_10MlpBwdArgsE"
_BWX = "_ZN5sparf14mlp_bwd_kernelILi2ELb%dENS_14PolicyX3DgradTILi%dEEELb%dEEEvNS_10MlpBwdArgsE"
ALL_KERNELS = {
    ("mlp_fwd_fp32_train.hip", _FWD % (1, 1)): (332, 332, 0, 22),
    ("mlp_fwd_fp32_infer.hip", _FWD % (1, 0)): (341, 341, 0, 0),
    ("mlp_fwd_x3_train.hip", _FWD % (2, 1)): (367, 367, 0, 0),
    ("mlp_fwd_x3_train_q8.hip", _FWD % (2, 2)): (372, 372, 0, 0),
    ("mlp_fwd_x3_infer.hip", _FWD % (2, 0)): (358, 358, 0, 0),
    ("mlp_fwd_bf16_train.hip", _FWD % (0, 1)): (256, 256, 8, 0),
    ("mlp_fwd_bf16_train_q8.hip", _FWD % (0, 2)): (256, 256, 16, 0),
    ("mlp_fwd_bf16_infer.hip", _FWD % (0, 0)): (254, 254, 0, 0),
    ("mlp_bwd.hip", _BWD % (0, 1, 0, 0)): (239, 240, 0, 0),
    ("mlp_bwd.hip", _BWD % (0, 0, 0, 0)): (217, 217, 0, 0),
    ("mlp_bwd_fp32.hip", _BWD % (1, 1, 1, 0)): (456, 456, 0, 0),
    ("mlp_bwd_fp32.hip", _BWD % (1, 0, 1, 0)): (445, 445, 0, 0),
    ("mlp_bwd_x3.hip", _BWX % (1, 8, 0)): (250, 250, 0, 0),
    ("mlp_bwd_x3.hip", _BWX % (0, 8, 0)): (238, 238, 0, 0),
    ("mlp_bwd_x3w4.hip", _BWX % (1, 4, 0)): (308, 308, 0, 0),
    ("mlp_bwd_x3w4.hip", _BWX % (0, 4, 0)): (244, 244, 0, 0),
    ("mlp_bwd_q8.hip", _BWD % (0, 1, 0, 1)): (238, 240, 0, 0),
    ("mlp_bwd_q8.hip", _BWD % (0, 0, 0, 1)): (219, 219, 0, 0),
    ("mlp_bwd_q8.hip", _BWX % (1, 8, 1)): (252, 252, 0, 0),
    ("mlp_bwd_q8.hip", _BWX % (0, 8, 1)): (241, 244, 0, 0),
}


def test_every_mlp_kernel_keeps_its_registers_and_parks_no_scalars(figs):
    seen = {k for k in figs if isinstance(k, tuple)}
    assert seen == set(ALL_KERNELS), seen ^ set(ALL_KERNELS)
    bad = {}
    for key, (_, vgpr, scratch, parked) in ALL_KERNELS.items():
        f = figs[key]
        waves2 = f["agpr_count"] == 0                                   # the 8-wave kernels: two waves per SIMD
        if not (f["vgpr_count"] <= vgpr and (not waves2 or f["vgpr_count"] <= 256) and f["private_segment_fixed_size"] <= scratch
                and f["sgpr_spill_count"] <= parked):
            bad[key] = f
    assert not bad, bad


def test_every_kernel_instance_is_compiled_once_and_the_dispatch_unit_holds_none(stream, figs, tmp_path):
    """csrc/kernels.h lists the instances of mlp_fwd_kernel / mlp_bwd_kernel, each unit instantiates its own explicitly, and the dispatch
    unit looks the launchers up without seeing the templates' definitions.  A definition that becomes visible where it should not
    compiles kernels a second time -- silently, and for many minutes."""
    d = str(tmp_path)
    owners = {}
    for unit, k in (key for key in figs if isinstance(key, tuple)):
        owners.setdefault(k, []).append(unit)
    for unit in stream.B.RAYS_UNITS:
        for k in stream.notes_of(stream.code_object(stream.object_of(unit, d), d)):
            owners.setdefault(k, []).append(unit)
    assert set(stream.MLP_UNITS) | set(stream.B.RAYS_UNITS) == set(stream.B.FUSED_UNITS)
    assert all("mlp_fwd_kernel" in k or "mlp_bwd_kernel" in k for k in owners), owners
    assert len(owners) == len(ALL_KERNELS) + len(stream.B.RAYS_UNITS), sorted(owners)        # (a ray-gradient-only unit holds one kernel)
    assert all(len(units) == 1 for units in owners.values()), {k: u for k, u in owners.items() if len(u) != 1}
    with pytest.raises(subprocess.CalledProcessError):                                        # no gfx950 code object in it at all
        stream.code_object(stream.object_of(stream.B.MLP_DISPATCH, d), d)
