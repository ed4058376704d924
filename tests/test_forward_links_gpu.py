"""Every link of the fused MLP forward against float64 ON ITS OWN STORED OPERANDS (tests/forward_referee.py has the referees, their
float32 yardsticks and the derivation of every bound; tests/test_forward_referee_cpu.py tests the referee and its caps).

One training forward through the C ABI per case (ops.build_pass_fwd(..., save=True) + sparf_pass_forward); then, from the bytes that
run left in the save area and from sigma_raw / rgb_samples / raylen:
  E  encodings: the raw point / direction columns bit for bit, the padding slots 0, the sin / cos columns against float64 sin / cos of
     the restated fp32 argument, the view columns identical over the rows of a ray, raylen bit for bit
  L  layers 0-8: every stored layer output against relu(W_eff X + b) on the STORED layer input, the ReLU bits tied to the stored values
  O  sigma_raw (layer 7 row 0, unrounded) and rgb = sigmoid(layer 9) on the stored H6 / G
  I  the same inputs with save=False -- the *_infer kernel of the precision -- give bit-identical sigma_raw and rgb_samples (both
     instantiate the same fwd_layer chunk order)

Bounds (asserted as they stand; every yardstick is recomputed in the run):
  E  fp32 areas: each element within max(4 x yardstick's worst distance, 2^-24); bf16 areas: within one ulp_bf16, share off the rounded
     referee <= 8 x yardstick share + 16 / elements
  L  element-wise ulp_area(ref) + 2 (K + 2) 2^-24 (|W| |X| + |b|) (+ the tail term T in bf16x3); fp32: rel. L2 per layer <= 4 x yardstick;
     bf16 areas: share off the rounded referee <= 8 x yardstick share + 16 / elements, layers under 1e5 elements pooled, the bound itself
     <= 1e-3 (bf16) or <= 1/4 of the share a dropped tail product moves (bf16x3, whose yardstick carries its own tail)
  O  element-wise the accumulation bound (/ 4 behind the sigmoid, + the yardstick's worst sigmoid distance); rel. L2 <= 4 x yardstick
     where the output has 15 elements or more (case 1x2 has 2 and 6: the element-wise bound stands alone there, forward_referee.py
     "Small samples")

Cases: one partial wave (1x2, 3x5); a partial tile that is no multiple of 128 or 256 rows (70x24, also without c2f and with inverse
depths, where the sin / cos arguments are orders of magnitude larger); many tiles in one round (333x64); and two row counts taken
from the device's CU count that make the persistent loop turn: `rounds` = 6 CUs x 64 (3 rounds of 128-row tiles, 1.5 of 256-row tiles:
some workgroups loop, some do not) and `ragged-rounds` = (11 CUs + 5) x 24 (a second round whose last tile has three full waves, one
24-row wave and waves wholly past the end: the clamped staging of the next tile's rows).  Both FAIL unless rows > tile rows x CUs.

Measured on an MI355X (256 CUs), worst over the cases from 1 680 rows up, kernel / yardstick (all 24 cases pass; `rounds` ran 98 304 rows,
`ragged-rounds` 67 704):
  fp32    E worst distance point 7.0e-8 / 7.0e-8, view 5.9e-8 / 5.9e-8 (the kernel's sincosf and torch's sin / cos give the same values)
          L rel. L2 per layer 2.3e-7 / 2.2e-7    O sigma_raw 3.2e-7 / 5.2e-7 (inverse depths; 2.3e-7 / 2.3e-7 otherwise), rgb 6.8e-8 / 5.0e-8
  bf16    E share off the referee point 9.9e-6 / 9.9e-6, view 3.0e-5 / 3.0e-5
          L share off the referee, all layers 3.0e-5 / 2.4e-5; worst single layer of 2.5e7 elements 2.7e-5 / 7.2e-6 (3.8 of the 8 allowed)
          O sigma_raw 1.1e-7 / 1.3e-7 (inverse depths; 7.2e-8 / 7.6e-8 otherwise), rgb 4.1e-8 / 4.3e-8
  bf16x3  E as bf16    L share, all layers 1.5e-3 / 1.3e-3, worst layer ratio 1.3 of the 8 allowed; a dropped tail product would move
          19 ... 23 % of the heads; sum T = 0.11 ... 0.14 of sum 2^-9 |W_hi| |X|
          O sigma_raw 2.9e-5 / 1.4e-5 (inverse depths, 2.1 of the 4 allowed; 1.1e-5 / 1.0e-5 otherwise), rgb 3.1e-6 / 3.7e-6
          (one tail unit: the resolution of a bf16x3 link, forward_referee.py "What the tail costs"; the CPU emulation gives the same figures)
  I       sigma_raw and rgb_samples of the inference kernels bit-identical to the training kernels' in all 24 cases.
"""
import ctypes

import pytest
import torch

from oracle import nerf_oracle as O
from sparf_amd import lib as L
from sparf_amd import ops
from tests import backward_referee as BR
from tests import forward_referee as FR
from tests.golden.recipe import small_opt, make_state_dict
from tests.test_hip_gpu import dev, make_scene, params_list

pytestmark = pytest.mark.gpu

CASES = ["1x2", "3x5", "70x24", "70x24-plain", "70x24-inverse", "333x64", "rounds", "ragged-rounds"]
PRECS = ["fp32", "bf16", "bf16x3"]


def _shape(case, lib):
    """-> (rays, samples, whether some workgroup must take a second tile)"""
    cus = BR.dgrad_plan(lib, 1)[1]
    if case == "rounds":                     # 1 536 x 64 = 98 304 rows on 256 CUs
        return 6 * cus, 64, cus
    if case == "ragged-rounds":              # 2 821 x 24 = 67 704 rows on 256 CUs = 264 full 256-row tiles + 120 rows
        return 11 * cus + 5, 24, cus
    R, N = (int(v) for v in case.split("-")[0].split("x"))
    return R, N, None


def _inputs(case, R, N, seed=5):
    d = dev()
    inverse = case.endswith("-inverse")
    opt = small_opt(barf_c2f=None if case.endswith("-plain") else [0.4, 0.7], nerf=dict(depth=dict(param="inverse" if inverse else "metric")))
    sd = make_state_dict(opt, 21, progress=0.55)
    center, dirs, jitter, _ = make_scene(R, N, seed)
    t = O.sample_depth(opt, 1, R, N, [1, 0] if inverse else [1.2, 5.2], "train", jitter)[0, :, :, 0].to(d).contiguous()
    plist = params_list(sd, d)
    c2f = ops.c2f_weights(sd["progress"].to(d), opt.barf_c2f, d)
    return center.to(d).contiguous(), dirs.to(d).contiguous(), t, plist, c2f


def _forward(prec_id, c, dr, t, packed, c2f, save):
    fa, out, area, keep = ops.build_pass_fwd(prec_id, c, dr, t, None, 0.0, False, packed, c2f, save)
    L.check(L.load().sparf_pass_forward(ctypes.byref(fa), L.stream_ptr(dev())), "fwd")
    torch.cuda.synchronize()
    return out, area, keep


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", CASES)
def test_forward_links(case, prec):
    lib = L.load()
    R, N, cus = _shape(case, lib)
    rows, tile_rows = R * N, FR.TILE_ROWS[prec]
    if cus is not None:
        assert rows > tile_rows * cus, f"{case}: {rows} rows are one round of {tile_rows}-row tiles on {cus} CUs: no workgroup takes a second tile"
    prec_id = L.PREC_IDS[prec]
    c, dr, t, plist, c2f = _inputs(case, R, N)
    packed = ops.pack_weights(plist, prec_id)
    out, save, keep = _forward(prec_id, c, dr, t, packed, c2f, True)
    tag = f"[{case} {R}x{N} {prec}]"
    fails, figures, state = FR.check_forward(prec, save, c, dr, t, c2f, plist, out["sigma_raw"], out["rgb_samples"], raylen=out["raylen"])
    # link I: the inference kernel on the same inputs
    out_i, _, keep_i = _forward(prec_id, c, dr, t, packed, c2f, False)
    for name, key in (("sigma_raw", "sigma_ref"), ("rgb_samples", "rgb_ref")):
        a, b = out[name].reshape(rows, -1), out_i[name].reshape(rows, -1)
        ne = _bits(a) != _bits(b)
        if bool(ne.any()):
            r, col = ne.nonzero()[0].tolist()
            want, bound, _ = state[key]
            inside = not bool(((b.double() - want).abs() > bound).any())
            fails.append(f"I {name}: inference differs from training at {int(ne.sum())} of {ne.numel()} values, max |diff| {float((a - b).abs().max()):.3e}; first: "
                         f"{FR.where_row(r, tile_rows)} column {col}: training {float(a[r, col])!r} inference {float(b[r, col])!r}; inference outputs "
                         f"{'inside' if inside else 'OUTSIDE'} link O's element-wise bound on the training run's stored operands")
    print(tag, FR.report(figures))
    assert not fails, tag + "\n" + "\n".join(fails)
    del state, save, keep, keep_i
    torch.cuda.empty_cache()
