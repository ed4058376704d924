"""sample_fine_kernel (csrc/ray_ops.hip) BIT FOR BIT against its exact numpy restatement, at the coarse / fine sample counts where its
64-sample chunks, the fp64 cdf carry and the power-of-two sort buffer can go wrong (tests/composite_referee.py has the restatement, the
sum-order condition under which it is exact and the case tables; tests/test_composite_referee_cpu.py tests it without a GPU).

  * t_fine and the merged output, from the device grid, the host grid (launch arguments), device ranges and floats;
  * nine weight patterns per call, one ray each: gamma-distributed, one-hot at bin 0 / 63 / 64 / Nc - 1, all zero (every sample = dmax),
    a zero plateau over bins 60 ... 70, a total of 1e-7 (the denominator's 1e-6 dominates, most u fall past cdf[-1]);
  * the random and the deterministic grid, the metric call and the inverse-depth call (range [1, 0], t_coarse descending);
  * (Nc, Nf) of FINE_SHAPES: Nt an exact power of two (no +inf padding) and one past it, Nf > 256 (the device-grid path), Nc across one
    and two chunks;
  * a shape past the launcher's 64 KiB LDS check raises SparfError without a launch.
Measured on an MI355X: bit-identical in all nine shapes, every pattern, grid, range and entry point.

The compositing parts of the same referee (stand-alone compositing at N = 2 ... 192 and the compositing links of a pass) have no GPU
test yet: against the referee composite_fwd_kernel misses the element-wise bound of the LAST weight of a ray (the exclusive sum formed
as incl - sd in fp64 keeps the prefix only to 2^-53 sd behind the closing interval, sd = density x 1e10 x |ray|: 4e-5 relative at
N = 2, 2e-4 at N = 192, bound 4e-7 ... 2e-6), and the fix moves the last-sample operands of tests/test_backward_links_gpu.py's
hybrid fp32 case, whose link A statistic then sits at 4.10 x its yardstick instead of below 4.  DESIGN.md 2 has the figures.
"""
import pytest
import torch

from sparf_amd import lib as L
from sparf_amd import ops
from tests import composite_referee as CR

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def dev():
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------------------------------- part S
def _same_bits(got, want, what, fails):
    got = got.cpu()
    if not torch.equal(got, want):
        ne = (got != want) | (got.isnan() != want.isnan())
        r, i = ne.nonzero()[0].tolist()
        fails.append(f"{what}: {int(ne.sum())} of {ne.numel()} values differ; first: ray {r} ({CR.FINE_PATTERNS[r]}) sample {i}: "
                     f"got {float(got[r, i])!r} want {float(want[r, i])!r}")


@pytest.mark.parametrize("shape", CR.FINE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sample_fine_bit_for_bit(shape):
    Nc, Nf = shape
    fails = []
    for grid in ("random", "det"):
        for rng in ("metric", "inverse"):
            w, tc, u, dmin, dmax, _ = CR.fine_inputs(Nc, Nf, grid, rng)
            tf, merged, violations = CR.fine_restatement(w, tc, u, dmin, dmax)
            assert not violations, violations[:3]
            tag = f"[{Nc}x{Nf} {grid} {rng}]"
            wd, tcd, ud = T(w).to(dev()), T(tc).to(dev()), T(u).to(dev())
            out_d, tf_d = ops.sample_fine(wd, tcd, ud, dmin, dmax, want_unsorted=True)
            _same_bits(tf_d, T(tf), f"{tag} t_fine, device grid", fails)
            _same_bits(out_d, T(merged), f"{tag} merged output, device grid", fails)
            out_n, tf_n = ops.sample_fine(wd, tcd, ud, dmin, dmax, want_unsorted=False)
            assert tf_n is None
            _same_bits(out_n, out_d.cpu(), f"{tag} merged output without t_fine", fails)
            if Nf <= 256:                                      # the grid in the launch arguments (sparf_sample_fine_hostgrid)
                out_h, tf_h = ops.sample_fine(wd, tcd, T(u), dmin, dmax, want_unsorted=True)
                _same_bits(tf_h, tf_d.cpu(), f"{tag} t_fine, host grid against device grid", fails)
                _same_bits(out_h, out_d.cpu(), f"{tag} merged output, host grid against device grid", fails)
            rd = torch.tensor([dmin, dmax], dtype=torch.float32, device=dev())
            out_r, tf_r = ops.sample_fine(wd, tcd, ud, 7.0, -3.0, want_unsorted=True, range_dev=rd)     # (the floats are overridden)
            _same_bits(tf_r, tf_d.cpu(), f"{tag} t_fine, range_dev against floats", fails)
            _same_bits(out_r, out_d.cpu(), f"{tag} merged output, range_dev against floats", fails)
    assert not fails, "\n".join(fails)


def test_sample_fine_refuses_what_exceeds_the_lds():
    """Nc + Nf = 8193 sorts in a 16384-float buffer: with the cdf that is past the launcher's 64 KiB check -> SparfError, nothing launched"""
    Nc, Nf = 4097, 4096
    w = torch.full((1, Nc), 0.25, device=dev())
    tc = torch.linspace(1.2, 5.2, Nc, device=dev())[None].contiguous()
    u = torch.linspace(0.01, 0.99, Nf, device=dev())
    out = torch.full((1, Nc + Nf), -7.0, device=dev())
    with pytest.raises(L.SparfError):
        ops.sample_fine(w, tc, u, 1.2, 5.2, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
