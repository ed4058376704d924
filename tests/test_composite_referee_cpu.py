"""tests/composite_referee.py tested on its own, without a GPU:
  * the float64 closed forms (outputs and gradients) against float64 torch autograd of NeRF.composite as the oracle restates it;
  * the exact restatement of the resampler: its linspace is torch's to the last two units, it lies within the existing 1e-5 of oracle.sample_pdf
    on non-degenerate bins, and EVERY input of the case table satisfies the sum-order condition under which it is exact;
  * the float32 yardstick stays inside every element-wise bound at every case and setting;
  * every mutant -- a deliberately wrong float64 formula -- falls outside the element-wise bounds at every sample count that exercises it.
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import composite_referee as CR
from tests.golden.recipe import small_opt

SETTINGS = [(k,) for k in CR.OUT_KEYS] + [CR.OUT_KEYS]


def _op(N, white_bg):
    op = CR.composite_case(N)
    op["raylen"] = CR.raylen32(op["dirs"])
    op["white_bg"] = white_bg
    return op


@pytest.mark.parametrize("white_bg", [False, True])
@pytest.mark.parametrize("N", CR.COMPOSITE_N)
def test_closed_forms_match_float64_autograd(N, white_bg):
    op = _op(N, white_bg)
    gall = CR.composite_grads(N)
    opt = small_opt(nerf=dict(setbg_opaque=white_bg))
    for keys in SETTINGS:
        g = {k: gall[k] for k in keys}
        ray, dens, rgbs = (op[k].double()[None].requires_grad_(True) for k in ("dirs", "dens", "rgbs"))
        ref = O.composite(opt, ray, rgbs, dens, op["t"].double()[None, :, :, None])
        mine = CR.composite_eval(op, g, exact_sd=True)
        loss = 0.0
        for k in CR.OUT_KEYS:
            r = ref[k][0].reshape(mine[k].shape)
            assert CR.rel_l2(mine[k], r.detach()) < 1e-12, (N, k, CR.rel_l2(mine[k], r.detach()))
            if k in g:
                loss = loss + (r * g[k].double()).sum()
        loss.backward()
        for k, x in (("d_density", dens), ("d_rgb_samples", rgbs), ("d_dir", ray)):
            want = x.grad[0] if x.grad is not None else torch.zeros_like(x[0])        # (e.g. the colours under a depth loss)
            err = (mine[k] - want).abs()
            # element by element against the magnitude of the terms that form it (T_N = T_{j+1} - sum_{i>j} w_i and 1 - O are
            # cancellations that leave 1e-17 in float64 autograd as well): the closing interval's 1e10 and the inverse-depth rays'
            # 1e8 must not hide the other samples
            w, q, dist = mine["weights"], mine["_q"].abs(), mine["_dist"].abs()
            wq = w * q
            mag = mine["_Tn"] * q + torch.cat([wq[:, 1:], torch.zeros_like(wq[:, :1])], 1).flip(1).cumsum(1).flip(1) + (mine["_gA"].abs() * mine["all_cumulated"])[:, None]
            scale = dict(d_density=mag * dist, d_rgb_samples=(w * (mine["_gC"].abs().sum(1) + mine["_gU"].abs())[:, None])[:, :, None].expand(-1, -1, 3),
                         d_dir=((mag * dist * op["dens"].double()).sum(1) / op["raylen"].double() ** 2)[:, None] * op["dirs"].double().abs())[k]
            over = err > 1e-9 * scale
            assert not bool(over.any()), (N, keys, k, over.nonzero()[0].tolist(), float(err[over].max()), float(scale[over].min()))


def test_restated_linspace_is_torchs():
    """the symmetric form start + step i / end - step (steps - 1 - i) with one fp32 step.  torch's vectorised CPU kernel forms
    (start + step i0) + step lane inside a vector, one rounding more: equal to the last two units, bit for bit below a vector's length"""
    for a, b in ((1.2, 5.2), (1.0, 0.0), (0.5, 4.5)):
        for n in (2, 3, 4, 64, 65, 66, 129, 130, 131):
            mine, ref = CR.linspace32(a, b, n), torch.linspace(a, b, n).numpy()
            assert mine[0] == np.float32(a) and mine[-1] == np.float32(b)
            assert float(np.abs(mine.astype(np.float64) - ref).max()) <= 2 * 2.0 ** -23 * max(abs(a), abs(b)), (a, b, n)
            if n <= 4:
                assert np.array_equal(mine, ref), (a, b, n)


@pytest.mark.parametrize("rng", ["metric", "inverse"])
@pytest.mark.parametrize("grid", ["random", "det"])
@pytest.mark.parametrize("shape", CR.FINE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_is_exact_and_near_the_oracle(shape, grid, rng):
    Nc, Nf = shape
    w, tc, u, dmin, dmax, g = CR.fine_inputs(Nc, Nf, grid, rng)
    tf, merged, violations = CR.fine_restatement(w, tc, u, dmin, dmax)
    assert not violations, violations[:3]                     # the sum-order condition: no input may break it, none is skipped
    assert merged.shape == (w.shape[0], Nc + Nf) and bool((np.diff(merged, axis=1) >= 0).all())
    zero = CR.FINE_PATTERNS.index("zeros")
    assert np.array_equal(tf[zero], np.full(Nf, np.float32(dmax)))                          # all weights zero: every sample is dmax
    # against the reference's port, where a rounding of the cdf (a few units of 2^-24) moves the sample by less than the 1e-5:
    # (c_hi - c_lo) 1e-5 > 4 x 2^-22 |d_hi - d_lo|  ("non-degenerate bins")
    wt = torch.from_numpy(w)
    ref = O.sample_pdf(wt[None], Nc, Nf, [dmin, dmax], g)[0, :, :, 0].numpy()
    pdf = wt / (wt.sum(-1, keepdim=True) + 1e-6)
    cdf = torch.cat([torch.zeros(w.shape[0], 1), pdf.cumsum(-1)], dim=-1).numpy()
    bins = CR.linspace32(dmin, dmax, Nc + 1)
    checked = 0
    for r in range(w.shape[0]):
        idx = np.searchsorted(cdf[r], u, side="right")
        il, ih = np.maximum(idx - 1, 0), np.minimum(idx, Nc)
        ok = (cdf[r][ih] - cdf[r][il]).astype(np.float64) * 1e-5 > 4 * 2.0 ** -22 * np.abs(bins[ih] - bins[il]).astype(np.float64)
        checked += int(ok.sum())
        assert float(np.abs(tf[r] - ref[r])[ok].max(initial=0.0)) <= 1e-5, (r, CR.FINE_PATTERNS[r])
    assert checked >= Nf                                       # (the mask leaves at least a ray's worth of samples)


@pytest.mark.parametrize("white_bg", [False, True])
@pytest.mark.parametrize("N", CR.COMPOSITE_N)
def test_yardstick_stays_inside_the_bounds(N, white_bg):
    op = _op(N, white_bg)
    gall = CR.composite_grads(N)
    for keys in SETTINGS:
        g = {k: gall[k] for k in keys}
        ref = CR.composite_eval(op, g)
        yard = CR.composite_eval(op, g, dtype=torch.float32)
        bounds = CR.composite_bounds(op, ref)
        for k in CR.OUT_KEYS + CR.GRAD_KEYS:
            over = ~((yard[k].double() - ref[k]).abs() <= bounds[k])
            assert not bool(over.any()), (N, keys, k, over.nonzero()[0].tolist(), float((yard[k].double() - ref[k]).abs()[over].max()),
                                          float(bounds[k][over].min()))


@pytest.mark.parametrize("mutant", CR.MUTANTS)
def test_mutant_falls_outside_the_bounds(mutant):
    """element-wise: the relative L2 of a tensor is dominated by the closing interval's 1e10 and cannot see a thin ray"""
    passes = []
    for N in CR.MUTANT_N[mutant]:
        op = _op(N, True)
        g = CR.composite_grads(N)
        ref = CR.composite_eval(op, g)
        yard = CR.composite_eval(op, g, dtype=torch.float32)
        bounds = CR.composite_bounds(op, ref)
        bad = CR.composite_eval(op, g, mutant=mutant)
        fails, figures = [], {}
        for k in CR.OUT_KEYS + CR.GRAD_KEYS:
            CR.check(k, bad[k], ref[k], bounds[k], yard[k], fails, figures)
        if not any("element-wise" in f for f in fails):
            passes.append(N)
    assert not passes, f"mutant {mutant} passes the element-wise bounds at N = {passes}"
