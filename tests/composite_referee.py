"""Float64 referees of the per-ray kernels of csrc/ray_ops.hip -- composite_fwd_kernel, composite_bwd_kernel, sample_fine_kernel --
on the operands the kernels themselves read, with their float32 yardsticks, element-wise bounds, case tables and mutants.

All three kernels give one 64-lane wavefront to one ray and walk the samples in chunks of 64 with an fp64 carry between chunks; several
values are picked out by index (T at N-2, the parked T at N-3, the start of the reverse loop ((N-1)/64)*64, the `lane < 63` mask of the
suffix, the cdf carry).  The sample counts of the case tables are the smallest at which each of these rules can go wrong.

Part S, resampling.  Every operation of sample_fine_kernel is a correctly rounded fp32 + - x / or a double sum rounded once to fp32, so
`fine_restatement` restates it EXACTLY in numpy:
    denom = fl32(fl32(sum64 w) + 1e-6f), pdf = fl32(w / denom), cdf_k = fl32(sum64_{i<k} pdf_i), idx = searchsorted(cdf, u, right),
    bins = torch's symmetric linspace, frac = fl32(fl32(u - c_lo) / fl32(fl32(c_hi - c_lo) + 1e-8f)), tf = fl32(d_lo + fl32(frac fl32(d_hi - d_lo))),
    merged = sort(cat(t_coarse, tf)).
The restatement is exact only where the order of a double sum cannot change its rounded fp32 value; that is a condition on the INPUTS:
every sum is formed sequentially in double and with math.fsum, and the case is in violation if the two round to different fp32 values
(`fine_restatement` returns the violations; the tests assert that there is none; weights on a 2^-20 grid, or 2^-40 for the tiny-total
pattern, satisfy it: their double sums are exact).

Part C, compositing.  The kernel forms sd = fl32(dens fl32(delta ell)) in fp32; that is restated exactly.  From sd on the referee is
float64: T_i = exp(-sum_{k<i} sd_k), alpha = 1 - exp(-sd), w = T alpha, the seven outputs of NeRF.composite and the closed-form gradients
of the kernel's header comment (`composite_eval`, which is also the YARDSTICK when run in float32 and, with `mutant=`, a deliberately
wrong formula).  With u = 2^-24 and every expf taken as within 2 units of fp32's last place (E = 4u relative; the device's and the CPU's
are specified to 1), the kernel's rounding steps give, to first order (`composite_bounds`; 5 % slack covers the second order):
    T      excl is rounded to fp32 before expf:           eT_i = T_i (u excl_i + E) + 2^-126        (also T_{i+1} of the backward, with incl)
    alpha  1 - expf(-sd):                                  eA_i = E exp(-sd_i) + u alpha_i
    w      T alpha:                                        bw_i = eT_i alpha_i + T_i eA_i + u w_i + 2^-126
    dots   any order of fp32 sums of n terms:              |sum_hat - sum| <= sum_i (term error) + (n + 2) u sum_i |term_i|
    q      <= 12 roundings over its terms' magnitudes + what the errors of the ray's own D, O, SC (fp32 dots of the stored w) move
    ds     eT_{j+1} |q_j| + T_{j+1} bq_j + sum_{k>j} (bw_k |q_k| + w_k bq_k) + u (|T q| + 2 |suffix|) + |gA| (eT_{N-2} + u A)
    d_density_j = ds_j delta_j ell:   bound = (bds_j + 2 u |ds_j|) |delta_j ell|  -- PER SAMPLE: the factor is 1e10 on the closing interval
Next to the element-wise bound: relative L2 per output <= 4 x the yardstick's own distance to the referee (the factor of the two link
tests); rgb_var, a cancellation residue, is measured against max(|ref|, 1), the floor tests/test_abi6_gpu.py gives it.

Failure strings name ray and sample; `report` prints kernel / yardstick figures.

Part S runs on the GPU in tests/test_composite_links_gpu.py.  Part C is tested here on the CPU only (tests/test_composite_referee_cpu.py:
closed forms against float64 autograd, yardstick inside every bound, every mutant outside); the docstring of
tests/test_composite_links_gpu.py says what its GPU tests found and why they are not in the suite yet.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24                     # unit roundoff of fp32
EXPF = 4.0 * U                     # relative error allowed to one expf: 2 units in the last place
TINY = 2.0 ** -126                 # smallest normal fp32: what a flushed or underflowed product can lose
SLACK = 1.05                       # second-order terms of the first-order bounds
L2_FACTOR = 4.0

COMPOSITE_N = [2, 3, 63, 64, 65, 66, 67, 128, 129, 130, 192]
FINE_SHAPES = [(2, 1), (63, 1), (64, 64), (64, 128), (65, 63), (65, 64), (128, 128), (129, 127), (130, 300)]
#   (64,64), (129,127): Nt an exact power of two, no +inf padding; (65,64): Nt = 129, one past a power of two; (130,300): Nf > 256, the
#   device-grid path; Nc crosses one and two chunks
OUT_KEYS = ("rgb", "depth", "opacity", "weights", "depth_var", "rgb_var", "all_cumulated")
GRAD_KEYS = ("d_density", "d_rgb_samples", "d_dir")
F32 = np.float32


# ======================================================================================================================= part S
def linspace32(start, end, steps):
    """torch.linspace(start, end, steps) in float32 as the CPU kernel (and ray_ops.hip linspace_at) computes it: the symmetric form"""
    start, end = F32(start), F32(end)
    step = F32(F32(end - start) / F32(steps - 1))
    i = np.arange(steps)
    lo = (start + (step * i.astype(F32)).astype(F32)).astype(F32)
    hi = (end - (step * (steps - i - 1).astype(F32)).astype(F32)).astype(F32)
    return np.where(i < steps // 2, lo, hi).astype(F32)


def _sum64(x, what, violations):
    """double sum of float32 values rounded once to fp32; records a violation if the summation order can change that value"""
    seq = 0.0
    for v in x:
        seq += float(v)
    fs = math.fsum(float(v) for v in x)
    if F32(seq) != F32(fs):
        violations.append(f"{what}: sequential double sum {seq!r} and math.fsum {fs!r} round to different fp32 values")
    return F32(fs)


def fine_restatement(w, tc, u, dmin, dmax):
    """w, tc [R, Nc] float32, u [Nf] float32 (the grid's interval mid-points), dmin, dmax: floats (rounded to fp32 as the C call does)
    -> (t_fine [R, Nf], merged [R, Nc + Nf], violations of the sum-order condition: list of str)"""
    w, tc, u = np.asarray(w, F32), np.asarray(tc, F32), np.asarray(u, F32)
    R, Nc = w.shape
    bins = linspace32(dmin, dmax, Nc + 1)
    tf = np.empty((R, u.size), F32)
    violations = []
    for r in range(R):
        tot = _sum64(w[r], f"ray {r} total", violations)
        denom = F32(tot + F32(1e-6))
        pdf = (w[r] / denom).astype(F32)
        seq = np.concatenate([[0.0], np.cumsum(pdf.astype(np.float64))])                     # numpy's cumsum is sequential
        cdf = np.zeros(Nc + 1, F32)
        for k in range(1, Nc + 1):
            cdf[k] = F32(math.fsum(float(v) for v in pdf[:k]))
            if cdf[k] != F32(seq[k]):
                violations.append(f"ray {r} cdf[{k}]: sequential double sum and math.fsum round to different fp32 values")
        idx = np.searchsorted(cdf, u, side="right")
        il, ih = np.maximum(idx - 1, 0), np.minimum(idx, Nc)
        cl, ch, dl, dh = cdf[il], cdf[ih], bins[il], bins[ih]
        frac = ((u - cl).astype(F32) / ((ch - cl).astype(F32) + F32(1e-8)).astype(F32)).astype(F32)
        tf[r] = (dl + (frac * (dh - dl).astype(F32)).astype(F32)).astype(F32)
    return tf, np.sort(np.concatenate([tc, tf], axis=1), axis=1), violations


FINE_PATTERNS = ("gamma", "hot0", "hot63", "hot64", "hot_last", "zeros", "plateau", "tiny", "gamma2")


def fine_weights(Nc, seed):
    """[len(FINE_PATTERNS), Nc] float32: one ray per weight pattern.  Weights are multiples of 2^-20 below 16 (2^-40 for the tiny-total
    ray), so every double sum of them is exact."""
    rs = np.random.RandomState(seed)
    grid = lambda x: (np.minimum(np.round(x * 2.0 ** 20), 2.0 ** 23) * 2.0 ** -20).astype(F32)
    rows = []
    for p in FINE_PATTERNS:
        if p.startswith("gamma"):
            x = grid(rs.gamma(0.5, 0.2, size=Nc))
        elif p.startswith("hot"):
            at = dict(hot0=0, hot63=63, hot64=64, hot_last=Nc - 1)[p]
            x = np.zeros(Nc, F32)
            x[min(at, Nc - 1)] = 0.75
        elif p == "zeros":
            x = np.zeros(Nc, F32)
        elif p == "plateau":                                   # zero from bin 60 to bin 70 (where the ray has them)
            x = np.maximum(grid(rs.gamma(0.5, 0.2, size=Nc)), F32(2.0 ** -20))
            x[60:71] = 0
        else:                                                  # total about 1e-7: the 1e-6 of the denominator dominates, most u fall past cdf[-1]
            share = rs.dirichlet(np.ones(Nc))
            x = (np.round(share * 1.1e5) * 2.0 ** -40).astype(F32)
        rows.append(x)
    return np.stack(rows)


def fine_inputs(Nc, Nf, grid, rng, seed=0):
    """one call's operands: grid in {"random", "det"}, rng in {"metric", "inverse"} -> (w, tc [R, Nc], u [Nf], dmin, dmax, grid [Nf + 1])"""
    rs = np.random.RandomState(1000 * Nc + Nf + seed)
    w = fine_weights(Nc, 7 * Nc + Nf + seed)
    R = w.shape[0]
    if grid == "det":
        g = torch.linspace(0, 1, Nf + 1)
    else:
        g = torch.from_numpy(rs.uniform(size=Nf + 1).astype(F32))                           # one shared UNSORTED draw (renderer.py:439)
    u = (0.5 * (g[:-1] + g[1:])).numpy()
    jit = rs.uniform(size=(R, Nc)).astype(F32)
    frac = ((jit + np.arange(Nc, dtype=F32)) / F32(Nc)).astype(F32)
    if rng == "metric":
        dmin, dmax = 1.2, 5.2
        tc = (frac * F32(4.0) + F32(1.2)).astype(F32)
    else:                                                      # the inverse-depth call: range [1, 0], t_coarse descending
        dmin, dmax = 1.0, 0.0
        tc = (F32(1.0) - frac).astype(F32)
    return w, tc, u, dmin, dmax, g


# ======================================================================================================================= part C
def composite_case(N, seed=0, R=7):
    """operands of one stand-alone compositing call, mixed within the call: ray 0 metric depths, density from transparent to opaque along
    the ray; 1 metric, thin (optical depth 0.7 in all, last density 0: opacity < 1, all_cumulated ~ 0.5), |ray| = 1.7; 2 inverse-depth
    depths up to 1e8, transparent to opaque; 3 inverse depth, thin; 4 zero density; 5 opaque at its first sample (T underflows behind
    it); 6 metric, uniform densities, |ray| = 0.6.  -> dict of float32 tensors t, dens [R, N], rgbs [R, N, 3], dirs [R, 3]"""
    assert R == 7
    rs = np.random.RandomState(100 + N + seed)
    i = np.arange(N, dtype=F32)
    jit = rs.uniform(size=(R, N)).astype(F32)
    jit[2, -1] = 1.0                                           # (u + i) / N = 1 at the last sample: t = 1 / (0 + 1e-8) = 1e8
    frac = ((jit + i) / F32(N)).astype(F32)
    t = (frac * F32(4.0) + F32(1.2)).astype(F32)
    inv = (F32(1.0) / ((F32(1.0) - frac).astype(F32) + F32(1e-8)).astype(F32)).astype(F32)
    t[2], t[3] = inv[2], inv[3]
    dirs = (rs.uniform(-0.3, 0.3, size=(R, 3)) + np.array([0.0, 0.0, 1.0])).astype(F32)
    dirs[1] *= F32(1.7 / np.linalg.norm(dirs[1]))
    dirs[6] *= F32(0.6 / np.linalg.norm(dirs[6]))
    ell = np.linalg.norm(dirs.astype(np.float64), axis=1)
    delta = np.concatenate([np.diff(t.astype(np.float64), axis=1), np.ones((R, 1))], axis=1) * ell[:, None]
    ramp = 10.0 ** np.linspace(-3.0, 2.0, N) * rs.uniform(0.5, 1.5, size=(R, N))
    dens = np.zeros((R, N))
    dens[0] = ramp[0]
    dens[1] = 0.7 / max(N - 1, 1) / delta[1] * rs.uniform(0.5, 1.5, size=N)
    dens[2] = ramp[2] / delta[2] * 4.0 / N                     # optical depth per sample as on a metric ray
    dens[3] = 0.7 / max(N - 1, 1) / delta[3] * rs.uniform(0.5, 1.5, size=N)
    dens[1, -1] = dens[3, -1] = 0.0
    dens[5] = rs.uniform(0.0, 3.0, size=N)
    dens[5, 0] = 1e4 / delta[5, 0]
    dens[6] = rs.uniform(0.0, 3.0, size=N)
    rgbs = rs.uniform(0.0, 1.0, size=(R, N, 3))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=F32))
    return dict(t=T(t), dens=T(dens), rgbs=T(rgbs), dirs=T(dirs))


def composite_grads(N, seed=0, R=7):
    """the seven upstream gradients of one call, uniform in (-1, 1)"""
    rs = np.random.RandomState(500 + N + seed)
    shp = dict(rgb=(R, 3), depth=(R,), opacity=(R,), weights=(R, N), depth_var=(R,), rgb_var=(R,), all_cumulated=(R,))
    return {k: torch.from_numpy(rs.uniform(-1, 1, size=s).astype(F32)) for k, s in shp.items()}


def raylen32(dirs):
    """|dir| as ray_len_kernel forms it: sqrtf(fl32(fl32(fl32(x x) + fl32(y y)) + fl32(z z)))"""
    d = dirs.float()
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sqrt()


def sd32(op):
    """(dist, sd) float32 as the kernels form them: delta = fl32(t_{i+1} - t_i) (1e10 behind the last sample), dist = fl32(delta ell),
    sd = fl32(dens dist)"""
    t = op["t"].float()
    delta = torch.cat([t[:, 1:] - t[:, :-1], torch.full_like(t[:, :1], 1e10)], dim=1)
    dist = delta * op["raylen"].float()[:, None]
    return delta, dist, op["dens"].float() * dist


MUTANTS = ("carry_dropped", "suffix_total_minus_prefix", "all_cum_at_nm1", "all_cum_at_nm3", "depth_var_term_dropped", "white_bg_sign",
           "all_cum_gate")
# the sample counts at which each mutant differs from the formula (COMPOSITE_N restricted).  total - prefix at N = 2: the fp32 sum of two
# terms has one order, total and prefix_1 are the same number and the residue behind the last sample is exactly 0
MUTANT_N = dict(carry_dropped=[65, 66, 67, 128, 129, 130, 192], suffix_total_minus_prefix=COMPOSITE_N[1:], all_cum_at_nm1=COMPOSITE_N,
                all_cum_at_nm3=COMPOSITE_N[1:], depth_var_term_dropped=COMPOSITE_N, white_bg_sign=COMPOSITE_N, all_cum_gate=COMPOSITE_N)


def composite_eval(op, g=None, dtype=torch.float64, mutant=None, exact_sd=False, ray_grad=True):
    """NeRF.composite and its closed-form gradients (ray_ops.hip composite_bwd_kernel's header comment) in `dtype`.
    op: t, dens [R, N], rgbs [R, N, 3], dirs [R, 3], raylen [R] float32, white_bg; optionally raw [R, N] float32 (the noised raw density
    of a pass: then d_density is chained through softplus and d_rgb_samples through the sigmoid, as the pass's d_sigma / d_z).
    g: dict of upstream gradients by output name (+ "density", "rgb_samples" in a pass), any subset.
    float64: the referee (sd restated in fp32 unless exact_sd: then everything is float64, for comparisons with autograd);
    float32: the yardstick; mutant: one of MUTANTS, a deliberately wrong formula."""
    g = g or {}
    R, N = op["t"].shape
    t, c = op["t"].to(dtype), op["rgbs"].to(dtype)
    if exact_sd:
        ell = op["dirs"].to(dtype).norm(dim=1)
        delta = torch.cat([t[:, 1:] - t[:, :-1], torch.full_like(t[:, :1], 1e10)], dim=1)
        dist = delta * ell[:, None]
        dens = op["dens"].to(dtype)
        sd = dens * dist
    else:
        d32, di32, s32 = sd32(op)
        delta, dist, sd, dens, ell = d32.to(dtype), di32.to(dtype), s32.to(dtype), op["dens"].to(dtype), op["raylen"].to(dtype)
    incl = sd.cumsum(1)
    excl = torch.cat([torch.zeros_like(sd[:, :1]), incl[:, :-1]], dim=1)
    if mutant == "carry_dropped" and N > 64:                  # T restarted at sample 64
        excl = torch.cat([excl[:, :64], excl[:, 64:] - excl[:, 64:65]], dim=1)
        incl = excl + sd
    T, Tn = torch.exp(-excl), torch.exp(-incl)
    alpha = -torch.expm1(-sd) if dtype == torch.float64 else 1.0 - torch.exp(-sd)
    w = T * alpha
    O, D, C = w.sum(1), (w * t).sum(1), (w[:, :, None] * c).sum(1)
    rgb = C + (1.0 - O)[:, None] if op["white_bg"] else C
    V = (w * (t - D[:, None]) ** 2).sum(1)
    Uv = (w * (c - C[:, None, :]).sum(-1)).sum(1)
    a_at = dict(all_cum_at_nm1=N - 1, all_cum_at_nm3=max(N - 3, 0)).get(mutant, N - 2)
    A = T[:, a_at]
    out = dict(rgb=rgb, depth=D, opacity=O, weights=w, depth_var=V, rgb_var=Uv, all_cumulated=A,
               _T=T, _Tn=Tn, _alpha=alpha, _sd=sd, _excl=excl, _incl=incl, _dist=dist, _delta=delta, _C=C)
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    gC = g["rgb"].to(dtype) if "rgb" in g else z(R, 3)
    gD, gO, gV, gU, gA = (g[k].to(dtype) if k in g else z(R) for k in ("depth", "opacity", "depth_var", "rgb_var", "all_cumulated"))
    gW = g["weights"].to(dtype) if "weights" in g else z(R, N)
    if op["white_bg"]:
        gO = gO + gC.sum(1) if mutant == "white_bg_sign" else gO - gC.sum(1)
    S, SC = c.sum(-1), C.sum(1)
    one_O = 1.0 - O
    q = (c * gC[:, None, :]).sum(-1) + gD[:, None] * t + gO[:, None] + gW
    dv = (t - D[:, None]) ** 2
    if mutant != "depth_var_term_dropped":
        dv = dv - 2.0 * t * (D * one_O)[:, None]
    q = q + gV[:, None] * dv + gU[:, None] * (S * one_O[:, None] - SC[:, None])
    wq = w * q
    if mutant == "suffix_total_minus_prefix":                 # the form of round 2: a total and a running prefix, both fp32, subtracted
        pre = torch.from_numpy(np.cumsum(wq.float().numpy(), axis=1, dtype=F32))                  # (numpy: a sequential fp32 sum)
        suffix = (wq.sum(1, keepdim=True).float() - pre).to(dtype)
    else:
        shifted = torch.cat([wq[:, 1:], torch.zeros_like(wq[:, :1])], dim=1)
        suffix = shifted.flip(1).cumsum(1).flip(1)
    gate = torch.arange(N)[None, :] < (N - 1 if mutant == "all_cum_gate" else N - 2)
    A_true = T[:, N - 2] if mutant in ("all_cum_at_nm1", "all_cum_at_nm3") else A        # (those two mutate the OUTPUT only)
    ds = Tn * q - suffix - (gA * A_true)[:, None] * gate.to(dtype)
    d_density = ds * dist
    if "density" in g:
        d_density = d_density + g["density"].to(dtype)
    d_rgbs = w[:, :, None] * (gC + (gU * one_O)[:, None])[:, None, :]
    if "rgb_samples" in g:
        d_rgbs = d_rgbs + g["rgb_samples"].to(dtype)
    d_len = (ds * dens * delta).sum(1)
    out.update(d_density=d_density, d_rgb_samples=d_rgbs, d_len=d_len, _q=q, _ds=ds, _suffix=suffix, _gC=gC, _gD=gD, _gO=gO, _gV=gV, _gU=gU,
               _gA=gA, _gW=gW)
    if ray_grad:
        out["d_dir"] = d_len[:, None] * op["dirs"].to(dtype) / ell.clamp_min(1e-12)[:, None]
    if "raw" in op:
        x = op["raw"].to(dtype)
        out["d_sigma"] = d_density * torch.where(x > 20.0, torch.ones_like(x), torch.sigmoid(x))
        out["d_z"] = d_rgbs * c * (1.0 - c)
    return out


def composite_bounds(op, ref):
    """element-wise bounds of every output and gradient from the referee's own intermediates (module docstring): dict name -> float64"""
    R, N = op["t"].shape
    t, c = op["t"].double(), op["rgbs"].double()
    T, Tn, alpha, sd, excl, incl, dist, delta = (ref[k] for k in ("_T", "_Tn", "_alpha", "_sd", "_excl", "_incl", "_dist", "_delta"))
    w, O, D, C = ref["weights"], ref["opacity"], ref["depth"], ref["_C"]
    gam = (N + 2) * U
    eT = T * (U * excl + EXPF) + TINY
    eTn = Tn * (U * incl + EXPF) + TINY
    eA = EXPF * torch.exp(-sd) + U * alpha
    bw = eT * alpha + T * eA + U * w + TINY
    dot = lambda x: (bw * x.abs()).sum(1) + gam * (w * x.abs()).sum(1)          # error of an fp32 dot product of the computed weights with x
    bO, bD = dot(torch.ones_like(t)), dot(t)
    bC = torch.stack([dot(c[:, :, k]) for k in range(3)], dim=1)
    b = dict(weights=bw, opacity=bO, depth=bD, all_cumulated=eT[:, N - 2])
    b["rgb"] = bC + (bO + U * (1.0 - O).abs() + U * ref["rgb"].abs().max(1).values)[:, None] if op["white_bg"] else bC
    dd = t - D[:, None]
    bdd = bD[:, None] + U * dd.abs()
    b["depth_var"] = (bw * dd ** 2 + 2.0 * w * dd.abs() * bdd + 2.0 * U * w * dd ** 2).sum(1) + gam * (w * dd ** 2).sum(1)
    s = (c - C[:, None, :]).sum(-1)
    sabs = (c - C[:, None, :]).abs().sum(-1)
    bs = bC.sum(1)[:, None] + 4.0 * U * sabs
    b["rgb_var"] = (bw * s.abs() + w * bs + U * w * s.abs()).sum(1) + gam * (w * sabs).sum(1)
    if "_q" in ref:
        gC, gD, gO, gV, gU, gA, gW = (ref[k] for k in ("_gC", "_gD", "_gO", "_gV", "_gU", "_gA", "_gW"))
        q, ds, suffix = ref["_q"], ref["_ds"], ref["_suffix"]
        S, SC = c.sum(-1), C.sum(1)
        bSC = dot(S)
        one_O = (1.0 - O).abs()
        gOmag = gO.abs() + (2.0 * gC.abs().sum(1) if op["white_bg"] else 0.0)
        Mq = ((c * gC.abs()[:, None, :]).sum(-1) + (gD[:, None] * t).abs() + gOmag[:, None] + gW.abs()
              + gV.abs()[:, None] * (dd ** 2 + 2.0 * (t * (D * one_O)[:, None]).abs()) + gU.abs()[:, None] * (S * one_O[:, None] + SC.abs()[:, None]))
        bq = (12.0 * U * Mq + gV.abs()[:, None] * (2.0 * dd.abs() * bD[:, None] + 2.0 * t.abs() * (bD * one_O + D.abs() * (bO + U))[:, None])
              + gU.abs()[:, None] * (S * (bO + U)[:, None] + bSC[:, None]))
        e = bw * q.abs() + w * bq
        shifted = torch.cat([e[:, 1:], torch.zeros_like(e[:, :1])], dim=1)
        bsuf = shifted.flip(1).cumsum(1).flip(1)
        gate = (torch.arange(N)[None, :] < N - 2).double()
        A = ref["all_cumulated"]
        bds = (eTn * q.abs() + Tn * bq + bsuf + U * ((Tn * q).abs() + 2.0 * suffix.abs())
               + (gA.abs() * (eT[:, max(N - 2, 0)] + 2.0 * U * A))[:, None] * gate)
        b["d_density"] = (bds + 2.0 * U * ds.abs()) * dist.abs() + U * ref["d_density"].abs()
        wu = (gU * (1.0 - O)).abs()
        b["d_rgb_samples"] = (bw[:, :, None] * (gC.abs() + wu[:, None])[:, None, :] + (w * (gU.abs() * (bO + U))[:, None])[:, :, None]
                              + 3.0 * U * ref["d_rgb_samples"].abs())
        dens = op["dens"].double()
        b_len = (bds * (dens * delta).abs()).sum(1) + (gam + 2.0 * U) * (ds * dens * delta).abs().sum(1)
        b["d_len"] = b_len
        if "d_dir" in ref:
            dirn = op["dirs"].double().abs() / op["raylen"].double().clamp_min(1e-12)[:, None]
            b["d_dir"] = b_len[:, None] * dirn + 3.0 * U * ref["d_dir"].abs()
        if "raw" in op:
            x = op["raw"].double()
            sig = torch.where(x > 20.0, torch.ones_like(x), torch.sigmoid(x))
            b["d_sigma"] = b["d_density"] * sig + (2.0 * EXPF + 2.0 * U) * ref["d_sigma"].abs()
            b["d_z"] = b["d_rgb_samples"] * (c * (1.0 - c)) + 4.0 * U * ref["d_z"].abs()
    return {k: SLACK * v for k, v in b.items()}


def rel_l2(a, b, floor=0.0):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), floor, 1e-300))


def check(name, got, ref, bound, yard, fails, figures, tag="", floor=None):
    """one output: element-wise bound, then relative L2 <= 4 x yardstick.  got: the kernel's (or a mutant's) values; floor: the absolute
    floor of the relative measure (rgb_var: 1)."""
    floor = (1.0 if name == "rgb_var" else 0.0) if floor is None else floor
    got, ref = got.double().cpu(), ref.double()
    over = ~((got - ref).abs() <= bound)                                        # (a NaN is past every bound)
    if bool(over.any()):
        i = over.nonzero()[0].tolist()
        where = f"ray {i[0]}" + (f" sample {i[1]}" if name in PER_SAMPLE else "") + f" index {i}"
        fails.append(f"{tag}{name}: {int(over.sum())} of {over.numel()} elements past the element-wise bound; first: {where}: got {float(got[tuple(i)])!r} "
                     f"want {float(ref[tuple(i)])!r} bound {float(bound[tuple(i)]):.3e}; rays affected {sorted(set(over.nonzero()[:, 0].tolist()))}")
    ek, ey = rel_l2(got, ref, floor), rel_l2(yard, ref, floor)
    figures[name] = (max(ek, figures.get(name, (0.0, 0.0))[0]), max(ey, figures.get(name, (0.0, 0.0))[1]))
    if not ek <= L2_FACTOR * ey:
        err = (got - ref).abs()
        i = [int(v) for v in np.unravel_index(int(err.argmax()), err.shape)]
        fails.append(f"{tag}{name}: relative L2 {ek:.3e} > {L2_FACTOR:g} x yardstick {ey:.3e}; largest error at ray {i[0]}"
                     + (f" sample {i[1]}" if name in PER_SAMPLE else "") + f" index {i}: got {float(got[tuple(i)])!r} want {float(ref[tuple(i)])!r}")


PER_SAMPLE = ("weights", "d_density", "d_rgb_samples", "d_sigma", "d_z", "density")


def report(figures):
    return "; ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in figures.items())
