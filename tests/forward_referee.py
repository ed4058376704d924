"""Float64 referee of the fused MLP forward, link by link, on the operands the kernel itself left in memory.

The training forward (csrc/mlp_fwd_impl.h) stores every layer INPUT in the save area (csrc/layout.h "AREAS"): the encoded point, the
seven hidden vectors, [feat | view encoding] and the colour branch's hidden vector, as fp32 (fp32 mode) or bf16 (bf16; bf16x3: the head
plane), plus one ReLU bit per stored activation.  What is stored is what the next layer multiplied, so the correct value of every link
is a fixed float64 expression of stored bytes and of the pass's inputs -- nothing compounds over the ten layers:

  link E  encodings   x0 = [p, sin/cos(p 2^k pi) w_k] with p = c + d t (mlp_fwd_impl.h), view = the same of d / max(|d|, 1e-12)
                      (ray_ops.hip ray_setup_kernel); one rounding to the area's element type
  link L  layers 0-8  X_{l+1} = fmt(relu(W_eff,l X_l + b_l)), X_l = `backward_referee.layer_inputs` of the decoded area
  link O  outputs     sigma_raw = row 0 of layer 7 (+ bias, no ReLU, fp32), rgb = sigmoid(W_9 G + b_9)
  link I  inference   the *_infer kernels' sigma_raw / rgb on the same inputs (tests/test_forward_links_gpu.py; bit-identical expected)

Decoders, feature-order maps, round_bf16 / ulp_bf16, effective_weights, layer_inputs and masks_feature are backward_referee's.
Every referee comes with its YARDSTICK: the same expression evaluated by torch in float32 on the same operands, on the same device.

Link E.  The argument a = fl32(p * fl32(pi) 2^k) is restated exactly in float32 (its rounding is part of the function: |a| reaches 1e7
under inverse depth); the referee is float64 sin / cos of that float32 a, times w_k.  The raw columns involve no transcendental: they
must be p (d) bit for bit in fp32 areas and round_bf16 of it in bf16 areas; padding slots must be 0; all rows of a ray carry the same
view columns.
  fp32 areas: |got - ref| <= max(4 x the yardstick's worst |yardstick - ref| of the case, 2^-24)   (2^-24: half a unit of fp32 at 1)
  bf16 areas: |got - ref| <= ulp_bf16(ref) (the conversion is one rounding of an fp32 value within a few fp32 units of ref); share of
              elements that are not round_bf16(ref) <= 8 x the yardstick's share + 16 / elements (a float32 sin lands on the other side
              of a bf16 rounding boundary about once in 2^16 elements; the count is a small-number statistic, hence the additive 16)

Link L, fp32 and bf16: the stored operand is the consumed operand.  With K = the layer's input width, every output is an fp32 sum of
K products (exact in fp32 for bf16 operands, one rounding each for fp32 operands) and the bias; any summation order commits at most
K + 1 roundings of partial sums that are each bounded by S = sum |W| |X| + |b|, the products at most K more: |acc - exact| <= 2 (K + 2)
2^-24 S (first order; the factor 2 covers the MFMA's internal order).  The area conversion adds half a unit of the area type at acc, at
most one unit at ref:
  element-wise |got - ref| <= ulp_area(ref) + 2 (K + 2) 2^-24 (|W_eff| |X| + |b|),  ulp_area = ulp_bf16 (bf16 areas) or 0 (fp32 areas)
  fp32 areas: relative L2 per layer <= 4 x yardstick
  bf16 areas: share of stored elements off round_bf16(ref) <= 8 x yardstick share + 16 / elements, and that bound itself <= 1e-3;
              layers under 1e5 elements are pooled per case (cases under 1e5 elements in all rely on the element-wise bound)
  the ReLU bits: set exactly where the stored output is > 0 (masks_feature(..., strict=True))

Link L, bf16x3.  The area holds the head plane hi = bf16(x) only; the kernel multiplied head + tail, lo = bf16(x - hi), in three MFMAs
per k-step, W_lo x_hi + W_hi x_lo + W_hi x_hi (mlp_dev.h Policy<PREC_X3>; W_lo x_lo does not exist).  The referee carries the tail
itself: its operand at layer l is the STORED head plus lo_l = round_bf16(fl32(xhat_l) - hi_l), xhat_l = the referee's own unrounded
output of the previous link (at the encodings: its float64 value), and its product is W_eff hi + W_hi lo.  Taking the head from the
kernel at every layer keeps the first eight bits from compounding; only the tail, below 2^-9 |x|, is the referee's.
  What the tail costs.  The kernel's tail is the same rounding of ITS fp32 accumulator.  x - hi keeps up to 16 significant bits of
which the tail keeps 8, so exact ties are common among fp32 values, and wherever accumulator and xhat lie on two sides of a tail
rounding boundary the tails differ by one unit of the tail's last place (2^-17 ... 2^-16 |x|).  That moves the next accumulator by
~sqrt(share of such elements) units, which in turn moves the share at the layer after: the disagreement saturates within three layers
at about one tail unit, 1e-5 relative (tests/test_forward_referee_cpu.py: an honest emulation sits at sigma_raw 1.2e-5, rgb 2.5e-6,
share of heads off the referee 1.3e-3 where the bf16 mode has 3e-5).  This is the resolution of a bf16x3 link cut at a head plane: no
referee can do better without the kernel's accumulators.  So that the caps stay reachable by a correct kernel, the bf16x3 YARDSTICK is
the honest float32 evaluation of the kernel's own scheme on the stored heads: it carries ITS tail from ITS fp32 accumulator of the
previous link, bf16(y - hi), and disagrees with the referee's tail in the same way.  The multiples stay (8 x share, 4 x relative L2).
The cap on the share bound itself, 1e-3, is what a bf16 link can hold; here it is replaced by the condition that the statistic
still resolves what it is there for: the bound must stay <= 1/4 of the share of heads that move when the referee leaves W_hi x_lo out
(19 ... 24 % of them, computed in every run; the honest share is 150 times smaller).
  Element-wise, the two tails differ by
      D_l <= |acc_l - xhat_l| + one unit of the tail's last place <= e_l + 2^-8 ulp_bf16(hi_l)
(|lo| <= ulp_bf16(hi) / 2, so a unit of the tail is at most 2^-8 ulp_bf16(hi)), and where the stored head is 0 the kernel's tail is 0
and D_l = |lo_l| exactly.  For e_l, the distance of a correct accumulator from xhat, the worst-case sum bound above is useless
(100 x the real thing, and it would compound through |W|); it is taken from the yardstick instead: e_l = 4 r_l S_l with r_l = the
yardstick's worst |acc_yardstick - acc_ref| / S over the layer, recomputed in every run -- the yardstick carries its own tail, so r_l
contains the saturated disagreement above -- and at the encodings 4 x the yardstick's worst distance, floor 2^-24.  This adds
      T_{l+1} = |W_hi| (D_l + e_l)
to the element-wise bound of the next link (and of link O).  A dropped W_hi x_lo is worth 2^-10 |W_hi| |X| on average (|lo| is spread
over [0, ulp / 2]); tests/test_forward_referee_cpu.py asserts sum T < 1/8 of sum 2^-9 |W_hi| |X| on the honest emulation at 312 rows
(measured 0.084 ... 0.089), a quarter of that, and that a forward with either tail product dropped in one layer, or in one 16-input
k-step of one layer, fails.  (r_l is a maximum over the layer's elements, so T grows slowly with the row count: 0.14 at 98 304 rows.)

Link O.  sigma_raw and the three pre-activations of rgb leave the accumulators unrounded: element-wise 2 (K + 2) 2^-24 S (+ T in
bf16x3); the sigmoid's slope is <= 1/4, and its evaluation 1 / (1 + expf(-z)) is held to the yardstick's worst distance of the same
float32 expression from float64: |rgb - ref| <= (2 (K + 2) 2^-24 S + T) / 4 + worst |sigmoid32(z) - sigmoid64(z)|.  Relative L2 of
sigma_raw and of rgb <= 4 x yardstick.

Small samples.  A relative L2 over n elements is a root mean square of n rounding errors, and so is the yardstick's; the ratio of two
such estimates exceeds 4 (16 in variance, F(n, n)) with probability 5.9e-2 at n = 2, 1.9e-3 at n = 6, 1.4e-6 at n = 15 for Gaussian
errors.  At the two sigma_raw values of case 1x2 an honest float32 emulation is past 4 x yardstick for one seed in four
(tests/test_forward_referee_cpu.py), so the relative-L2 statistics are asserted from L2_MIN = 15 elements on (case 3x5 has 15 sigma_raw
values); below that the element-wise bound stands alone, as it does for the share statistic under 1e5 elements.

A failure names the link, the layer, the feature column, and the row as (workgroup tile, wave, row of the wave's 32-row tile).
"""
import torch

from tests import backward_referee as BR
from tests.backward_referee import PI32, U24, round_bf16, ulp_bf16

TILE_ROWS = {"fp32": 128, "bf16": 256, "bf16x3": 128}                 # rows of a workgroup tile: 32 x waves (mlp_dev.h Policy<>::NWAVES)
L_POINT, L_VIEW = 10, 4
L2_MIN = 15                                                           # elements from which a relative-L2 statistic is asserted
POOL_MIN = 1e5                                                        # elements below which a layer's share statistic is pooled
# layer l's stored output: (index into layer_inputs, column range)
STORED_OUT = [(1, 256), (2, 256), (3, 256), (4, 256), (5, 256), (6, 256), (7, 256), (8, 256), (9, 128)]


def area_fmt(prec):
    return "fp32" if prec == "fp32" else "bf16"


# ----------------------------------------------------------------------------------------------------------------------- link E
def sample_points(center, dirs, t):
    """fp32, the kernel's steps: p = fadd(c, fmul(d, t)) per coordinate; center, dirs [R, 3], t [R, N] -> [R N, 3]"""
    R, N = t.shape
    return (center[:, None, :] + dirs[:, None, :] * t[:, :, None]).reshape(R * N, 3)


def view_dirs(dirs):
    """fp32, ray_setup_kernel's steps: len = sqrt((x x + y y) + z z), d = dir / fmaxf(len, 1e-12) -> (d [R, 3], len [R])"""
    x, y, z = dirs.unbind(1)
    ln = ((x * x + y * y) + z * z).sqrt()
    return dirs / ln.clamp_min(1e-12)[:, None], ln


def encoding_args(v, L):
    """a = fmul(v, ldexp(fl32(pi), k)): [n, 3] float32 -> [n, 3, L] float32"""
    fr = torch.tensor([PI32 * 2.0 ** k for k in range(L)], dtype=torch.float32, device=v.device)       # exact: fl32(pi) times 2^k
    return v[:, :, None] * fr


def encoding_reference(v, w):
    """v [n, 3] float32, band weights w [L] float32 -> (referee float64, yardstick float32), both [n, 3 + 6 L] in feature order
    [v(3), per coordinate: L sines, L cosines]"""
    a = encoding_args(v, w.numel())
    ad = a.double()
    ref = torch.stack([ad.sin(), ad.cos()], dim=2) * w.double()
    yard = torch.stack([a.sin(), a.cos()], dim=2) * w
    n = v.shape[0]
    return torch.cat([v.double(), ref.reshape(n, -1)], dim=1), torch.cat([v, yard.reshape(n, -1)], dim=1)


def where_row(r, tile_rows):
    return f"row {r} (workgroup tile {r // tile_rows}, wave {r % tile_rows // 32}, row {r % 32} of its 32-row tile {r // 32})"


def describe(name, got, ref, bound, tile_rows):
    """the first element past its bound: layer / column / tile / wave / row, values, and how many rows and columns are affected"""
    err = (got.double() - ref).abs()
    over = err > bound
    r, c = over.nonzero()[0].tolist()
    b = float(bound[r, c]) if torch.is_tensor(bound) and bound.dim() == 2 else float(bound)
    return (f"{name}: {int(over.sum())} of {over.numel()} elements past the element-wise bound; first: {where_row(r, tile_rows)} column {c}: "
            f"got {float(got[r, c])!r} want {float(ref[r, c])!r} bound {b:.3e}; rows affected {int(over.any(1).sum())}, columns affected "
            f"{int(over.any(0).sum())}")


def check_encoding(name, got, ref, yard, fmt, tile_rows, fails, figures):
    """link E of one encoded vector: got [n, 3 + 6 L] float32 (decoded area, feature order), ref float64, yard float32"""
    raw_want = ref[:, :3] if fmt == "fp32" else round_bf16(ref[:, :3])
    ne = (got[:, :3].view(torch.int32) != raw_want.float().view(torch.int32)) if fmt == "fp32" else (got[:, :3].double() != raw_want)
    if bool(ne.any()):
        r, c = ne.nonzero()[0].tolist()
        fails.append(f"E {name}: raw coordinate columns differ from the restated fp32 value at {int(ne.sum())} of {ne.numel()} places; first: "
                     f"{where_row(r, tile_rows)} column {c}: stored {float(got[r, c])!r} want {float(raw_want[r, c])!r}")
    g, rf, y = got[:, 3:], ref[:, 3:], yard[:, 3:]
    n = rf.numel()
    if fmt == "fp32":
        ey = float((y.double() - rf).abs().max())
        ek = float((g.double() - rf).abs().max())
        bound = max(4 * ey, U24)
        figures[f"E {name} worst distance"] = (ek, ey)
        if not ek <= bound:
            fails.append(f"E {name} (4 x yardstick {ey:.3e}, floor 2^-24) " + describe(name, g, rf, bound, tile_rows).replace("column", "sin/cos column"))
        return
    if bool(((g.double() - rf).abs() > ulp_bf16(rf)).any()):
        fails.append(f"E {name} (one ulp_bf16) " + describe(name, g, rf, ulp_bf16(rf), tile_rows).replace("column", "sin/cos column"))
    rr = round_bf16(rf)
    nk, ny = int((g.double() != rr).sum()), int((y.bfloat16().double() != rr).sum())
    figures[f"E {name} share off the referee"] = (nk / n, ny / n)
    if not nk / n <= 8 * ny / n + 16 / n:
        bad = (g.double() != rr).nonzero()[0].tolist()
        fails.append(f"E {name}: share of elements off the rounded referee {nk / n:.3e} > 8 x yardstick {ny / n:.3e} + 16 / {n}; first: "
                     f"{where_row(bad[0], tile_rows)} sin/cos column {bad[1]}")


# ------------------------------------------------------------------------------------------------------------------ links L and O
def head_weights(params, l):
    """bf16(W_l) as float64: the A operand of the two bf16x3 products that read it (pack.hip)"""
    return params[2 * l].detach().float().bfloat16().double()


def layer_reference(X, Weff, b, lo=None, Whi=None):
    """float64: (acc = W_eff X + b [+ W_hi lo], S = |W_eff| |X| + |b| [+ |W_hi| |lo|]); X [rows, in], W [out, in]"""
    X = X.double()
    b = b.detach().double()
    acc = X @ Weff.t() + b
    mag = X.abs() @ Weff.abs().t() + b.abs()
    if lo is not None:
        acc = acc + lo @ Whi.t()
        mag = mag + lo.abs() @ Whi.abs().t()
    return acc, mag


def layer_yardstick(X, W, b, prec, lo=None):
    """the same expression in float32 torch on the same operands -> fp32 accumulator (bf16x3: the three products of the kernel in ONE
    accumulation, [hi | lo | hi] @ [W_lo | W_hi | W_hi]^T)"""
    X, W, b = X.float(), W.detach().float(), b.detach().float()
    if prec == "fp32":
        return X @ W.t() + b
    head = W.bfloat16().float()
    if prec == "bf16":
        return X @ head.t() + b
    tail = (W - head).bfloat16().float()
    return torch.cat([X, lo.float(), X], dim=1) @ torch.cat([tail, head, head], dim=1).t() + b


def act(l, acc):
    """what layer l hands on: ReLU of everything but the raw density (row 0 of layer 7) and the colour pre-activations (layer 9)"""
    if l == 9:
        return acc
    if l == 7:
        return torch.cat([acc[:, :1], acc[:, 1:].clamp_min(0)], dim=1)
    return acc.clamp_min(0)


def tail_of(xhat, hi):
    """-> (the referee's tail lo = round_bf16(xhat - hi), D = bound of its distance to the kernel's tail without the e_l part):
    one unit of the tail's last place, <= 2^-8 ulp_bf16(hi); where the stored head is 0 the kernel's tail is 0: D = |lo|"""
    hi = hi.double()
    lo = round_bf16(xhat.float().double() - hi)          # (the kernel's x is an fp32 number: x - hi is exact, ties are ties of fp32 values)
    return lo, torch.where(hi == 0, lo.abs(), ulp_bf16(hi) * 2.0 ** -8)


def sigmoid32(z):
    """the kernel's expression in float32: 1 / (1 + exp(-z))"""
    return 1.0 / (1.0 + torch.exp(-z))


def check_forward(prec, save, center, dirs, t, c2f, params, sigma_raw, rgb, raylen=None, l2_min=L2_MIN):
    """All links of one training forward.  save: the plane save area (uint8); center, dirs [R, 3], t [R, N], c2f [16] float32: the
    pass's inputs; params: the 20 fp32 tensors; sigma_raw [R, N], rgb [R, N, 3]: the pass's per-sample outputs.
    -> (fails: list of str, figures: dict name -> (kernel, yardstick), state: link O's (referee, bound, yardstick) for link I)"""
    fmt, tile_rows, x3 = area_fmt(prec), TILE_ROWS[prec], prec == "bf16x3"
    R, N = t.shape
    rows = R * N
    fails, figures = [], {}
    X, M = BR.decode_planes(save, BR.SAVE_BUFS, 9, fp32=fmt == "fp32")
    Xs = BR.layer_inputs(X[:rows])
    try:
        BR.masks_feature(M, rows, X, strict=True)
    except AssertionError as e:
        fails.append(f"L ReLU bits: {e}")
    pad = BR.padding_columns(BR.SAVE_BUFS, "save").to(X.device)
    if not bool((X[:rows][:, pad] == 0).all()):
        bad = (X[:rows][:, pad] != 0).nonzero()[0].tolist()
        fails.append(f"E: a padding slot of x0 / the view encoding is not 0; first: {where_row(bad[0], tile_rows)}, padding slot {bad[1]} of 6")

    # ---- link E
    p = sample_points(center, dirs, t)
    d, ln = view_dirs(dirs)
    x0_ref, x0_yard = encoding_reference(p, c2f[:L_POINT])
    v_ref, v_yard = encoding_reference(d, c2f[L_POINT:L_POINT + L_VIEW])
    v_ref, v_yard = v_ref.repeat_interleave(N, dim=0), v_yard.repeat_interleave(N, dim=0)
    x0, view = Xs[0], Xs[8][:, 256:]
    check_encoding("point", x0, x0_ref, x0_yard, fmt, tile_rows, fails, figures)
    check_encoding("view", view, v_ref, v_yard, fmt, tile_rows, fails, figures)
    vr = view.view(R, N, -1)
    if not bool((vr.view(torch.int32) == vr[:, :1].view(torch.int32)).all()):
        r = int((vr.view(torch.int32) != vr[:, :1].view(torch.int32)).any(2).flatten().nonzero()[0])
        fails.append(f"E view: the rows of a ray do not carry bit-identical view columns; first: {where_row(r, tile_rows)}")
    if raylen is not None and not torch.equal(raylen.view(torch.int32), ln.view(torch.int32)):
        fails.append(f"E view: raylen differs from sqrt((x x + y y) + z z) at {int((raylen != ln).sum())} rays")

    # ---- links L and O
    Weff = BR.effective_weights(params, prec)
    # bf16x3: xhat of the current layer input and e of it (see the module docstring); enc_e: 4 x the yardstick's worst distance
    enc_e = lambda ref, yard: max(4 * float((yard.double() - ref).abs().max()), U24)
    xhat0, e0 = x0_ref, enc_e(x0_ref[:, 3:], x0_yard[:, 3:])
    xhat_v, e_v = v_ref, enc_e(v_ref[:, 3:], v_yard[:, 3:])
    raw_cols = lambda n, e, dev: torch.cat([torch.zeros(3, dtype=torch.float64, device=dev), torch.full((n - 3,), e, dtype=torch.float64, device=dev)])
    xhat, e_in = xhat0, raw_cols(63, e0, X.device).expand(rows, -1)
    yx = x0_yard                                                     # bf16x3: the yardstick's own fp32 layer input, source of ITS tail
    pool, lines, drops, t_ratio = [0, 0, 0, 0], [], [], (0.0, 0.0)
    state = {}
    for l in range(BR.N_LAYERS):
        hi = Xs[l]
        W, b = params[2 * l], params[2 * l + 1]
        K = hi.shape[1]
        lo = T = None
        if x3:
            lo, D = tail_of(xhat, hi)
            Whi = head_weights(params, l)
            T = (D + e_in) @ Whi.abs().t()
            t_ratio = (t_ratio[0] + float(T.sum()), t_ratio[1] + float((hi.double().abs() @ Whi.abs().t()).sum()) * 2.0 ** -9)
        acc, mag = layer_reference(hi, Weff[l], b, lo, Whi if x3 else None)
        ylo = (yx - hi).bfloat16().float() if x3 else None
        yacc = layer_yardstick(hi, W, b, prec, ylo)
        accb = 2.0 * (K + 2) * U24 * mag + (T if x3 else 0.0)
        ref = act(l, acc)
        if l == 7 or l == 9:                                        # link O: unrounded fp32 outputs
            if l == 7:
                got, want, y, bound, what = sigma_raw.reshape(rows, 1), ref[:, :1], yacc[:, :1], accb[:, :1], "sigma_raw (layer 7 row 0)"
            else:
                ys = sigmoid32(yacc)
                exp_y = float((ys.double() - torch.sigmoid(yacc.double())).abs().max())
                got, want, y, bound, what = rgb.reshape(rows, 3), torch.sigmoid(ref), ys, accb / 4 + exp_y, "rgb (layer 9)"
                figures["O sigmoid worst distance of the yardstick"] = (exp_y, exp_y)
            if bool(((got.double() - want).abs() > bound).any()):
                fails.append("O " + describe(what, got, want, bound, tile_rows))
            ek, ey = BR.rel_l2(got, want), BR.rel_l2(y, want)
            figures[f"O {what.split()[0]} rel. L2"] = (ek, ey)
            if got.numel() >= l2_min and not ek <= 4 * ey:
                fails.append(f"O {what}: kernel rel. L2 {ek:.3e} > 4 x yardstick {ey:.3e}")
            state["sigma_ref" if l == 7 else "rgb_ref"] = (want, bound, y)
        if l < 9:                                                   # link L: the stored output
            src, width = STORED_OUT[l]
            got = Xs[src][:, :width]
            want = ref[:, 1:] if l == 7 else ref
            wb = accb[:, 1:] if l == 7 else accb
            y = act(l, yacc)
            y = y[:, 1:] if l == 7 else y
            name = f"layer {l} -> {['H0', 'H1', 'H2', 'h3 of XS', 'H4', 'H5', 'H6', 'feat of FV', 'G'][l]}"
            bound = wb + (ulp_bf16(want) if fmt != "fp32" else 0.0)
            if bool(((got.double() - want).abs() > bound).any()):
                fails.append("L " + describe(name, got, want, bound, tile_rows))
            if fmt == "fp32":
                ek, ey = BR.rel_l2(got, want), BR.rel_l2(y, want)
                lines.append((ek, ey))
                if not ek <= 4 * ey:
                    fails.append(f"L {name}: kernel rel. L2 {ek:.3e} > 4 x yardstick {ey:.3e}")
            else:
                rr = round_bf16(want)
                nk, ny, n = int((got.double() != rr).sum()), int((y.bfloat16().double() != rr).sum()), rr.numel()
                lines.append((nk / n, ny / n))
                cap = 1e-3
                if x3:                                          # the share a dropped tail product moves, a quarter of it (module docstring)
                    nd = int((round_bf16(act(l, acc - lo @ Whi.t())[:, -width:]) != rr).sum())
                    drops.append(nd / n)
                    cap = nd / n / 4
                if n < POOL_MIN:
                    pool = [pool[0] + nk, pool[1] + ny, pool[2] + n, pool[3] + (nd if x3 else 0)]
                else:
                    limit = 8 * ny / n + 16 / n
                    if not limit <= cap:
                        fails.append(f"L {name}: the bound of the share, {limit:.2e}, exceeds {cap:.2e}")
                    if not nk / n <= limit:
                        bad = (got.double() != rr).nonzero()[0].tolist()
                        fails.append(f"L {name}: share of stored elements off the rounded referee {nk / n:.3e} > 8 x yardstick {ny / n:.3e} + 16 / {n}; "
                                     f"first: {where_row(bad[0], tile_rows)} column {bad[1]}")
        if x3:                                                      # hand the unrounded output and its e on
            r_l = float(((yacc.double() - acc).abs() / mag.clamp_min(1e-300)).max())
            e_out = 4.0 * r_l * mag
            out = ref[:, 1:] if l == 7 else ref
            e_out = e_out[:, 1:] if l == 7 else e_out
            yx = act(l, yacc)
            yx = yx[:, 1:] if l == 7 else yx
            if l == 3:
                xhat, e_in = torch.cat([out, xhat0], dim=1), torch.cat([e_out, raw_cols(63, e0, X.device).expand(rows, -1)], dim=1)
                yx = torch.cat([yx, x0_yard], dim=1)
            elif l == 7:
                xhat, e_in = torch.cat([out, xhat_v], dim=1), torch.cat([e_out, raw_cols(27, e_v, X.device).expand(rows, -1)], dim=1)
                yx = torch.cat([yx, v_yard], dim=1)
            else:
                xhat, e_in = out, e_out
    if pool[2] >= POOL_MIN:
        limit, cap = 8 * pool[1] / pool[2] + 16 / pool[2], (pool[3] / pool[2] / 4 if x3 else 1e-3)
        if not (limit <= cap and pool[0] / pool[2] <= limit):
            fails.append(f"L pooled layers: share {pool[0] / pool[2]:.3e}, yardstick {pool[1] / pool[2]:.3e}, bound {limit:.3e} (<= {cap:.2e} required)")
    worst = max(lines, key=lambda v: v[0] / max(v[1], 1e-300) if v[1] > 0 else v[0])
    figures["L " + ("rel. L2 per layer" if fmt == "fp32" else "share off the referee") + ", worst layer"] = worst
    if fmt != "fp32":
        n_all = sum(rows * w for _, w in STORED_OUT)
        figures["L share off the referee, all layers"] = (sum(v[0] * rows * w for v, (_, w) in zip(lines, STORED_OUT)) / n_all,
                                                          sum(v[1] * rows * w for v, (_, w) in zip(lines, STORED_OUT)) / n_all)
    if x3 and drops:
        figures["L share moved by a dropped tail product, least / most"] = (min(drops), max(drops))
    if x3:
        figures["L sum T / sum 2^-9 |W_hi| |X|"] = (t_ratio[0] / t_ratio[1], t_ratio[0] / t_ratio[1])
    return fails, figures, state


def chain_reference(center, dirs, t, c2f, params):
    """the links chained in float64 in fp32 format -- no tails, no area rounding, every layer input the referee's own previous output --
    -> (sigma_raw [R N], rgb [R N, 3]); tests/test_forward_referee_cpu.py holds this to the oracle"""
    N = t.shape[1]
    x0, _ = encoding_reference(sample_points(center, dirs, t), c2f[:L_POINT])
    v, _ = encoding_reference(view_dirs(dirs)[0], c2f[L_POINT:L_POINT + L_VIEW])
    v = v.repeat_interleave(N, dim=0)
    Weff = BR.effective_weights(params, "fp32")
    x, sigma = x0, None
    for l in range(BR.N_LAYERS):
        if l == 4:
            x = torch.cat([x, x0], dim=1)
        if l == 8:
            x = torch.cat([x, v], dim=1)
        out = act(l, layer_reference(x, Weff[l], params[2 * l + 1])[0])
        if l == 7:
            sigma, out = out[:, 0], out[:, 1:]
        x = out
    return sigma, torch.sigmoid(x)


def report(figures):
    return "; ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in figures.items())
