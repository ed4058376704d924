"""The backward referee (tests/backward_referee.py) is itself tested here, without a GPU.

(a) The three link referees chained in float64 -- masks from a float64 forward, no operand rounding -- equal torch.autograd of
    oracle.pass_fixed(..., compute_dtype=float64) to 1e-10 relative, parameters and pose, with and without c2f and density noise.
    That pins every index convention of the referee to the oracle, which is pinned to the reference.
(b) Mutation table on synthetic bf16 operands at 1 680 and 21 312 rows: honest float32 evaluations (torch's blocked product; the rows
    in reverse order) pass every bound the GPU tests assert; each mutation fails at least one of them.
(c) The layout maps and the mask-word decoder against an independent re-statement of csrc/layout.h."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nerf_oracle as O
from tests import backward_referee as BR
from tests.golden.recipe import small_opt, make_state_dict


def _scene(R, N, seed):
    rs = np.random.RandomState(seed)
    center = torch.from_numpy(rs.uniform(-0.5, 0.5, size=(R, 3))) + torch.tensor([0.0, 0.0, -3.0], dtype=torch.float64)
    ray = torch.from_numpy(rs.uniform(-0.3, 0.3, size=(R, 3))) + torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    jitter = torch.from_numpy(rs.uniform(0, 1, size=(1, R, N, 1)))
    noise = torch.from_numpy(rs.normal(size=(1, R, N)))
    return center, ray, jitter, noise


def _forward64(opt, sd, center, ray, t):
    """float64 forward that keeps every layer input (nn.Linear order) -> (X list, z, raw)"""
    P = {k: v.double() for k, v in sd.items()}
    pts = O.points_from_depth(center[None], ray[None], t[None, :, :, None])[0]                # [R, N, 3]
    R, N = t.shape
    x0 = torch.cat([pts, O.positional_encoding(opt, pts, 10, P["progress"], torch.float64)], dim=-1).reshape(R * N, 63)
    d = F.normalize(ray, dim=-1)[:, None, :].expand(R, N, 3)
    v = torch.cat([d, O.positional_encoding(opt, d, 4, P["progress"], torch.float64)], dim=-1).reshape(R * N, 27)
    X, h, raw = [], x0, None
    for l in range(8):
        if l == 4:
            h = torch.cat([h, x0], dim=1)
        X.append(h)
        y = F.linear(h, P[f"mlp_feat.{l}.weight"], P[f"mlp_feat.{l}.bias"])
        if l == 7:
            raw, y = y[:, 0], y[:, 1:]
        h = F.relu(y)
    X.append(torch.cat([h, v], dim=1))
    g = F.relu(F.linear(X[8], P["mlp_rgb.0.weight"], P["mlp_rgb.0.bias"]))
    X.append(g)
    return X, F.linear(g, P["mlp_rgb.1.weight"], P["mlp_rgb.1.bias"]), raw


@pytest.mark.parametrize("c2f,noise_reg", [(None, False), ([0.4, 0.7], True), ([0.4, 0.7], False), (None, True)])
def test_chained_link_referees_equal_float64_autograd_of_the_oracle(c2f, noise_reg):
    R, N = 7, 6
    opt = small_opt(barf_c2f=c2f, nerf=dict(density_noise_reg=1.0 if noise_reg else False, setbg_opaque=True))
    sd = make_state_dict(opt, 9, progress=0.62)
    center, ray, jitter, noise = _scene(R, N, 4)
    t = O.sample_depth(opt, 1, R, N, [1.2, 5.2], "train", jitter, dtype=torch.float64)[0, :, :, 0]
    rs = np.random.RandomState(8)
    lw = {k: torch.from_numpy(rs.uniform(-1, 1, size=s)) for k, s in (("rgb", (R, 3)), ("depth", (R, 1)), ("opacity", (R, 1)), ("weights", (R, N, 1)))}
    # the oracle and its autograd
    sdo = {k: v.double().requires_grad_(k != "progress") for k, v in sd.items()}
    co, ro = center.clone().requires_grad_(True), ray.clone().requires_grad_(True)
    ref = O.pass_fixed(opt, sdo, co[None], ro[None], t[None, :, :, None], mode="train", noise=noise, compute_dtype=torch.float64)
    sum((ref[k][0] * w).sum() for k, w in lw.items()).backward()
    # the chain's inputs: the forward's saved layer inputs, and d_z / d_sigma / d_len from the compositing alone
    X, z, raw = _forward64(opt, sd, center, ray, t)
    zl, rl, rc = z.detach().requires_grad_(True), raw.detach().requires_grad_(True), ray.clone().requires_grad_(True)
    dens = F.softplus(rl.view(1, R, N) + (noise * opt.nerf.density_noise_reg if noise_reg else 0.0))
    comp = O.composite(opt, rc[None], zl.sigmoid().view(1, R, N, 3), dens, t[None, :, :, None])
    assert torch.allclose(comp["rgb"], ref["rgb"].detach(), rtol=1e-12, atol=1e-14)            # (the restated forward is the oracle's)
    sum((comp[k][0] * w).sum() for k, w in lw.items()).backward()
    raylen = ray.norm(dim=-1)
    d_len = (rc.grad * ray).sum(-1) / raylen
    # link B chained, unrounded
    Weff = [sd[f"{n}.weight"].double() for n in BR.PARAM_NAMES]
    masks = {f"dY{l}": X[l + 1][:, :256] > 0 for l in range(7)}
    masks["dY7"], masks["dG"] = X[8][:, :256] > 0, X[9] > 0
    grads = {"dZ": zl.grad}
    for name, *_ in BR.CHAIN:
        rr, bound, _ = BR.link_b_reference(name, grads, masks, Weff, "fp32")
        grads[name] = torch.cat([rl.grad[:, None], rr], dim=1) if name == "dY7" else rr
    # link A
    dYs = [grads[f"dY{l}"] for l in range(8)] + [grads["dG"], grads["dZ"]]
    tol = 1e-10
    for l, n in enumerate(BR.PARAM_NAMES):
        dW, db, _, _ = BR.link_a_reference(dYs[l], X[l])
        assert BR.rel_l2(dW, sdo[n + ".weight"].grad) < tol and BR.rel_l2(db, sdo[n + ".bias"].grad) < tol, n
    # link C
    w_pos, w_view = O.c2f_mask(opt, 10, sd["progress"]), O.c2f_mask(opt, 4, sd["progress"])
    band = torch.ones(16, dtype=torch.float64)
    if w_pos is not None:
        band[:10], band[10:14] = w_pos.double(), w_view.double()
    dv, dp = BR.pose_reference(grads, Weff, center, ray, t, band)
    d_center, d_dir = BR.ray_reference(dp, dv, d_len, ray, raylen, t, band)
    assert BR.rel_l2(d_center, co.grad) < tol and BR.rel_l2(d_dir, ro.grad) < tol


def test_layout_maps_and_mask_bits_restate_layout_h():
    """the decoders invert an encoder written straight from the layout.h formulas; every feature appears once"""
    pos_of = lambda q, h, ch: (q // ch) * (2 * ch) + h * ch + q % ch
    # a bf16 save area of one tile whose element at (buffer, pos) holds a code of (q, h): decode -> canonical
    rows = 32
    area = torch.zeros(sum(BR.SAVE_BUFS) * 32 * 2 + 9 * 1024, dtype=torch.uint8)
    vals = area[:sum(BR.SAVE_BUFS) * 64].view(torch.bfloat16)
    off = 0
    for b, C in enumerate(BR.SAVE_BUFS):
        blk = vals[off * 32:(off + C) * 32].view(C // 8, 32, 8)                                   # [chunk][row][el]
        for h in (0, 1):
            for q in range(C // 2):
                pos = pos_of(q, h, 8)
                blk[pos // 8, :, pos % 8] = float((q + 1) * (1 - 2 * h))                          # code(h, q): |.| <= 160, exact in bf16
        off += C
    # mask words: lane (n, h) pushes slot q as bit 31 - q % 32 of word q // 32; set the bit iff (q + n + h) % 3 == 0
    words = torch.zeros(9, 64, 4, dtype=torch.int64)
    for h in (0, 1):
        for q in range(128):
            for n in range(32):
                if (q + n + h) % 3 == 0:
                    words[:, n + 32 * h, q // 32] |= 1 << (31 - q % 32)
    area[sum(BR.SAVE_BUFS) * 64:] = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).view(-1).view(torch.uint8)
    X, M = BR.decode_planes(area, BR.SAVE_BUFS, 9)
    off = 0
    for C in BR.SAVE_BUFS:
        want = torch.cat([torch.arange(C // 2) + 1.0, -(torch.arange(C // 2) + 1.0)])
        assert torch.equal(X[0, off:off + C], want.float())
        off += C
    bits = BR.decode_masks(M, rows)
    n = torch.arange(32)[:, None]
    for h in (0, 1):
        q = torch.arange(128)[None, :]
        assert torch.equal(bits[:, 1, h * 128:(h + 1) * 128], (q + n + h) % 3 == 0)
        assert torch.equal(bits[:, BR.SB_G, h * 128:(h + 1) * 128], ((q + n + h) % 3 == 0) & (q < 64))
    # feature maps: hidden vectors carry C-row crow_of(q, h) = 32 (q >> 4) + (q & 3) + 8 ((q & 15) >> 2) + 4 h
    crow = lambda q, h: 32 * (q >> 4) + (q & 3) + 8 * ((q & 15) >> 2) + 4 * h
    code = lambda h, q: float((q + 1) * (1 - 2 * h))
    Xs = BR.layer_inputs(X)
    for f in (0, 1, 5, 37, 255):
        (h, q), = [(h, q) for h in (0, 1) for q in range(128) if crow(q, h) == f]
        assert float(Xs[1][0, f]) == code(h, q) and float(Xs[4][0, f]) == code(h, q) and float(Xs[8][0, f]) == code(h, q)
    # x0: [p(3), per coordinate 10 sin, 10 cos]; lane half h evaluates arguments a = 15 h + (q >> 1), slots 30 / 31 hold the raw point
    assert [float(v) for v in Xs[0][0, :3]] == [code(0, 128 + 30), code(0, 128 + 31), code(1, 128 + 30)]
    for c in range(3):
        for k in range(10):
            a = c * 10 + k
            h, q = a // 15, 2 * (a % 15)
            assert float(Xs[0][0, 3 + c * 20 + k]) == code(h, 128 + q) and float(Xs[0][0, 3 + c * 20 + 10 + k]) == code(h, 128 + q + 1)
            assert float(Xs[4][0, 256 + 3 + c * 20 + k]) == code(h, 128 + q)
    for c in range(3):
        for k in range(4):
            a = c * 4 + k
            h, q = a // 6, 2 * (a % 6)
            assert float(Xs[8][0, 256 + 3 + c * 8 + k]) == code(h, 128 + q) and float(Xs[8][0, 256 + 3 + c * 8 + 4 + k]) == code(h, 128 + q + 1)
    assert sorted(BR._DV_POS) == sorted(set(BR._DV_POS)) and min(BR._DV_POS) >= 0
    assert int(BR.padding_columns(BR.SAVE_BUFS, "save").sum()) == 1 + 5 and int(BR.padding_columns(BR.GRAD_BUFS, "grad").sum()) == 31 + 29


def test_round_bf16_is_one_rounding_to_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415926, 0.0, 1e-20], dtype=torch.float64)
    got = BR.round_bf16(x)
    assert [float(v) for v in got[:4]] == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]
    assert torch.equal(got, x.float().bfloat16().double())
    # a double-rounding case: float32 first lands on the tie, which then rounds to even = down; one rounding goes up
    y = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert float(BR.round_bf16(y)) == 1.0 + 2.0 ** -7


# ------------------------------------------------------------------------------------------------------------------ mutation table
def _synthetic(rows, seed):
    g = torch.Generator().manual_seed(seed)
    bf = lambda x: x.bfloat16().float()
    dY = bf(torch.randn(rows, 256, generator=g) * 0.02)
    X = bf(torch.relu(torch.randn(rows, 256, generator=g)))
    W = torch.randn(256, 256, generator=g) / 16                            # [out, in] of the layer whose transpose the link applies
    mask = torch.rand(rows, 256, generator=g) < 0.5
    return dY, X, W, mask


def _link_a_verdict(got_W, got_b, dY, X, nsplit, rps):
    """the checks of link A as the GPU test applies them -> list of the checks that fail"""
    refW, refb, magW, magb = BR.link_a_reference(dY, X)
    yW, yb = BR.link_a_yardstick(dY, X, nsplit, rps)
    bW, bb = BR.link_a_bound(dY.shape[0], magW, magb)
    fails = []
    if bool(((got_W.double() - refW).abs() > bW).any()) or bool(((got_b.double() - refb).abs() > bb).any()):
        fails.append("element-wise")
    for name, got, ref, y in (("W", got_W, refW, yW), ("b", got_b, refb, yb)):
        ys = BR.rel_l2(y, ref)
        assert 4 * ys < 1e-4, (name, ys)                                 # the condition of the statistic
        if BR.rel_l2(got, ref) > 4 * ys:
            fails.append("rel-l2 " + name)
    return fails


@pytest.mark.parametrize("rows", [1680, 21312])
def test_link_a_checks_pass_honest_float32_and_catch_every_mutation(rows):
    dY, X, _, _ = _synthetic(rows, 1)
    nsplit, rps = (3, 576) if rows == 1680 else (6, 3584)                 # what the library plans for these row counts (wgrad_splits)
    assert (nsplit - 1) * rps < rows <= nsplit * rps
    f32 = lambda a, b: (a.t() @ b, a.sum(0))
    # honest evaluations: torch's blocked product; the rows in reverse order; the yardstick's shape with another split size
    assert _link_a_verdict(*f32(dY, X), dY, X, nsplit, rps) == []
    assert _link_a_verdict(*f32(dY.flip(0), X.flip(0)), dY, X, nsplit, rps) == []
    assert _link_a_verdict(*BR.link_a_yardstick(dY, X, (rows + 1023) // 1024, 1024), dY, X, nsplit, rps) == []
    r = rows // 3
    keep = torch.ones(rows, dtype=torch.bool)
    keep[r] = False
    mutants = {
        "one row dropped": f32(dY[keep], X[keep]),
        "one row used twice": f32(torch.cat([dY, dY[r:r + 1]]), torch.cat([X, X[r:r + 1]])),
        "one split's partial block left out of the reduce": BR.link_a_yardstick(dY, X, nsplit, rps, drop_split=nsplit - 1),
    }
    pad = (-rows) % 32 or 32
    W, _ = f32(dY, X)
    mutants["bias sum over padded rows"] = (W, torch.cat([dY, torch.full((pad, 256), 0.02)]).sum(0))
    for name, (gW, gb) in mutants.items():
        assert _link_a_verdict(gW, gb, dY, X, nsplit, rps) != [], f"mutation not caught: {name}"


def _link_b_verdict(got, dY, W, mask):
    """the checks of link B as the GPU test applies them (bf16 areas, bf16x3 weights) -> list of the checks that fail"""
    params = [None, None, W] + [None] * 17                                 # layer 1 of the chain: dY0 = mask * (W1^T dY1)
    head = W.bfloat16().float()
    weff = head.double() + (W - head).bfloat16().double()
    grads, masks = {"dY1": dY}, {"dY0": mask}
    ref, bound, _ = BR.link_b_reference("dY0", grads, masks, [None, weff], "bf16")
    y = BR.link_b_yardstick("dY0", grads, masks, params, "bf16x3")
    fails = []
    if bool(((got.double() - ref).abs() > bound).any()):
        fails.append("element-wise")
    limit = 8 * float((y.double() != ref).double().mean()) + 16 / ref.numel()
    assert limit <= 1e-3, limit                                            # the condition of the statistic
    if float((got.double() != ref).double().mean()) > limit:
        fails.append("share")
    return fails


@pytest.mark.parametrize("rows", [1680, 21312])
def test_link_b_checks_pass_honest_float32_and_catch_every_mutation(rows):
    dY, _, W, mask = _synthetic(rows, 2)
    head = W.bfloat16().float()
    tail = (W - head).bfloat16().float()
    m = mask.float()
    bf = lambda x: x.bfloat16().float()
    # honest: two separate float32 products summed; one product of the float32 sum head + tail
    assert _link_b_verdict(bf((dY @ head + dY @ tail) * m), dY, W, mask) == []
    assert _link_b_verdict(bf((dY @ (head + tail)) * m), dY, W, mask) == []
    neighbour = mask.clone()
    neighbour[32:64] = mask[64:96]
    exact = (dY.double() @ (head.double() + tail.double())) * m.double()
    mutants = {
        "one 32-row tile's mask taken from its neighbour": bf((dY @ head + dY @ tail) * neighbour.float()),
        "tail product dropped": bf((dY @ head) * m),
        "weights not split": bf((dY @ W) * m),
        "truncation instead of nearest in the dY rounding": BR.trunc_bf16(exact).float(),
    }
    for name, got in mutants.items():
        assert _link_b_verdict(got, dY, W, mask) != [], f"mutation not caught: {name}"
