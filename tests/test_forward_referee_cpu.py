"""The forward referee (tests/forward_referee.py) is itself tested here, without a GPU.

(a) The links chained in float64 in fp32 format -- no tails, no area rounding -- equal oracle.nerf_oracle.mlp evaluated in float64 on
    the same rays to 1e-10, with c2f on and off.  That pins the referee's index conventions and its restated encodings to the oracle.
(b) Honest emulation: each mode's arithmetic emulated in torch float32 at 312 rows -- fp32 products, or bf16 operands, or the
    three-product head / tail scheme with its fp32 accumulator and the bf16(x - float(head)) tail, accumulated k-step by k-step as the
    kernel does (so it is NOT the yardstick's single product), rounded once to the area type, encoded into a save area byte for byte
    (encode_planes and its fp32 sibling below, mask words included) -- passes every check of links E, L and O.  That is the condition
    under which the caps (1e-3 share, 4 x and 8 x yardstick) are reachable by a correct kernel.
(c) Every mutation of that emulation fails at least one check.
(d) bf16x3: the tail term T of the element-wise bound stays below 1/8 of 2^-9 |W_hi| |X|."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import backward_referee as BR
from tests import forward_referee as FR
from tests.golden.recipe import small_opt, make_state_dict

PRECS = ["fp32", "bf16", "bf16x3"]


def _scene(R, N, seed, exact_len=False):
    rs = np.random.RandomState(seed)
    center = torch.from_numpy(rs.uniform(-0.5, 0.5, size=(R, 3)).astype(np.float32)) + torch.tensor([0.0, 0.0, -3.0])
    if exact_len:      # components k / 64: the sum of squares is exact in fp32 in any order, so every normalisation agrees bit for bit
        dirs = torch.from_numpy(rs.randint(-19, 20, size=(R, 3)).astype(np.float32)) / 64 + torch.tensor([0.0, 0.0, 1.0])
    else:
        dirs = torch.from_numpy(rs.uniform(-0.3, 0.3, size=(R, 3)).astype(np.float32)) + torch.tensor([0.0, 0.0, 1.0])
    jitter = torch.from_numpy(rs.uniform(0, 1, size=(1, R, N, 1)).astype(np.float32))
    return center, dirs, jitter


def _bands(opt, sd):
    """the pass's 16-float band vector (10 point bands, 4 view bands, 2 pad) from the oracle's c2f mask"""
    band = torch.zeros(16)
    band[:14] = 1.0
    if opt.barf_c2f is not None:
        band[:10], band[10:14] = O.c2f_mask(opt, 10, sd["progress"]), O.c2f_mask(opt, 4, sd["progress"])
    return band


def _plist(sd):
    return [sd[f"{n}.{k}"] for n in BR.PARAM_NAMES for k in ("weight", "bias")]


@pytest.mark.parametrize("c2f", [None, [0.4, 0.7]], ids=["plain", "c2f"])
def test_chained_links_equal_the_float64_oracle(c2f):
    R, N = 9, 7
    opt = small_opt(barf_c2f=c2f)
    sd = make_state_dict(opt, 9, progress=0.62)
    center, dirs, jitter = _scene(R, N, 4, exact_len=True)
    t = O.sample_depth(opt, 1, R, N, [1.2, 5.2], "train", jitter)[0, :, :, 0]
    sd64 = {k: v.double() for k, v in sd.items()}
    rgb, dens = O.mlp(opt, sd64, O.points_from_depth(center[None], dirs[None], t[None, :, :, None]), dirs[None], "val", None,
                      compute_dtype=torch.float64)
    sigma, got_rgb = FR.chain_reference(center, dirs, t, _bands(opt, sd), _plist(sd))
    assert BR.rel_l2(torch.nn.functional.softplus(sigma), dens.reshape(-1)) < 1e-10
    assert BR.rel_l2(got_rgb, rgb.reshape(-1, 3)) < 1e-10


# --------------------------------------------------------------------------------------------------- save-area encoders (test side)
def _encode_planes_fp32(X, bufs, tail):
    """fp32 sibling of backward_referee.encode_planes: 4-element chunks, pos = (q // 4) * 8 + h * 4 + q % 4 (layout.h pos_of)"""
    ntiles = X.shape[0] // 32
    parts, off = [], 0
    for C in bufs:
        pos = torch.arange(C)
        q = (pos // 8) * 4 + pos % 4
        h = (pos // 4) % 2
        order = torch.argsort(h * (C // 2) + q)
        x = torch.empty(X.shape[0], C)
        x[:, order] = X[:, off:off + C]
        vals = x.view(ntiles, 32, C // 4, 4).permute(0, 2, 1, 3).contiguous()
        parts.append(vals.view(torch.uint8).reshape(ntiles, C * 128))
        off += C
    return torch.cat(parts + [tail], dim=1).reshape(-1)


def _encode_masks(bits):
    """inverse of backward_referee.decode_masks: bool [rows_padded, 9, 256] (canonical h * 128 + q) -> mask bytes [tiles, 9 KiB]"""
    ntiles = bits.shape[0] // 32
    b = bits.view(ntiles, 32, 9, 2, 4, 32).long()                                   # [tile][n][buffer][h][word][bit 31 - j]
    w = (b << (31 - torch.arange(32))).sum(-1)                                      # [tile][n][buffer][h][word]
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    return w.permute(0, 2, 3, 1, 4).reshape(ntiles, 9 * 64 * 4).contiguous().view(torch.uint8)      # lane = n + 32 h


def _assemble(vectors, relu_out, rows, fp32):
    """feature-order stored vectors -> save area bytes.  vectors: dict buffer -> [rows, features] (XS: [h3 | x0], FV: [feat | view]);
    relu_out: dict buffer -> [rows, 256 | 128] the ReLU outputs whose bits live next to that buffer"""
    rp = (rows + 31) // 32 * 32
    X = torch.zeros(rp, sum(BR.SAVE_BUFS))
    bits = torch.zeros(rp, 9, 256, dtype=torch.bool)
    maps = {BR.SB_XS: BR._XS, BR.SB_FV: BR._FV, BR.SB_G: BR._HID128}
    for b, v in vectors.items():
        o = sum(BR.SAVE_BUFS[:b])
        X[:rows, torch.tensor(maps.get(b, BR._HID256)) + o] = v
    for b, v in relu_out.items():
        if b == BR.SB_G:
            c = torch.tensor(BR._HID128)
            bits[:rows, b, (c // 64) * 128 + c % 64] = v
        else:
            bits[:rows, b, torch.tensor(BR._HID256)] = v
    tail = _encode_masks(bits)
    return _encode_planes_fp32(X, BR.SAVE_BUFS, tail) if fp32 else BR.encode_planes(X, BR.SAVE_BUFS, tail)


# ------------------------------------------------------------------------------------------------------------------- the emulation
def _emulate(prec, center, dirs, t, band, params, mut=None):
    """-> (save area bytes, sigma_raw [R, N], rgb [R, N, 3]) of mode `prec` in float32; `mut`: one mutation of the table below"""
    R, N = t.shape
    rows = R * N
    x3, fp32 = prec == "bf16x3", prec == "fp32"
    rnd = (lambda x: BR.trunc_bf16(x.double()).float()) if mut == "truncation" else (lambda x: x.bfloat16().float())
    tt = t.clone()
    if mut == "second tile with the first tile's depths":
        tr = FR.TILE_ROWS[prec]
        flat = tt.view(-1)
        flat[tr:min(2 * tr, rows)] = flat[:min(2 * tr, rows) - tr].clone()
    w_pos, w_view = band[:10].clone(), band[10:14]
    if mut == "band weight on the neighbouring band":
        w_pos = torch.roll(w_pos, 1)
    _, x0 = FR.encoding_reference(FR.sample_points(center, dirs, tt), w_pos)          # the float32 evaluation
    _, v = FR.encoding_reference(FR.view_dirs(dirs)[0], w_view)
    if mut == "view columns of a ray from its neighbour":
        v[3] = v[4]
    v = v.repeat_interleave(N, dim=0)
    if mut == "two x0 columns exchanged":
        x0[:, [5, 17]] = x0[:, [17, 5]]

    def operand(x):                                     # fp32 value -> (what is stored = head, tail or None)
        if fp32:
            return x, None
        hi = rnd(x)
        return hi, ((x - hi).bfloat16().float() if x3 else None)

    def layer(l, hi, lo):
        W, b = params[2 * l].float(), params[2 * l + 1].float()
        Wh = W if fp32 else W.bfloat16().float()
        Wl = (W - Wh).bfloat16().float() if x3 else None
        acc = b.expand(rows, -1).clone()
        if mut == "bias missing on one 32-output block" and l == 2:
            acc[:, 32:64] = 0.0
        for k0 in range(0, hi.shape[1], 16):            # one 16-input k-step after the other into the fp32 accumulator
            if mut == "one 16-input k-chunk omitted" and l == 5 and k0 == 48:
                continue
            s = slice(k0, k0 + 16)
            if x3:
                if not (mut == "W_lo x_hi dropped" and l == 2):
                    acc += hi[:, s] @ Wl[:, s].t()
                if not (mut == "W_hi x_lo dropped" and l == 6) and not (mut == "W_hi x_lo dropped in one 16-input k-chunk" and l == 6 and k0 == 48):
                    acc += lo[:, s] @ Wh[:, s].t()
            acc += hi[:, s] @ Wh[:, s].t()
        return acc

    stored, relu_out = {}, {}
    x0h, x0l = operand(x0)
    vh, vl = operand(v)
    cat = lambda a, b: None if a is None else torch.cat([a, b], dim=1)
    hi, lo = x0h, x0l
    bufs = [BR.SB_H0, BR.SB_H1, BR.SB_H2, BR.SB_XS, BR.SB_H4, BR.SB_H5, BR.SB_H6, BR.SB_FV, BR.SB_G]
    sigma = None
    for l in range(9):
        if l == 4:
            hi, lo = torch.cat([hi, x0h], dim=1), cat(lo, x0l)
        if l == 8:
            hi, lo = torch.cat([hi, vh], dim=1), cat(lo, vl)
        acc = layer(l, hi, lo)
        if l == 7:
            sigma, acc = acc[:, 0], acc[:, 1:]
            if mut == "sigma_raw after the ReLU":
                sigma = sigma.clamp_min(0)
        hi, lo = operand(acc.clamp_min(0))
        relu_out[bufs[l]] = hi > 0
        stored[bufs[l]] = hi
    stored[BR.SB_XS] = torch.cat([stored[BR.SB_XS], x0h], dim=1)
    stored[BR.SB_FV] = torch.cat([stored[BR.SB_FV], vh], dim=1)
    if mut == "mask bit cleared under a positive value":
        r, c = (stored[BR.SB_H4] > 0).nonzero()[7].tolist()
        relu_out[BR.SB_H4][r, c] = False
    z = layer(9, hi, lo)
    if mut == "rgb channel with the wrong row of layer 9":
        z[:, 1] = z[:, 2]
    rgb = FR.sigmoid32(z)
    return _assemble(stored, relu_out, rows, fp32), sigma.view(R, N), rgb.view(R, N, 3)


MUTATIONS = ["W_hi x_lo dropped", "W_lo x_hi dropped", "W_hi x_lo dropped in one 16-input k-chunk", "one 16-input k-chunk omitted", "bias missing on one 32-output block",
             "two x0 columns exchanged", "band weight on the neighbouring band", "truncation", "second tile with the first tile's depths",
             "view columns of a ray from its neighbour", "sigma_raw after the ReLU", "rgb channel with the wrong row of layer 9",
             "mask bit cleared under a positive value"]


def _applies(mut, prec):
    return prec == "bf16x3" if "dropped" in mut else prec != "fp32" if mut == "truncation" else True


_CASES = {}


def _case(c2f):
    """one scene (13 x 24 = 312 rows: a second workgroup tile in every mode), shared and left unchanged"""
    if c2f not in _CASES:
        R, N = 13, 24
        opt = small_opt(barf_c2f=[0.4, 0.7] if c2f else None)
        sd = make_state_dict(opt, 21, progress=0.55)
        center, dirs, jitter = _scene(R, N, 5)
        t = O.sample_depth(opt, 1, R, N, [1.2, 5.2], "train", jitter)[0, :, :, 0].contiguous()
        _CASES[c2f] = (center, dirs, t, _bands(opt, sd), _plist(sd))
    return _CASES[c2f]


@pytest.mark.parametrize("c2f", [True, False], ids=["c2f", "plain"])
@pytest.mark.parametrize("prec", PRECS)
def test_honest_emulation_passes_every_check(prec, c2f):
    center, dirs, t, band, params = _case(c2f)
    save, sigma, rgb = _emulate(prec, center, dirs, t, band, params)
    fails, figures, _ = FR.check_forward(prec, save, center, dirs, t, band, params, sigma, rgb)
    print(FR.report(figures))
    assert not fails, "\n".join(fails)
    if prec == "bf16x3":
        assert figures["L sum T / sum 2^-9 |W_hi| |X|"][0] < 1 / 8


@pytest.mark.parametrize("mut,prec", [(m, p) for m in MUTATIONS for p in PRECS if _applies(m, p)])
def test_every_mutation_fails_a_check(mut, prec):
    center, dirs, t, band, params = _case(True)
    save, sigma, rgb = _emulate(prec, center, dirs, t, band, params, mut)
    fails, _, _ = FR.check_forward(prec, save, center, dirs, t, band, params, sigma, rgb)
    print("\n".join(fails[:4]))
    assert fails, f"mutation not caught in {prec}: {mut}"


def test_relative_l2_caps_need_fifteen_elements():
    """the small-sample rule of the referee (module docstring): at 1 x 2 rows an honest emulation is past 4 x yardstick on the two
    sigma_raw values for some seeds when the statistic is asserted on them; from 15 elements on (3 x 5 rows) it never is"""
    opt = small_opt(barf_c2f=[0.4, 0.7])
    sd = make_state_dict(opt, 21, progress=0.55)
    band, params = _bands(opt, sd), _plist(sd)
    past = {(1, 2): 0, (3, 5): 0}
    for (R, N) in past:
        for seed in range(12):
            center, dirs, jitter = _scene(R, N, seed)
            t = O.sample_depth(opt, 1, R, N, [1.2, 5.2], "train", jitter)[0, :, :, 0].contiguous()
            save, sigma, rgb = _emulate("fp32", center, dirs, t, band, params)
            fails, _, _ = FR.check_forward("fp32", save, center, dirs, t, band, params, sigma, rgb, l2_min=0)
            assert all("rel. L2" in f and f.startswith("O ") for f in fails), fails          # (nothing else ever fails)
            past[(R, N)] += bool(fails)
            assert not FR.check_forward("fp32", save, center, dirs, t, band, params, sigma, rgb)[0]
    assert past[(1, 2)] >= 2 and past[(3, 5)] == 0, past


def test_test_side_encoders_invert_the_decoders():
    g = torch.Generator().manual_seed(3)
    X = torch.randn(64, sum(BR.SAVE_BUFS), generator=g)
    bits = torch.rand(64, 9, 256, generator=g) < 0.5
    bits[:, BR.SB_G] &= (torch.arange(256) % 128 < 64)
    tail = _encode_masks(bits)
    got, M = BR.decode_planes(_encode_planes_fp32(X, BR.SAVE_BUFS, tail), BR.SAVE_BUFS, 9, fp32=True)
    assert torch.equal(got, X) and torch.equal(BR.decode_masks(M, 64), bits)
