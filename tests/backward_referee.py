"""Float64 referee of the backward pass, link by link, on the operands the kernels themselves left in memory.

The forward's save area and the data-gradient kernel's gradient area (csrc/layout.h "AREAS") hold, as bf16 / fp32 / 8-bit values,
exactly what the next kernel multiplies.  Given those bytes the correct output of every link of the backward chain is a fixed float64
expression with no ReLU decision left in it:

  link A  weight gradient   dW_l = dY_l^T X_l, db_l = sum over rows of dY_l                       (wgrad.hip + wgrad_reduce_kernel)
  link B  data gradient     dY_{l-1} = mask_{l-1} * (W_eff,l[:, segment]^T dY_l), rounded once    (mlp_bwd_impl.h)
  link C  pose tail         dv, dp (encoding backward of d x0), then d_center / d_dir             (mlp_bwd_impl.h, ray_reduce_kernel)

Everything here is plain torch on whatever device the operands live on; nothing reads the library except the host-only layout
queries `workspace_offsets`, `dgrad_plan` and `wgrad_split`.  Every referee comes with its YARDSTICK: the same expression evaluated by torch in
float32 on the same operands.  Bounds of the tests are multiples of the yardstick's own distance to float64, computed in every run.

Conventions
  * "canonical order" of a decoded buffer: column = h * (C / 2) + q for lane half h and register slot q (layout.h pos_of).
  * "feature order": the nn.Linear index of a layer input / output (X_l [rows, layer_in], dY_l [rows, layer_out]); the maps
    canonical -> feature restate layout.h crow_of / x0_feat / view_feat / out_row_of_crow.
  * ReLU decisions: the FULL bit order of the mask words (layout.h "ReLU masks") is decoded (`decode_masks`): the referee takes its
    decisions from the bits the data-gradient kernel pops, and `masks_feature` cross-checks them -- bit set exactly where the saved
    activation of that column is > 0 -- for the plane formats (in the 8-bit format a small positive activation is stored as 0: there
    the bits are the only record of the decision, and the cross-check is one-sided: a positive stored value has its bit set).
  * What is stored is what is consumed: mlp_bwd_impl.h `masked_units` / `masked_to` pack the masked pair with ONE conversion
    (v_cvt_pk_bf16_f32, round to nearest even) into the B operand `out[]`, and `store_slice` stores that operand.  The bf16x3
    data-gradient chain keeps dY as plain bf16 and multiplies it with head + tail weights (mlp_dev.h PolicyX3DgradT: two MFMAs per
    k-step into one accumulator); d x0 and d view leave the accumulators as fp32, unmasked.  The 8-bit format is the exception:
    its gradient area holds the QUANTISED image of the bf16 operand the chain consumed (mlp_bwd_impl.h store_slice, Q8 branch), so
    links B and C cannot be cut there; tests/test_q8_saves_gpu.py holds that chain bit-identical to the plane format's, and link A
    takes the 8-bit operands as `dequantise` gives them, which is what wgrad.hip convert_q8 multiplies.
  * Rows past `rows` of the last 32-row tile: the data-gradient kernel stores zeros there (mlp_bwd_impl.h: `valid` gates d_z and
    d_sigma, everything downstream is linear in them) and the weight-gradient kernel reads whole ring slots (wgrad.hip `ntiles`): it
    relies on those zeros.  `check_pad_rows_zero` asserts them; tiles past the last row's tile are never read.
"""
import ctypes

import torch

SAVE_BUFS = [320, 256, 256, 256, 256, 256, 256, 288, 128]                 # csrc/layout.h SaveBuf: XS H0 H1 H2 H4 H5 H6 FV G
GRAD_BUFS = [256] * 7 + [288, 128, 32]                                   # csrc/layout.h GradBuf: DY0..DY6 DY7 DG DZ
SB_XS, SB_H0, SB_H1, SB_H2, SB_H4, SB_H5, SB_H6, SB_FV, SB_G = range(9)
GB_DY7, GB_DG, GB_DZ = 7, 8, 9
N_LAYERS = 10
LAYER_SHAPES = [(256, 63), (256, 256), (256, 256), (256, 256), (256, 319), (256, 256), (256, 256), (257, 256), (128, 283), (3, 128)]
PARAM_NAMES = [f"mlp_feat.{i}" for i in range(8)] + ["mlp_rgb.0", "mlp_rgb.1"]
U24 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- area decoders
def _canon(x, C, ch):
    """[rows][pos] -> canonical column = h * (C / 2) + q, pos = (q // ch) * 2 ch + h * ch + q % ch (layout.h pos_of)"""
    pos = torch.arange(C, device=x.device)
    q = (pos // (2 * ch)) * ch + pos % ch
    h = (pos // ch) % 2
    return x[:, torch.argsort(h * (C // 2) + q)]


def decode_planes(area, bufs, n_mask_kib, fp32=False):
    """plane area (bf16, or fp32 with fp32=True) -> ([rows_padded, sum(bufs)] float32 in canonical order per buffer, mask bytes per tile)"""
    eb, ch, dt = (4, 4, torch.float32) if fp32 else (2, 8, torch.bfloat16)
    cols = sum(bufs)
    tile_bytes = cols * 32 * eb + n_mask_kib * 1024
    ntiles = area.numel() // tile_bytes
    blocks = area[:ntiles * tile_bytes].view(ntiles, tile_bytes)
    out, off = [], 0
    for C in bufs:
        raw = blocks[:, off * 32 * eb:(off + C) * 32 * eb].contiguous()
        vals = raw.view(dt).view(ntiles, C // ch, 32, ch).float()                            # [tile][chunk][row][el]
        out.append(_canon(vals.permute(0, 2, 1, 3).reshape(ntiles * 32, C), C, ch))
        off += C
    return torch.cat(out, dim=1), blocks[:, cols * 32 * eb:cols * 32 * eb + n_mask_kib * 1024]


def decode_q8(area, bufs, n_mask_kib):
    """8-bit area -> (u [rows_padded, sum(bufs)] int32 canonical, steps [rows_padded, len(bufs), 2] float32, mask bytes per tile)"""
    cols = sum(bufs)
    tile_bytes = cols * 32 + n_mask_kib * 1024 + len(bufs) * 256
    ntiles = area.numel() // tile_bytes
    blocks = area[:ntiles * tile_bytes].view(ntiles, tile_bytes)
    out, off = [], 0
    for C in bufs:
        raw = blocks[:, off * 32:(off + C) * 32].contiguous().view(ntiles, C // 32, 2, 32, 16)     # [tile][block][h][row][slot in block]
        u = raw.permute(0, 3, 2, 1, 4).reshape(ntiles * 32, C).int()                               # [row][h][block][slot] = h * C/2 + q
        out.append(u)
        off += C
    so = cols * 32 + n_mask_kib * 1024
    steps = blocks[:, so:so + len(bufs) * 256].contiguous().view(torch.float32).view(ntiles, len(bufs), 2, 32)
    steps = steps.permute(0, 3, 1, 2).reshape(ntiles * 32, len(bufs), 2)
    return torch.cat(out, dim=1), steps, blocks[:, cols * 32:so]


def encode_planes(X, bufs, tail):
    """inverse of decode_planes: canonical-order values [rows_padded, sum(bufs)] -> bf16 plane area bytes; `tail`: the bytes that follow
    the planes in every tile block (mask words), [ntiles, n] uint8"""
    ntiles = X.shape[0] // 32
    parts, off = [], 0
    for C in bufs:
        pos = torch.arange(C, device=X.device)
        q = (pos // 16) * 8 + pos % 8
        h = (pos // 8) % 2
        order = torch.argsort(h * (C // 2) + q)
        x = torch.empty(X.shape[0], C, device=X.device)
        x[:, order] = X[:, off:off + C]
        vals = x.view(ntiles, 32, C // 8, 8).permute(0, 2, 1, 3).contiguous().to(torch.bfloat16)
        parts.append(vals.view(torch.uint8).reshape(ntiles, C * 64))
        off += C
    return torch.cat(parts + [tail], dim=1).reshape(-1)


def dequantise(U, S, bufs):
    """what the weight-gradient kernel multiplies out: bf16(fma(u, step, -128 step)), canonical order, as float32"""
    out, off = [], 0
    for b, C in enumerate(bufs):
        half = C // 2
        part = ((torch.arange(C, device=U.device) % half) >= 128).long()
        st = S[:, b, :][:, part].double()                                                # [rows, C]
        v = (U[:, off:off + C].double() * st - 128.0 * st).float()                       # exact in float64, one rounding to float32 = the FMA
        out.append(v.to(torch.bfloat16).float())
        off += C
    return torch.cat(out, dim=1)


def decode_save(save, rows, fp32):
    """plane save area -> (X [rows, 2272] float32 canonical, mask words [tiles, 9, 64, 4] int32)"""
    X, M = decode_planes(save, SAVE_BUFS, 9, fp32)
    return X[:rows], M.contiguous().view(torch.int32).view(-1, 9, 64, 4)


def decode_masks(mask_bytes, rows):
    """mask bytes per tile [tiles, 9 KiB] (uint8) -> bool [rows, 9, 256] in canonical order (h * 128 + q; the 128-wide G: q < 64 of each
    half, the rest False).  layout.h "ReLU masks": lane (n, h) = n + 32 h owns four words of a buffer, word p carries m-blocks 2p and
    2p + 1, element e = 16 * (mb & 1) + r of it at bit 31 - e; slot q = 16 mb + r, so q sits in word q // 32 at bit 31 - q % 32."""
    w = mask_bytes.contiguous().view(torch.int32).view(-1, 9, 64, 4).long() & 0xFFFFFFFF          # [tile][buffer][lane][word]
    ntiles = w.shape[0]
    q = torch.arange(128, device=w.device)
    bits = (w[:, :, :, q // 32] >> (31 - q % 32)) & 1                                             # [tile][buffer][lane][q]
    bits = bits.view(ntiles, 9, 2, 32, 128).permute(0, 3, 1, 2, 4).reshape(ntiles * 32, 9, 256)   # [row][buffer][h * 128 + q]
    out = bits[:rows].bool()
    out[:, SB_G] &= ((torch.arange(256, device=w.device) % 128) < 64)[None, :]
    return out


# ------------------------------------------------------------------------------------------- canonical order <-> feature order
def _crow(q, h):
    return 32 * (q >> 4) + (q & 3) + 8 * ((q & 15) >> 2) + 4 * h


def _x0_feat(q, h):
    if q < 30:
        a = 15 * h + (q >> 1)
        return 3 + (a // 10) * 20 + (q & 1) * 10 + (a % 10)
    if q == 30:
        return 0 if h == 0 else 2
    return 1 if h == 0 else -1


def _view_feat(q, h):
    if q < 12:
        a = 6 * h + (q >> 1)
        return 3 + (a // 4) * 8 + (q & 1) * 4 + (a % 4)
    if q == 12:
        return 0 if h == 0 else 2
    if q == 13:
        return 1 if h == 0 else -1
    return -1


def _index(C, nfeat, feat_of):
    """feature -> canonical column of a C-wide buffer; feat_of(q, h) -> feature or -1"""
    idx = [-1] * nfeat
    for h in (0, 1):
        for q in range(C // 2):
            f = feat_of(q, h)
            if f >= 0:
                assert idx[f] == -1
                idx[f] = h * (C // 2) + q
    assert min(idx) >= 0
    return idx


_HID256 = _index(256, 256, _crow)
_HID128 = _index(128, 128, _crow)
_XS = _index(320, 319, lambda q, h: _crow(q, h) if q < 128 else (256 + _x0_feat(q - 128, h) if _x0_feat(q - 128, h) >= 0 else -1))
_FV = _index(288, 283, lambda q, h: _crow(q, h) if q < 128 else (256 + _view_feat(q - 128, h) if _view_feat(q - 128, h) >= 0 else -1))
_DY7 = _index(288, 257, lambda q, h: _crow(q, h) + 1 if q < 128 else (0 if (q == 128 and h == 0) else -1))
_DZ = _index(32, 3, lambda q, h: _crow(q, h) if _crow(q, h) < 3 else -1)
# dv rows of the workspace: [row][32] fp32 in pos layout with CH = 4 (mlp_bwd_impl.h, ray_reduce_kernel): feature -> pos
_DV_POS = [-1] * 27
for _h in (0, 1):
    for _q in range(16):
        if _view_feat(_q, _h) >= 0:
            _DV_POS[_view_feat(_q, _h)] = (_q // 4) * 8 + _h * 4 + _q % 4


def _buf(X, bufs, b):
    o = sum(bufs[:b])
    return X[:, o:o + bufs[b]]


def layer_inputs(X):
    """decoded save area (canonical, [rows, 2272]) -> list of the ten layer inputs X_l [rows, layer_in(l)] in nn.Linear order
    (layout.h wjob: layer 0 reads x0 out of XS, the skip layer 4 = [h3 | x0] = XS, layer 8 = [feat | view] = FV, layer 9 = G)"""
    ix = lambda l: torch.tensor(l, device=X.device)
    xs = _buf(X, SAVE_BUFS, SB_XS)[:, ix(_XS)]
    hid = lambda b: _buf(X, SAVE_BUFS, b)[:, ix(_HID256)]
    return [xs[:, 256:], hid(SB_H0), hid(SB_H1), hid(SB_H2), xs, hid(SB_H4), hid(SB_H5), hid(SB_H6),
            _buf(X, SAVE_BUFS, SB_FV)[:, ix(_FV)], _buf(X, SAVE_BUFS, SB_G)[:, ix(_HID128)]]


def layer_grads(G):
    """decoded gradient area (canonical, [rows, 2240]) -> list of the ten pre-activation gradients dY_l [rows, layer_out(l)] in
    nn.Linear row order (raw density = row 0 of layer 7: the q = 128, h = 0 slot of DY7)"""
    ix = lambda l: torch.tensor(l, device=G.device)
    out = [_buf(G, GRAD_BUFS, l)[:, ix(_HID256)] for l in range(7)]
    return out + [_buf(G, GRAD_BUFS, GB_DY7)[:, ix(_DY7)], _buf(G, GRAD_BUFS, GB_DG)[:, ix(_HID128)], _buf(G, GRAD_BUFS, GB_DZ)[:, ix(_DZ)]]


def padding_columns(bufs, which):
    """canonical columns of the concatenated area that carry no feature (which = "save" / "grad"): bool [sum(bufs)]"""
    used = torch.zeros(sum(bufs), dtype=torch.bool)
    real = dict(save={SB_XS: _XS, SB_FV: _FV, SB_G: _HID128}, grad={GB_DY7: _DY7, GB_DG: _HID128, GB_DZ: _DZ})[which]
    for b, C in enumerate(bufs):
        o = sum(bufs[:b])
        used[torch.tensor(real.get(b, _HID256)) + o] = True
    return ~used


def masks_feature(mask_bytes, rows, X=None, strict=True):
    """mask words -> dict of bool [rows, width] in feature order, keyed by the gradient they gate: "dY0".."dY6" (256), "dY7" (the 256
    feature rows 1..256 of layer 7), "dG" (128).  With X (decoded save area, canonical) the bits are cross-checked against the saved
    activations: strict = bit set exactly where the value is > 0 (plane formats); otherwise only value > 0 => bit set (8-bit format)."""
    M = decode_masks(mask_bytes, rows)
    ix = lambda l: torch.tensor(l, device=M.device)
    src = {"dY0": SB_H0, "dY1": SB_H1, "dY2": SB_H2, "dY3": SB_XS, "dY4": SB_H4, "dY5": SB_H5, "dY6": SB_H6, "dY7": SB_FV, "dG": SB_G}
    out = {}
    for k, b in src.items():
        m = M[:, b]
        out[k] = m[:, ix(_HID256)] if b != SB_G else torch.cat([m[:, :64], m[:, 128:192]], dim=1)[:, ix(_HID128)]
        if X is not None:
            xb = _buf(X[:rows], SAVE_BUFS, b)
            act = (xb[:, ix(_XS)][:, :256] if b == SB_XS else xb[:, ix(_FV)][:, :256] if b == SB_FV else xb[:, ix(_HID128)] if b == SB_G
                   else xb[:, ix(_HID256)]) > 0
            bad = (act != out[k]) if strict else (act & ~out[k])
            if bool(bad.any()):
                r, c = bad.nonzero()[0].tolist()
                raise AssertionError(f"mask bits of {k} disagree with the saved activations at {int(bad.sum())} places; first: row {r} (tile {r // 32}) "
                                     f"feature {c}: bit {bool(out[k][r, c])}, saved activation > 0: {bool(act[r, c])}")
    return out


# ------------------------------------------------------------------------------------------------------------ effective weights
def _scale2(x, e):
    """x * 2^e exactly (2^e built from its bit pattern: torch.ldexp goes through pow(), which is not exact on every device)"""
    return x * ((e.long() + 1023) << 52).view(torch.float64)


def round_bf16(x):
    """float64 -> nearest bf16 value (ties to even), as float64 -- one rounding (torch's double -> bfloat16 goes through float32)"""
    m, e = torch.frexp(x)
    return _scale2(torch.round(m * 256.0) / 256.0, e)


def ulp_bf16(x):
    """one unit in the last place of bf16 at x: 2^(e - 7) for 2^e <= |x| < 2^(e + 1), i.e. between 2^-8 |x| and 2^-7 |x|; 0 at 0.
    (2^-8 |x| itself is HALF a unit at the top of a binade: two neighbouring bf16 values just below a power of two are further apart
    than that, and an honest float32 evaluation of a link lands on the neighbour of the float64 referee's value about once in 2e4.)"""
    m, e = torch.frexp(x)
    return torch.where(x == 0, torch.zeros_like(x), _scale2(torch.ones_like(x), e - 8))


def trunc_bf16(x):
    m, e = torch.frexp(x)
    return _scale2(torch.trunc(m * 256.0) / 256.0, e)


def effective_weights(params, prec):
    """params: the 20 fp32 tensors (W0, b0, ...).  -> list of ten float64 [out, in] matrices the data-gradient chain multiplies with:
    fp32 W; bf16 bf16(W); bf16x3 head + tail, head = bf16(W), tail = bf16(W - head), both round to nearest even (pack.hip)"""
    out = []
    for l in range(N_LAYERS):
        W = params[2 * l].detach().float()
        if prec == "fp32":
            out.append(W.double())
        else:
            head = W.bfloat16().float()
            out.append(head.double() if prec == "bf16" else head.double() + (W - head).bfloat16().double())
    return out


# ---------------------------------------------------------------------------------------------------------- library layout queries
def workspace_offsets(lib, prec_id, nrays, nsamp, pose):
    out = (ctypes.c_int64 * 8)()
    assert lib.sparf_debug_bwd_workspace(prec_id, nrays, nsamp, int(pose), out) == 0
    return dict(zip(("grad", "d_sigma", "d_z", "d_len", "partial", "dp", "dv", "total"), [int(v) for v in out]))


def dgrad_plan(lib, rows):
    """-> (rows8, cus, name): rows [0, rows8) in the 8-wave kernel, the rest in the 4-wave kernel; name = all8 / all4 / hybrid"""
    r8, cus = ctypes.c_int64(), ctypes.c_int()
    assert lib.sparf_debug_x3_dgrad_plan(rows, ctypes.byref(r8), ctypes.byref(cus)) == 0
    return r8.value, cus.value, "all8" if r8.value == rows else "all4" if r8.value == 0 else "hybrid"


def wgrad_split(lib, rows_total, rows_active):
    nt, na, rps = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.sparf_debug_wgrad_split(rows_total, rows_active, ctypes.byref(nt), ctypes.byref(na), ctypes.byref(rps)) == 0
    return na.value, rps.value


# ------------------------------------------------------------------------------------------------------------------------ link A
def link_a_reference(dY, X):
    """float64: (dW [out, in], db [out]) = (dY^T X, column sums of dY) and the magnitude sums |dY|^T |X|, sum |dY| of the bound"""
    dY, X = dY.double(), X.double()
    return dY.t() @ X, dY.sum(0), dY.abs().t() @ X.abs(), dY.abs().sum(0)


def link_a_yardstick(dY, X, nsplit, rows_per_split, drop_split=None, fp32_operands=False):
    """float32 in the kernel's summation shape: inside every split-K range a running fp32 sum of 16-row partial products (one MFMA
    k-step of wgrad.hip), then the fp32 sum over the splits in wgrad_reduce_kernel's order.  -> (dW, db) float32.
    The bias gradient involves no MFMA, so its shape is restated exactly (wgrad.hip `bsum` / WOps::fsum): a lane half owns rows
    [8 h, 8 h + 8) of every 16-row k-step (fp32 operands: row 2 kk + h of every 2-row k-step), sums them in order starting from 0, adds
    that to its running sum over the split's k-steps; the halves are added at the end of the split, the splits in order.
    (`drop_split`: a mutation for the referee's own test: that split's partial block is left out of the reduce)"""
    dY, X = dY.float(), X.float()
    total = torch.zeros(dY.shape[1], X.shape[1], device=X.device)
    total_b = torch.zeros(dY.shape[1], device=X.device)
    for s in range(nsplit):
        a, b = s * rows_per_split, min((s + 1) * rows_per_split, dY.shape[0])
        n = b - a
        if n <= 0 or s == drop_split:
            continue
        pad = (-n) % 16
        dy = torch.nn.functional.pad(dY[a:b], (0, 0, 0, pad)).view(-1, 16, dY.shape[1])
        xa = torch.nn.functional.pad(X[a:b], (0, 0, 0, pad)).view(-1, 16, X.shape[1])
        part = torch.bmm(dy.transpose(1, 2), xa)                                            # [16-row group][out][in]
        acc = torch.zeros_like(total)
        for k in range(part.shape[0]):
            acc += part[k]
        total += acc
        if fp32_operands:
            steps = dy.reshape(-1, 2, dY.shape[1])                                          # [k-step][h][out]: row 2 kk + h
        else:
            d8 = dy.view(-1, 2, 8, dY.shape[1])                                             # [k-step][h][row of the half][out]
            steps = torch.zeros(d8.shape[0], 2, dY.shape[1], device=X.device)
            for j in range(8):
                steps = steps + d8[:, :, j]
        bacc = torch.zeros(2, dY.shape[1], device=X.device)
        for k in range(steps.shape[0]):
            bacc += steps[k]
        total_b += bacc[0] + bacc[1]
    return total, total_b


def link_a_bound(rows, magW, magb):
    """element-wise: |got - ref| <= 2 (rows + 2) 2^-24 (|dY|^T |X|)"""
    f = 2.0 * (rows + 2) * U24
    return f * magW, f * magb


# ------------------------------------------------------------------------------------------------------------------------ link B
# the chain as mlp_bwd_impl.h runs it: (name of the output, layer whose W^T is applied, input column range of that layer, source dY)
CHAIN = [("dG", 9, (0, 128), "dZ"), ("dY7", 8, (0, 256), "dG"), ("dY6", 7, (0, 256), "dY7"), ("dY5", 6, (0, 256), "dY6"),
         ("dY4", 5, (0, 256), "dY5"), ("dY3", 4, (0, 256), "dY4"), ("dY2", 3, (0, 256), "dY3"), ("dY1", 2, (0, 256), "dY2"),
         ("dY0", 1, (0, 256), "dY1")]


def named_grads(dYs):
    """list of layer_grads -> dict dY0..dY7 (257 wide, column 0 = raw density), dG, dZ"""
    d = {f"dY{l}": dYs[l] for l in range(8)}
    d["dG"], d["dZ"] = dYs[8], dYs[9]
    return d


def link_b_reference(name, grads, masks, Weff, fmt):
    """float64 referee of one link from the STORED source gradient.  -> (ref rounded to the area's element type, element-wise bound,
    unrounded ref).  dY7's column 0 (raw density) is not a product: it is compared with d_sigma by `first_link`."""
    out, l, (c0, c1), src = next(c for c in CHAIN if c[0] == name)
    dy = grads[src].double()
    W = Weff[l][:, c0:c1]
    acc = dy @ W
    mag = dy.abs() @ W.abs()
    ref = acc * masks[name].double()
    K = W.shape[0]
    rr = round_bf16(ref) if fmt != "fp32" else ref
    ulp = ulp_bf16(ref) if fmt != "fp32" else 0.0
    return rr, ulp + 2.0 * (K + 2) * U24 * mag, ref


def link_b_yardstick(name, grads, masks, params, prec):
    """the same expression in float32 torch on the same operands, rounded to the area's element type (bf16x3: the two products of a
    k-step go into ONE accumulation, as in the kernel: [dY | dY] @ [tail ; head])"""
    out, l, (c0, c1), src = next(c for c in CHAIN if c[0] == name)
    dy = grads[src].float()
    W = params[2 * l].detach().float()[:, c0:c1]
    if prec == "fp32":
        acc = dy @ W
    elif prec == "bf16":
        acc = dy @ W.bfloat16().float()
    else:
        head = W.bfloat16().float()
        acc = torch.cat([dy, dy], dim=1) @ torch.cat([(W - head).bfloat16().float(), head], dim=0)
    y = acc * masks[name].float()
    return y if prec == "fp32" else y.bfloat16().float()


def first_link(grads, d_sigma, d_z, fmt):
    """stored DZ and raw-density slot == the rounded d_z / d_sigma of composite_bwd_kernel; -> list of failure strings"""
    want_z, want_s = (d_z.double(), d_sigma.double()) if fmt == "fp32" else (round_bf16(d_z.double()), round_bf16(d_sigma.double()))
    bad = []
    for what, got, want, src in (("DZ", grads["dZ"].double(), want_z, d_z), ("raw-density slot of DY7", grads["dY7"][:, 0].double(), want_s, d_sigma)):
        ne = got != want
        if bool(ne.any()):
            i = tuple(ne.nonzero()[0].tolist())
            bad.append(f"{what} differs from the rounded {'d_z' if what == 'DZ' else 'd_sigma'} at {int(ne.sum())} of {ne.numel()} places; first at {list(i)}: "
                       f"stored {float(got[i])!r}, workspace value {float(src[i])!r} rounds to {float(want[i])!r}")
    return bad


def describe_mismatch(name, got, ref, bound):
    """the first element past its bound: row, 32-row tile, feature, values"""
    over = (got.double() - ref).abs() > bound
    r, c = over.nonzero()[0].tolist()
    return (f"{name}: {int(over.sum())} of {over.numel()} elements past the element-wise bound; first: row {r} (tile {r // 32}, row {r % 32} of it) "
            f"feature {c}: got {float(got[r, c])!r} want {float(ref[r, c])!r} bound {float(bound[r, c]) if torch.is_tensor(bound) else bound:.3e}; "
            f"rows affected {int(over.any(1).sum())}, features affected {int(over.any(0).sum())}")


# ------------------------------------------------------------------------------------------------------------------------ link C
PI32 = 3.14159274101257324219                    # float(pi) as fp32, the constant of mlp_bwd_impl.h / ray_ops.hip pe_freq


def decode_dv(dv):
    """workspace dv [rows, 32] (pos layout, CH = 4) -> [rows, 27] in the view encoding's feature order"""
    return dv[:, torch.tensor(_DV_POS, device=dv.device)]


def pose_reference(grads, Weff, center, dirs, t, c2f, dtype=torch.float64):
    """d view encoding (dv [rows, 27]) and d point (dp [rows, 3]) from the STORED dG, dY4, dY0:
        dv  = W_eff,8[:, 256:]^T dG
        dX0 = W_eff,0^T dY0 + W_eff,4[:, 256:]^T dY4            ([p(3), per coordinate: 10 sin, 10 cos])
        dp_c = dX0[c] + sum_k w_k f_k (cos(a) dX0[sin c,k] - sin(a) dX0[cos c,k]),  a = fl32(p_c f_k),  p = fl32(center + fl32(dir t))
    dtype = float64: the referee; float32: the yardstick.  The sample point and the encoding arguments are formed in the dtype of
    center / dirs / t: float32 tensors reproduce the kernel's (and the reference's) rounding of them, which is part of the function;
    float64 tensors are for comparisons with float64 autograd."""
    R, N = t.shape
    W = [w.to(dtype) for w in Weff]
    dv = grads["dG"].to(dtype) @ W[8][:, 256:]
    dx0 = grads["dY0"].to(dtype) @ W[0] + grads["dY4"].to(dtype) @ W[4][:, 256:]
    p = (center[:, None, :] + dirs[:, None, :] * t[:, :, None]).reshape(R * N, 3)
    fr = torch.tensor([PI32 * 2.0 ** k for k in range(10)], dtype=t.dtype, device=t.device)           # exact: powers of two times fl32(pi)
    arg = (p[:, :, None] * fr).to(dtype)                                                                # the product in the inputs' precision
    wk = (c2f[:10].to(dtype) * fr.to(dtype))
    enc = dx0[:, 3:].reshape(R * N, 3, 2, 10)
    dp = dx0[:, :3] + (wk * (arg.cos() * enc[:, :, 0] - arg.sin() * enc[:, :, 1])).sum(-1)
    return dv, dp


def ray_reference(dp, dv, d_len, dirs, raylen, t, c2f, dtype=torch.float64):
    """ray_reduce_kernel's formula over the STORED dp [rows, 3], dv [rows, 27] (feature order), d_len [rays]:
        d_center = sum_i dp_i;   d_dir = sum_i t_i dp_i + d_len dir / len + (g - (g . d) d) / len,  d = dir / len,
        g_c = sum_i dv_i[c] + sum_k w_k f_k (cos(b) sum_i dv_i[sin c,k] - sin(b) sum_i dv_i[cos c,k]),  b = fl32(d_c f_k)"""
    R, N = t.shape
    dp, dv = dp.to(dtype).view(R, N, 3), dv.to(dtype).view(R, N, 27)
    tt = t.to(dtype)
    d_center = dp.sum(1)
    sr = (tt[:, :, None] * dp).sum(1)
    dvs = dv.sum(1)
    inv = raylen.clamp_min(1e-12)
    d32 = dirs / inv[:, None]                                                                           # (in the inputs' precision, as above)
    fr = torch.tensor([PI32 * 2.0 ** k for k in range(4)], dtype=t.dtype, device=t.device)
    arg = (d32[:, :, None] * fr).to(dtype)
    wk = c2f[10:14].to(dtype) * fr.to(dtype)
    enc = dvs[:, 3:].reshape(R, 3, 2, 4)
    g = dvs[:, :3] + (wk * (arg.cos() * enc[:, :, 0] - arg.sin() * enc[:, :, 1])).sum(-1)
    d, invd = d32.to(dtype), inv.to(dtype)[:, None]
    d_dir = sr + d_len.to(dtype)[:, None] * dirs.to(dtype) / invd + (g - (g * d).sum(1, keepdim=True) * d) / invd
    return d_center, d_dir


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def check_pad_rows_zero(G, rows):
    """rows [rows, end of their 32-row tile) of the decoded gradient area are exact zeros (see the module docstring)"""
    end = (rows + 31) // 32 * 32
    return bool((G[rows:end] == 0).all())
