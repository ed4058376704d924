"""Every link of the backward chain against float64 ON ITS OWN STORED OPERANDS (tests/backward_referee.py has the referees, their
float32 yardsticks and the reasons; tests/test_backward_referee_cpu.py tests the referee).

One forward + backward through the C ABI per case; then, from the bytes that run left in the save area and the workspace:
  A  weight gradient = wgrad + wgrad_reduce against dY^T X / column sums of dY over the decoded areas: fp32, bf16, bf16x3 and the
     8-bit format (operands = dequantise(...));
  B  data gradient, layer by layer, from the STORED dY_l (plane formats; the 8-bit format's chain is held bit-identical to them by
     tests/test_q8_saves_gpu.py), on the launch plan of the pass and, bf16x3, on the pinned 8-wave and 4-wave launches;
  C  pose tail: dv, dp in the workspace, then d_center / d_dir from the STORED dp, dv, d_len.

Bounds (derived in the referee module, asserted as they stand; the yardstick is recomputed in every run):
  A  element-wise |got - ref| <= 2 (rows + 2) 2^-24 (|dY|^T |X|); per parameter tensor rel. L2 <= 4 x yardstick, 4 x yardstick < 1e-4;
     yardstick = float32 in the kernel's summation shape: per split-K range (sparf_debug_wgrad_split) a running sum of 16-row partial
     products, then the splits in order; the bias sums, which involve no MFMA, in the kernel's exact order
  B  element-wise |got - ref| <= ulp_area(ref) + 2 (K + 2) 2^-24 (|W_eff|^T |dY|); bf16 areas: share of stored elements that are not
     the rounded referee's value <= 8 x yardstick share + 16 / elements (<= 1e-3; layers under 1e5 elements pooled per case, cases
     under 1e5 elements in all rely on the element-wise bound); fp32 areas: rel. L2 per layer <= 4 x yardstick
     (ulp_area: one unit in the last place of bf16 at ref, i.e. 2^(floor(log2 |ref|) - 7); 2^-8 |ref| is half of that at the top of
     a binade and fails an honest float32 evaluation, tests/test_backward_referee_cpu.py)
  C  rel. L2 of dv, dp, d_center, d_dir <= 4 x the float32 torch evaluation of the same formulas

The row counts of the last three cases come from the launch plan of the device the test runs on (sparf_debug_x3_dgrad_plan): one round
of 128-row tiles (all in 4 waves), 1.5 rounds of 256-row tiles (hybrid: a full round in 8 waves, the rest in 4, `row_begin` > 0 in
the second launch), and two ray segments of which the first has no gradient (active range [row_begin, rows), all in 8 waves); the
test FAILS if the plan it meets is another.

Measured on an MI355X (256 CUs), worst over the cases from 1 680 rows up, kernel / yardstick (all 75 cases pass; the all-4-wave, hybrid
and all-8-wave plans were the ones met):
  fp32       A rel. L2 1.1e-6 / 3.5e-7 (mlp_feat.7.weight at 98 304 rows: the fp32 MFMA's k-step is 2 rows, the yardstick's 16)
             B rel. L2 per layer 2.1e-7 / 2.1e-7    C dv 1.5e-7 / 1.5e-7, dp 2.7e-7 / 2.0e-7, d_center 6.4e-8 / 6.7e-8, d_dir 1.1e-7 / 1.1e-7
  bf16       A 4.3e-7 / 3.2e-7    B share off the referee 3.3e-5 / 3.3e-5 (worst ratio 1.1)    C dv 4.4e-8 / 4.9e-8, dp 9.3e-8 / 9.9e-8,
             d_center 6.0e-8 / 8.9e-8, d_dir 8.2e-8 / 8.2e-8
  bf16x3     A 4.4e-7 / 3.3e-7    B share 6.0e-5 / 2.6e-5 (worst ratio 2.8 of the 8 allowed; 8-wave, 4-wave and planned launches give the
             same figures)    C dv 1.2e-7 / 8.0e-8, dp 1.7e-7 / 1.9e-7, d_center 6.2e-8 / 7.2e-8, d_dir 7.7e-8 / 9.2e-8
  bf16+q8    A 4.2e-7 / 3.2e-7         bf16x3+q8  A 4.6e-7 / 4.2e-7
  bias gradients: bit-identical to the yardstick (no MFMA in that sum; its order is restated exactly).
A library built with -DSP_X3_DGRAD_PARTS=1 (weight heads only, the tail product gone) fails link B on every bf16x3 case while
tests/test_hip_gpu.py::test_pass_backward[bf16x3] still passes.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from sparf_amd import lib as L
from sparf_amd import ops
from tests import backward_referee as BR
from tests.golden.recipe import small_opt, make_state_dict
from tests.test_hip_gpu import dev, make_scene, params_list

pytestmark = pytest.mark.gpu

CASES = ["1x2", "3x5", "70x24", "333x64", "all4", "hybrid", "segments"]
PRECS = ["fp32", "bf16", "bf16x3", "bf16+q8", "bf16x3+q8"]


def _shape(case, lib):
    """-> (rays, samples, rays of an inactive first segment, the bf16x3 data-gradient plan the active rows must get)"""
    if "x" in case:
        R, N = (int(v) for v in case.split("x"))
        return R, N, 0, None
    cus = BR.dgrad_plan(lib, 1)[1]
    if case == "all4":                       # one round of 128-row tiles: 1 024 x 32 on 256 CUs
        return 4 * cus, 32, 0, "all4"
    if case == "hybrid":                     # 1.5 rounds of 256-row tiles: 1 536 x 64 on 256 CUs
        return 6 * cus, 64, 0, "hybrid"
    return 2 * cus + 3, 64, 2, "all8"        # 515 x 64 on 256 CUs, the first two rays without gradients


def _run_pass(prec_id, R, N, first, pose, seed=5):
    d = dev()
    lib = L.load()
    opt = small_opt(barf_c2f=[0.4, 0.7])
    sd = make_state_dict(opt, 21, progress=0.55)
    center, dirs, jitter, _ = make_scene(R, N, seed)
    t = O.sample_depth(opt, 1, R, N, [1.2, 5.2], "train", jitter)[0, :, :, 0].to(d).contiguous()
    c, dr = center.to(d).contiguous(), dirs.to(d).contiguous()
    plist = params_list(sd, d)
    packed = ops.pack_weights(plist, prec_id)
    c2f = ops.c2f_weights(sd["progress"].to(d), opt.barf_c2f, d)
    rs = np.random.RandomState(100 + seed)
    g = [torch.from_numpy(rs.uniform(-1, 1, size=s).astype(np.float32)).to(d) for s in ((R, 3), (R,), (R,), (R, N))]
    segs = [(0, first, 0.0), (first, R - first, 0.0)] if first else None
    fa, out, save, keep1 = ops.build_pass_fwd(prec_id, c, dr, t, None, 0.0, False, packed, c2f, True, segs=segs)
    s = L.stream_ptr(d)
    L.check(lib.sparf_pass_forward(ctypes.byref(fa), s), "fwd")
    grads = [(None,) * 4, tuple(x[first:].contiguous() for x in g)] if first else tuple(g)
    ba, gp, dc, dd, keep2 = ops.build_pass_bwd(prec_id, c, dr, t, None, 0.0, False, packed, c2f, save, out, grads, pose, segs=segs)
    ws = keep2[0]
    assert ws.data_ptr() == ba.ws
    ws.zero_()                               # (inactive rows' area contents are not part of any result; zeros make the decode finite)
    L.check(lib.sparf_pass_backward(ctypes.byref(ba), s), "bwd")
    torch.cuda.synchronize()
    return dict(lib=lib, plist=plist, c2f=c2f, center=c, dirs=dr, t=t, out=out, save=save, ws=ws, gp=gp, dc=dc, dd=dd, fa=fa, ba=ba,
                keep=(keep1, keep2, packed, g))


def _decode(P, prec, rows_total):
    """-> (X, G canonical float32 [rows_total, ...], mask bytes per tile, workspace offsets)"""
    lib, save, ws = P["lib"], P["save"], P["ws"]
    R, N = P["t"].shape
    off = BR.workspace_offsets(lib, L.PREC_IDS[prec], R, N, P["dc"] is not None)
    assert off["total"] == ws.numel() and off["grad"] == 0
    garea = ws[:off["d_sigma"]]
    if prec.endswith("+q8"):
        U, S, M = BR.decode_q8(save, BR.SAVE_BUFS, 9)
        Ug, Sg, _ = BR.decode_q8(garea, BR.GRAD_BUFS, 0)
        X, G = BR.dequantise(U, S, BR.SAVE_BUFS), BR.dequantise(Ug, Sg, BR.GRAD_BUFS)
    else:
        X, M = BR.decode_planes(save, BR.SAVE_BUFS, 9, fp32=prec == "fp32")
        G, _ = BR.decode_planes(garea, BR.GRAD_BUFS, 0, fp32=prec == "fp32")
    return X, G, M, off


def _f32(ws, off, n):
    return ws[off:off + 4 * n].view(torch.float32)


def _link_a(P, prec, X, G, row0, rows, report, fails, tag):
    lib = P["lib"]
    R, N = P["t"].shape
    nsplit, rps = BR.wgrad_split(lib, R * N, rows - row0)
    Xs, dYs = BR.layer_inputs(X[row0:rows]), BR.layer_grads(G[row0:rows])
    gp, o = P["gp"], 0
    worst = (0.0, 0.0, "")
    for l, (no, ni) in enumerate(BR.LAYER_SHAPES):
        refW, refb, magW, magb = BR.link_a_reference(dYs[l], Xs[l])
        yW, yb = BR.link_a_yardstick(dYs[l], Xs[l], nsplit, rps, fp32_operands=prec == "fp32")
        bW, bb = BR.link_a_bound(rows - row0, magW, magb)
        for name, n, ref, y, bound in ((".weight", no * ni, refW, yW, bW), (".bias", no, refb, yb, bb)):
            got = gp[o:o + n].view(ref.shape)
            o += n
            name = BR.PARAM_NAMES[l] + name
            over = (got.double() - ref).abs() > bound
            if bool(over.any()):
                i = over.nonzero()[0].tolist()
                fails.append(f"{tag} A {name}: {int(over.sum())} elements past the element-wise bound; first at {i}: got {float(got[tuple(i)])!r} "
                             f"want {float(ref[tuple(i)])!r}; wgrad split {nsplit} x {rps} rows, active rows [{row0}, {rows})")
            ek, ey = BR.rel_l2(got, ref), BR.rel_l2(y, ref)
            if ek > worst[0]:
                worst = (ek, ey, name)
            if not 4 * ey < 1e-4:
                fails.append(f"{tag} A {name}: 4 x yardstick = {4 * ey:.2e} is not below 1e-4")
            if not ek <= 4 * ey:
                fails.append(f"{tag} A {name}: kernel {ek:.3e} > 4 x yardstick {ey:.3e}; wgrad split {nsplit} x {rps} rows, active rows [{row0}, {rows})")
    assert o == L.N_PARAMS
    report.append(f"{tag} A worst tensor {worst[2]}: kernel {worst[0]:.2e} yardstick {worst[1]:.2e} (split {nsplit} x {rps})")


def _link_b(P, prec, X, G, M, off, row0, rows, report, fails, tag, plan):
    R, N = P["t"].shape
    fmt = "fp32" if prec == "fp32" else "bf16"
    masks = BR.masks_feature(M, rows, X, strict=True)
    masks = {k: v[row0:rows] for k, v in masks.items()}
    grads = BR.named_grads(BR.layer_grads(G[row0:rows]))
    Weff = BR.effective_weights(P["plist"], prec)
    d_sigma, d_z = _f32(P["ws"], off["d_sigma"], R * N)[row0:rows], _f32(P["ws"], off["d_z"], R * N * 3).view(-1, 3)[row0:rows]
    fails += [f"{tag} B first link ({plan}): {m}" for m in BR.first_link(grads, d_sigma, d_z, fmt)]
    pool = [0, 0, 0]                                                   # kernel mismatches, yardstick mismatches, elements
    lines = []
    for name, l, (c0, c1), src in BR.CHAIN:
        ref, bound, _ = BR.link_b_reference(name, grads, masks, Weff, fmt)
        y = BR.link_b_yardstick(name, grads, masks, P["plist"], prec)
        got = grads[name][:, 1:] if name == "dY7" else grads[name]
        if bool(((got.double() - ref).abs() > bound).any()):
            fails.append(f"{tag} B ({plan}) " + BR.describe_mismatch(name, got, ref, bound))
        if fmt == "fp32":
            ek, ey = BR.rel_l2(got, ref), BR.rel_l2(y, ref)
            lines.append(f"{name} {ek:.1e}/{ey:.1e}")
            if not ek <= 4 * ey:
                fails.append(f"{tag} B ({plan}) {name}: kernel rel. L2 {ek:.3e} > 4 x yardstick {ey:.3e}")
            continue
        nk, ny, n = int((got.double() != ref).sum()), int((y.double() != ref).sum()), ref.numel()
        lines.append(f"{name} {nk / n:.1e}/{ny / n:.1e}")
        if n < 1e5:
            pool = [pool[0] + nk, pool[1] + ny, pool[2] + n]
            continue
        limit = 8 * ny / n + 16 / n
        if not limit <= 1e-3:
            fails.append(f"{tag} B ({plan}) {name}: the bound of the share, {limit:.2e}, exceeds 1e-3")
        if not nk / n <= limit:
            fails.append(f"{tag} B ({plan}) {name}: share of stored elements off the rounded referee {nk / n:.3e} > 8 x yardstick {ny / n:.3e} + 16 / {n}")
    if pool[2] >= 1e5:
        limit = 8 * pool[1] / pool[2] + 16 / pool[2]
        if not (limit <= 1e-3 and pool[0] / pool[2] <= limit):
            fails.append(f"{tag} B ({plan}) pooled layers: share {pool[0] / pool[2]:.3e}, yardstick {pool[1] / pool[2]:.3e}, bound {limit:.3e}")
    report.append(f"{tag} B ({plan}) kernel/yardstick " + ("rel. L2" if fmt == "fp32" else "share off the referee") + ": " + " ".join(lines))
    return grads, Weff


def _link_c(P, grads, Weff, off, row0, rows, report, fails, tag, plan, rays):
    """dv, dp of the workspace against the referee on the stored gradients; with `rays` d_center / d_dir on the stored dp, dv, d_len"""
    R, N = P["t"].shape
    ray0, ws = row0 // N, P["ws"]
    c, dr, t, c2f = P["center"][ray0:], P["dirs"][ray0:], P["t"][ray0:], P["c2f"]
    dp = _f32(ws, off["dp"], R * N * 3).view(-1, 3)[row0:rows]
    dv = BR.decode_dv(_f32(ws, off["dv"], R * N * 32).view(-1, 32)[row0:rows])
    W32 = [w.float() for w in Weff]                                     # (head + tail is not always a float32 number: rounded once here)
    rv, rp = BR.pose_reference(grads, Weff, c, dr, t, c2f)
    yv, yp = BR.pose_reference(grads, W32, c, dr, t, c2f, dtype=torch.float32)
    checks = [("dv", dv, rv, yv), ("dp", dp, rp, yp)]
    if rays:
        d_len, raylen = _f32(ws, off["d_len"], R)[ray0:], P["out"]["raylen"][ray0:]
        rc, rd = BR.ray_reference(dp, dv, d_len, dr, raylen, t, c2f)
        yc, yd = BR.ray_reference(dp, dv, d_len, dr, raylen, t, c2f, dtype=torch.float32)
        checks += [("d_center", P["dc"][ray0:], rc, yc), ("d_dir", P["dd"][ray0:], rd, yd)]
        if ray0 > 0 and not (bool((P["dc"][:ray0] == 0).all()) and bool((P["dd"][:ray0] == 0).all())):
            fails.append(f"{tag} C: rays of the inactive segment received a gradient")
    line = []
    for name, got, ref, y in checks:
        ek, ey = BR.rel_l2(got, ref), BR.rel_l2(y, ref)
        line.append(f"{name} {ek:.1e}/{ey:.1e}")
        if not ek <= 4 * ey:
            fails.append(f"{tag} C ({plan}) {name}: kernel rel. L2 {ek:.3e} > 4 x yardstick {ey:.3e}")
    report.append(f"{tag} C ({plan}) kernel/yardstick rel. L2: " + " ".join(line))


@pytest.mark.parametrize("pose", [False, True], ids=["fixed_pose", "pose_grad"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", CASES)
def test_backward_links(case, prec, pose):
    lib = L.load()
    R, N, first, want_plan = _shape(case, lib)
    prec_id = L.PREC_IDS[prec]
    rows_total, row0 = R * N, first * N
    rows8, cus, plan = BR.dgrad_plan(lib, rows_total - row0)
    if want_plan is not None:
        assert plan == want_plan, f"{case}: {rows_total - row0} active rows on {cus} CUs are planned {plan} (rows8 = {rows8}), not {want_plan}"
    P = _run_pass(prec_id, R, N, first, pose)
    tag = f"[{case} {R}x{N} {prec} {'pose' if pose else 'fixed'}]"
    report, fails = [], []
    X, G, M, off = _decode(P, prec, rows_total)
    if not BR.check_pad_rows_zero(G, rows_total):
        fails.append(f"{tag}: the gradient area's rows past the last row of its 32-row tile are not zero")
    _link_a(P, prec, X, G, row0, rows_total, report, fails, tag)
    if not prec.endswith("+q8"):
        x3 = prec == "bf16x3"
        launches = [(1, f"plan {plan}, rows8 = {rows8} on {cus} CUs" if x3 else "the pass")]
        if x3 and not first:                                             # (the pinned launches cover [0, rows): not for the segmented case)
            launches += [(3, "pinned 8 waves"), (4, "pinned 4 waves")]
        for i, (which, name) in enumerate(launches):
            if i > 0:
                L.check(lib.sparf_launch_kernel(which, ctypes.byref(P["fa"]), ctypes.byref(P["ba"]), L.stream_ptr(dev())), "dgrad")
                torch.cuda.synchronize()
                G, _ = BR.decode_planes(P["ws"][:off["d_sigma"]], BR.GRAD_BUFS, 0, fp32=prec == "fp32")
            grads, Weff = _link_b(P, prec, X, G, M, off, row0, rows_total, report, fails, tag, name)
            if pose:                                                     # (d_center / d_dir are the pass's own: ray_reduce ran behind its launches)
                _link_c(P, grads, Weff, off, row0, rows_total, report, fails, tag, name, rays=i == 0)
    else:
        BR.masks_feature(M, rows_total, X, strict=False)                # 8-bit saves: a positive stored value has its bit set
    print("\n".join(report))
    assert not fails, "\n".join(fails)
    torch.cuda.empty_cache()


def _poison_planes(area, bufs, n_mask_kib, fp32, rows_from, pad_cols, value):
    """in place: every element of rows >= rows_from, and the padding columns of every row, := value"""
    eb, ch, dt = (4, 4, torch.float32) if fp32 else (2, 8, torch.bfloat16)
    cols = sum(bufs)
    tile_bytes = cols * 32 * eb + n_mask_kib * 1024
    ntiles = area.numel() // tile_bytes
    blocks = area[:ntiles * tile_bytes].view(ntiles, tile_bytes)
    row = torch.arange(ntiles * 32, device=area.device).view(ntiles, 1, 32, 1)
    off = 0
    for C in bufs:
        vals = blocks[:, off * 32 * eb:(off + C) * 32 * eb].view(dt).view(ntiles, C // ch, 32, ch)        # [tile][chunk][row][el], a view
        vals.masked_fill_(row >= rows_from, value)
        for col in pad_cols[off:off + C].nonzero().flatten().tolist():
            h, q = col // (C // 2), col % (C // 2)
            pos = (q // ch) * 2 * ch + h * ch + q % ch
            vals[:, pos // ch, :, pos % ch] = value
        off += C


def _poison_q8(area, bufs, n_mask_kib, rows_from, pad_cols):
    """in place: rows >= rows_from := byte 255 with step 1e30; the padding columns of every row := byte 255"""
    cols = sum(bufs)
    tile_bytes = cols * 32 + n_mask_kib * 1024 + len(bufs) * 256
    ntiles = area.numel() // tile_bytes
    blocks = area[:ntiles * tile_bytes].view(ntiles, tile_bytes)
    row = torch.arange(ntiles * 32, device=area.device).view(ntiles, 32)
    off = 0
    for C in bufs:
        raw = blocks[:, off * 32:(off + C) * 32].view(ntiles, C // 32, 2, 32, 16)                       # [tile][block][h][row][slot]
        raw.masked_fill_((row >= rows_from).view(ntiles, 1, 1, 32, 1), 255)
        for col in pad_cols[off:off + C].nonzero().flatten().tolist():
            h, q = col // (C // 2), col % (C // 2)
            raw[:, q // 16, h, :, q % 16] = 255
        off += C
    so = cols * 32 + n_mask_kib * 1024
    steps = blocks[:, so:so + len(bufs) * 256].view(torch.float32).view(ntiles, len(bufs), 2, 32)
    steps.masked_fill_((row >= rows_from).view(ntiles, 1, 1, 32), 1e30)


@pytest.mark.parametrize("prec", PRECS)
def test_weight_gradient_reads_no_padding(prec):
    """Padding columns (x0 slot 63, view slots 27..31, the unused slots of DZ and of DY7's last block) and rows past `rows` must not
    contribute: the padded tail of both areas is overwritten with large finite values and the weight-gradient kernels are relaunched
    alone.  Save area: every row >= rows.  Gradient area: every row from the end of the last row's 32-row tile on -- inside that tile
    the data-gradient kernel's zeros ARE the contract (wgrad.hip reads whole ring slots; asserted by test_backward_links)."""
    R, N = 70, 24
    rows = R * N
    lib = L.load()
    P = _run_pass(L.PREC_IDS[prec], R, N, 0, False)
    before = P["gp"].clone()
    off = BR.workspace_offsets(lib, L.PREC_IDS[prec], R, N, False)
    garea = P["ws"][:off["d_sigma"]]
    ps, pg = BR.padding_columns(BR.SAVE_BUFS, "save"), BR.padding_columns(BR.GRAD_BUFS, "grad")
    gfrom = (rows + 31) // 32 * 32
    if prec.endswith("+q8"):
        _poison_q8(P["save"], BR.SAVE_BUFS, 9, rows, ps)
        _poison_q8(garea, BR.GRAD_BUFS, 0, gfrom, pg)
    else:
        _poison_planes(P["save"], BR.SAVE_BUFS, 9, prec == "fp32", rows, ps, 2.0 ** 50)
        _poison_planes(garea, BR.GRAD_BUFS, 0, prec == "fp32", gfrom, pg, 2.0 ** 50)
    X, G, _, _ = _decode(P, prec, rows)
    assert float(X[rows:].abs().min()) >= 1e15 and float(G[gfrom:].abs().min()) >= 1e15              # (the poison is in place)
    P["gp"].fill_(float("nan"))
    L.check(lib.sparf_launch_kernel(2, ctypes.byref(P["fa"]), ctypes.byref(P["ba"]), L.stream_ptr(dev())), "wgrad")
    torch.cuda.synchronize()
    assert torch.equal(P["gp"], before), f"{int((P['gp'] != before).sum())} parameter gradients changed"
