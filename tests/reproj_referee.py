"""Float64 referee of the correspondence loss (tests/test_reproj_cpu.py, tests/test_reproj_gpu.py): the formulas as
include/sparf_hip.h states them, in torch.float64 on the CPU on the fp32 operands cast to double, with autograd for the gradients --
so the hand-derived seeds of csrc/reproj.hip are checked against a derivation they do not share.  (The reference's own method cannot
run in float64: it calls .float() on the pixels.)

Bounds (the issue's, from the arithmetic contract: double arithmetic on the fp32 operands, double sums, one rounding per stored value):
the loss and each stat within ONE fp32 spacing of the float64 value -- a double result rounded once is within half a spacing, the other
half covers the referee's own summation order; each d depth_i element likewise; every gradient tensor (d depth, d T, d pose) relative
L2 <= 2^-22 -- a correctly rounded tensor is <= 2^-24, the margin covers cancellation in the 16 sums of d T; the valid mask EQUAL (the
fixture keeps every match 0.01 px / 1e-4 away from its threshold, tests/golden/make_reproj_golden.py).  The torch restatement
(sparf_amd.losses.*_torch) runs in fp32 like the reference and is held to 4x the reference's own distance from this referee.

Fixture names (tests/golden/reproj.npz):
  t<n>_{pi,di,pj,dj,w,Ki,Kj,T}              one scene per size; pi is an integer pixel grid stored as float32
  t<n>_<case>_{loss,d_di,d_T,valid,stats}   the reference's fp32 results; stats = (perc_val_pix_rep, perc_val_depth_rep), 0 where off
  p<n>_{ps,po,ds,do,fs,fo,w,Ks,Ko,Ps,Po}    pair scenes: pixels, depths, fine depths, weights, intrinsics, w2c poses [4,4]
  p<n>_f<0|1>_<case>_{loss,d_ds,d_do,d_fs,d_fo,d_Ps,d_Po,stats}     stats = (pix, depth, depth_in_corr_loss)
"""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reproj.npz")
# 63 / 65: one lane short of a wave and one over; 257: a second pass of the 256-thread workgroup with one live lane; 4096 / 4097: the
# last size one workgroup handles in one launch and the first that goes through the partial totals of several
NS = (1, 63, 65, 257, 1025, 4096, 4097)
PAIR_NS = (65, 1025)
PIX_THRESH, DEPTH_THRESH = 10.0, 0.1
# case -> (loss_type, checks on, weights given)
CASES = {"huber": ("huber", False, True), "l1": ("l1", False, True), "mse": ("mse", False, True), "epe": ("epe", False, True),
         "huber_checks": ("huber", True, True), "huber_now": ("huber", False, False)}
PAIR_CASES = ("huber", "huber_checks")
GRAD_BOUND = 2.0 ** -22


def fixture():
    return dict(np.load(FIXTURE))


def thresholds(checks):
    return (PIX_THRESH, DEPTH_THRESH) if checks else (None, None)


def f64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).clone()


def project(pi, di, Ki, Kj, T):
    one = torch.ones_like(di)[:, None]
    x = (torch.cat([pi, one], 1) @ torch.linalg.inv(Ki).T) * di[:, None]
    h = torch.cat([x, one], 1) @ T.T
    X = h[:, :3] / (h[:, 3:] + 1e-6)
    y = X @ Kj.T
    return y[:, :2] / (y[:, 2:] + 1e-6), X[:, 2]


def term(pi, di, Ki, pj, dj, Kj, T, w, loss_type, pix_thresh, depth_thresh):
    """float64 tensors -> (loss, valid [n] bool, (perc_val_pix_rep, perc_val_depth_rep), (pixel error [n], depth ratio [n]))"""
    n = di.shape[0]
    uv, z = project(pi, di, Ki, Kj, T)
    e = uv - pj
    r = (e * e).sum(-1).sqrt()
    ratio = ((dj - z).abs() / (dj + 1e-6)).detach() if dj is not None else None
    valid = torch.ones(n, dtype=torch.bool)
    pix = dep = torch.zeros((), dtype=torch.float64)
    if pix_thresh is not None:
        vp = r.detach() <= pix_thresh
        valid, pix = valid & vp, vp.sum().double() / (n + 1e-6)
    if depth_thresh is not None:
        vd = ratio <= depth_thresh
        valid, dep = valid & vd, vd.sum().double() / (n + 1e-6)
    a = e.abs()
    if loss_type == "huber":
        l = torch.where(a <= 1.0, 0.5 * e * e, a - 0.5).sum(-1)
    elif loss_type == "l1":
        l = a.sum(-1)
    elif loss_type == "mse":
        l = (e * e).sum(-1)
    elif loss_type == "epe":
        l = r
    else:
        raise ValueError(loss_type)
    if w is not None:
        l = l * w
    m = valid.double()
    return (l * m).sum() / (m.sum() + 1e-6), valid, (pix, dep), (r.detach(), ratio)


def rigid_inverse(P):
    Rt = P[:3, :3].T
    return torch.cat([torch.cat([Rt, -Rt @ P[:3, 3:]], 1), torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=P.dtype)], 0)


def pair(ps, po, ds, do, fs, fo, Ks, Ko, Ps, Po, w, loss_type, pix_thresh, depth_thresh):
    """float64 tensors, poses [4,4] -> (loss, (pix, depth, depth_in_corr_loss), [per term: (valid, (pixel error, depth ratio))])"""
    T = Po @ rigid_inverse(Ps)
    Ti = rigid_inverse(T)
    loss, terms = 0.0, []
    for a, b in ((ds, do),) + (((fs, fo),) if fs is not None else ()):
        for args in ((ps, a, Ks, po, b, Ko, T), (po, b, Ko, ps, a, Ks, Ti)):
            l, valid, (pix, dep), margins = term(*args, w, loss_type, pix_thresh, depth_thresh)
            loss = loss + l
            terms.append((valid, margins))
    return loss / len(terms), (pix, dep, ds.detach().mean()), terms


def term_case(fx, n, case):
    """-> (inputs as float32 numpy dict, keyword options) of one single-term fixture case"""
    loss_type, checks, weights = CASES[case]
    k = f"t{n}_"
    inp = {s: fx[k + s] for s in ("pi", "di", "pj", "dj", "w", "Ki", "Kj", "T")}
    if not weights:
        inp["w"] = None
    pt, dt = thresholds(checks)
    return inp, dict(loss_type=loss_type, pixel_thresh=pt, depth_thresh=dt)


def pair_case(fx, n, fine, case):
    loss_type, checks, _ = CASES[case]
    k = f"p{n}_"
    inp = {s: fx[k + s] for s in ("ps", "po", "ds", "do", "fs", "fo", "w", "Ks", "Ko", "Ps", "Po")}
    if not fine:
        inp["fs"] = inp["fo"] = None
    pt, dt = thresholds(checks)
    return inp, dict(loss_type=loss_type, pixel_thresh=pt, depth_thresh=dt)


def term_want(inp, opts):
    """the float64 values of a single-term case: dict(loss, d_di, d_T, valid, stats)"""
    t = {k: f64(v) if v is not None else None for k, v in inp.items()}
    di, T = t["di"].requires_grad_(), t["T"].requires_grad_()
    loss, valid, (pix, dep), _ = term(t["pi"], di, t["Ki"], t["pj"], t["dj"], t["Kj"], T, t["w"], opts["loss_type"], opts["pixel_thresh"],
                                      opts["depth_thresh"])
    g_di, g_T = torch.autograd.grad(loss, (di, T))
    return dict(loss=loss.item(), d_di=g_di.numpy(), d_T=g_T.numpy(), valid=valid.numpy(), stats=np.array([pix.item(), dep.item()]))


def pair_want(inp, opts):
    """the float64 values of a pair case: dict(loss, d_ds, d_do, d_fs, d_fo, d_Ps, d_Po [3,4], stats)"""
    t = {k: f64(v) if v is not None else None for k, v in inp.items()}
    leaves = {k: t[k].requires_grad_() for k in ("ds", "do", "fs", "fo", "Ps", "Po") if t[k] is not None}
    loss, stats, _ = pair(t["ps"], t["po"], t["ds"], t["do"], t["fs"], t["fo"], t["Ks"], t["Ko"], t["Ps"], t["Po"], t["w"], opts["loss_type"],
                          opts["pixel_thresh"], opts["depth_thresh"])
    gs = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
    out = dict(loss=loss.item(), stats=np.array([float(s) for s in stats]))
    for k, g in gs.items():
        out["d_" + k] = g.numpy()[:3] if k in ("Ps", "Po") else g.numpy()
    return out


def to_np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def fwd_excess(got, want64):
    """max over elements of |got - want| / spacing(fp32(|want|)): <= 1 passes"""
    got, want64 = to_np(got).astype(np.float64), np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape, (got.shape, want64.shape)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want64) / np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)))


def fwd_abs(got, want64):
    got = to_np(got).astype(np.float64)
    return float(np.max(np.abs(got - want64))) if got.size else 0.0


def rel_l2(got, want64):
    got, want64 = to_np(got).astype(np.float64), np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape, (got.shape, want64.shape)
    den = float(np.sqrt((want64 ** 2).sum()))
    num = float(np.sqrt(((got - want64) ** 2).sum()))
    return num / den if den > 0 else num
