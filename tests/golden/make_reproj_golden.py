"""Generate tests/golden/reproj.npz: inputs and the REFERENCE's own fp32 results (CPU) for the correspondence loss
(tests/test_reproj_cpu.py, tests/test_reproj_gpu.py; names, sizes and cases: tests/reproj_referee.py).

Runs only where the reference is importable (through tests/ref_harness.install_reference()): the committed file holds arrays only.
The single-term results come from the reference's unmodified compute_render_and_repro_loss_w_repro_thres, called unbound on a stand-in
whose compute_diff_loss is BaseLoss.compute_diff_loss; the pair results from the same method in the call order of corres_loss.py:183-219
with the reference's pose_inverse_4x4.

Scene: a 378x504 image, fx = fy = 500 (the other view of a PAIR has a general K: unequal focal lengths, a skew, a shifted principal
point); a relative pose of about 0.2 rad and 0.4 units; depths in [1.5, 5]; target pixels = the exact projection plus noise of sigma
0.3 px for half of the matches and 6 px for the rest (both Huber branches, ~12 % beyond the 10 px check); depth_j = the projected depth
x (1 + 0.08 N(0,1)) (~22 % fail the 0.1 check); fine depths = the coarse ones x (1 + 0.02 N(0,1)).

Margins are a CONDITION: a match whose float64 pixel error lies within 0.01 px of the pixel threshold or whose depth ratio lies within
1e-4 of its threshold -- in any term that uses it -- is redrawn, and the reference's fp32 mask must equal the float64 one on every case.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "compat")]

from tests import ref_harness                                           # noqa: E402
from tests import reproj_referee as R                                   # noqa: E402

assert ref_harness.install_reference(), "the reference tree is not importable"
from easydict import EasyDict as edict                                  # noqa: E402
from source.training.core.base_losses import BaseLoss                   # noqa: E402
from source.training.core.corres_loss import CorrespondencesPairRenderDepthAndGet3DPtsAndReproject as Corres   # noqa: E402
from source.utils.camera import pose_inverse_4x4                        # noqa: E402

H, W = 378, 504
K_PINHOLE = np.array([[500.0, 0, W / 2], [0, 500.0, H / 2], [0, 0, 1]])
K_GENERAL = np.array([[510.0, 0.5, W / 2 + 3.0], [0, 495.0, H / 2 - 2.0], [0, 0, 1]])
PIX_MARGIN, DEPTH_MARGIN = 0.01, 1e-4
METHOD = Corres.compute_render_and_repro_loss_w_repro_thres
STAND_IN = types.SimpleNamespace(compute_diff_loss=lambda **k: BaseLoss.compute_diff_loss(None, **k))


def rot(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def rigid4(w, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(w), t
    return T


T_REL = rigid4([0.05, -0.2, 0.03], [0.4, -0.05, 0.1])
P_SELF = rigid4([0.1, 0.05, -0.07], [0.1, -0.2, 0.3])


def draw(rs, n, Ki, Kj, T):
    """n candidate matches in float64: integer pixels in i, depth, noisy projection in j, noisy projected depth, fine depths, weight"""
    pi = np.stack([rs.randint(0, W, n), rs.randint(0, H, n)], 1).astype(np.float64)
    di = rs.uniform(1.5, 5.0, n)
    X = (np.linalg.inv(Ki) @ np.c_[pi, np.ones(n)].T).T * di[:, None]
    Xj = X @ T[:3, :3].T + T[:3, 3]
    y = Xj @ Kj.T
    pj = y[:, :2] / y[:, 2:] + rs.standard_normal((n, 2)) * np.where(rs.rand(n, 1) < 0.5, 0.3, 6.0)
    dj = Xj[:, 2] * (1 + 0.08 * rs.standard_normal(n))
    fi, fj = di * (1 + 0.02 * rs.standard_normal(n)), dj * (1 + 0.02 * rs.standard_normal(n))
    return [a.astype(np.float32) for a in (pi, di, pj, dj, fi, fj, rs.uniform(0.5, 1.0, n))]


def near_threshold(margins):
    r, ratio = (m.numpy() for m in margins)
    return (np.abs(r - R.PIX_THRESH) < PIX_MARGIN) | (np.abs(ratio - R.DEPTH_THRESH) < DEPTH_MARGIN)


def scene(rs, n, Ki, Kj, T, bad_rows):
    """draw n matches, redraw the rows bad_rows(arrays) flags until it flags none"""
    arrs = draw(rs, n, Ki, Kj, T)
    for _ in range(100):
        bad = bad_rows(arrs)
        if not bad.any():
            return arrs
        new = draw(rs, int(bad.sum()), Ki, Kj, T)
        for a, b in zip(arrs, new):
            a[bad] = b
    raise RuntimeError("margins not met")


def f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


def opt_of(opts):
    return edict(diff_loss_type=opts["loss_type"], renderrepro_do_pixel_reprojection_check=opts["pixel_thresh"] is not None,
                 renderrepro_do_depth_reprojection_check=opts["depth_thresh"] is not None,
                 renderrepro_pixel_reprojection_thresh=R.PIX_THRESH, renderrepro_depth_reprojection_thresh=R.DEPTH_THRESH)


def stat(stats, key):
    return float(stats[key]) if key in stats else 0.0


def main():
    rs = np.random.RandomState(20261)
    out = {}
    for n in R.NS:
        Ki = Kj = K_PINHOLE.astype(np.float32)
        T = T_REL.astype(np.float32)

        def bad_rows(a):
            return near_threshold(R.term(R.f64(a[0]), R.f64(a[1]), R.f64(Ki), R.f64(a[2]), R.f64(a[3]), R.f64(Kj), R.f64(T), None, "huber",
                                         R.PIX_THRESH, R.DEPTH_THRESH)[3])
        pi, di, pj, dj, _, _, w = scene(rs, n, K_PINHOLE, K_PINHOLE, T_REL, bad_rows)
        k = f"t{n}_"
        out.update({k + "pi": pi, k + "di": di, k + "pj": pj, k + "dj": dj, k + "w": w, k + "Ki": Ki, k + "Kj": Kj, k + "T": T})
        for case in R.CASES:
            inp, opts = R.term_case(out, n, case)
            d, Tt = f32(di).requires_grad_(), f32(T).requires_grad_()
            conf = f32(inp["w"])[:, None] if inp["w"] is not None else None
            loss, stats, valid = METHOD(STAND_IN, opt_of(opts), f32(pi).long(), d, f32(Ki), f32(pj), f32(dj), f32(Kj), Tt, conf, {},
                                        return_valid_mask=True)
            g_d, g_T = torch.autograd.grad(loss, (d, Tt))
            want = R.term_want(inp, opts)
            assert np.array_equal(valid.numpy()[:, 0], want["valid"]), (n, case)
            c = k + case + "_"
            out.update({c + "loss": loss.detach().numpy(), c + "d_di": g_d.numpy(), c + "d_T": g_T.numpy(), c + "valid": valid.numpy()[:, 0],
                        c + "stats": np.array([stat(stats, "perc_val_pix_rep"), stat(stats, "perc_val_depth_rep")], dtype=np.float32)})
    for n in R.PAIR_NS:
        Ks, Ko = K_PINHOLE.astype(np.float32), K_GENERAL.astype(np.float32)
        Ps, Po = P_SELF.astype(np.float32), (T_REL @ P_SELF).astype(np.float32)
        T64 = Po.astype(np.float64) @ np.linalg.inv(Ps.astype(np.float64))

        def bad_rows(a):
            ps, ds, po, do, fs, fo = (R.f64(x) for x in a[:6])
            terms = R.pair(ps, po, ds, do, fs, fo, R.f64(Ks), R.f64(Ko), R.f64(Ps), R.f64(Po), None, "huber", R.PIX_THRESH, R.DEPTH_THRESH)[2]
            return np.any([near_threshold(m) for _, m in terms], axis=0)
        ps, ds, po, do, fs, fo, w = scene(rs, n, K_PINHOLE, K_GENERAL, T64, bad_rows)
        k = f"p{n}_"
        out.update({k + "ps": ps, k + "po": po, k + "ds": ds, k + "do": do, k + "fs": fs, k + "fo": fo, k + "w": w, k + "Ks": Ks, k + "Ko": Ko,
                    k + "Ps": Ps, k + "Po": Po})
        for fine in (0, 1):
            for case in R.PAIR_CASES:
                inp, opts = R.pair_case(out, n, fine, case)
                opt = opt_of(opts)
                t = {s: f32(inp[s]).requires_grad_() for s in ("ds", "do", "fs", "fo", "Ps", "Po") if inp[s] is not None}
                conf, pxs, pxo = f32(w)[:, None], f32(ps).long(), f32(po)
                # corres_loss.py:183-219
                stats = {"depth_in_corr_loss": t["ds"].detach().mean()}
                T_s2o = t["Po"] @ pose_inverse_4x4(t["Ps"])
                valids = []
                loss = 0
                for a, b in (("ds", "do"),) + ((("fs", "fo"),) if fine else ()):
                    l, stats, v = METHOD(STAND_IN, opt, pxs, t[a], f32(Ks), pxo, t[b], f32(Ko), T_s2o, conf, stats, return_valid_mask=True)
                    loss = loss + l
                    valids.append(v)
                    l, stats, v = METHOD(STAND_IN, opt, pxo, t[b], f32(Ko), pxs, t[a], f32(Ks), pose_inverse_4x4(T_s2o), conf, stats,
                                         return_valid_mask=True)
                    loss = loss + l
                    valids.append(v)
                loss = loss / 4. if fine else loss / 2.
                gs = dict(zip(t, torch.autograd.grad(loss, list(t.values()))))
                t64 = {s: R.f64(v) if v is not None else None for s, v in inp.items()}
                terms = R.pair(t64["ps"], t64["po"], t64["ds"], t64["do"], t64["fs"], t64["fo"], t64["Ks"], t64["Ko"], t64["Ps"], t64["Po"], None,
                               opts["loss_type"], opts["pixel_thresh"], opts["depth_thresh"])[2]
                for v32, (v64, _) in zip(valids, terms):
                    assert np.array_equal(v32.numpy()[:, 0], v64.numpy()), (n, fine, case)
                c = f"{k}f{fine}_{case}_"
                out[c + "loss"] = loss.detach().numpy()
                out[c + "stats"] = np.array([stat(stats, "perc_val_pix_rep"), stat(stats, "perc_val_depth_rep"), stat(stats, "depth_in_corr_loss")],
                                            dtype=np.float32)
                for s, g in gs.items():
                    out[c + "d_" + s] = g.numpy()
    for key, v in out.items():
        assert (v.dtype == np.float32 or v.dtype == np.bool_) and np.isfinite(v).all(), key
    np.savez_compressed(R.FIXTURE, **out)
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes,", len(out), "arrays")
    k = "t257_huber_checks_"
    print("n = 257 with both checks: valid share", out[k + "valid"].mean(), "stats", out[k + "stats"])


if __name__ == "__main__":
    main()
