"""Float64 referee of the evaluation-metrics kernel (tests/test_metrics_cpu.py, tests/test_metrics_gpu.py,
tests/golden/make_metrics_golden.py): the formulas as include/sparf_hip.h states them, in float64 numpy on the fp32 operands cast to
double.  SSIM is a DIRECT 2-D convolution with the reference's stored fp32 11 x 11 window (the fixture's `window`), zero padding of 5,
written as 121 shifted sums (no BLAS call: the same bits on every machine) -- not the separable passes of csrc/metrics.hip, so the
kernel's window is checked against a derivation it does not share.

Bound (the issue's): every finite output within ONE fp32 spacing of the float64 value -- double arithmetic on the fp32 operands and the
separable window cost less than 0.01 spacing of a mean, the rounding of the stored value 0.5 --; NaN / inf in the same places; the two
counts exact.  The torch restatement (sparf_amd.metrics.image_metrics_torch) runs in fp32 like the reference and is held to 4x the
reference's own distance from this referee on the same case.

Fixture (tests/golden/metrics.npz, arrays only):
  window [11,11] float32        create_window(11, 1)[0, 0] of the reference;  window_1d [11] its gaussian(11, 1.5)
  pool_check                    a few values of the pools below, so that a test sees a generator that drifted
  ref_<case> [heads,10] float32 the REFERENCE's own values on the CPU in the order of OUTS, from its unmodified MSE_loss, ssim,
                                compute_metrics and compute_metrics_masked (NaN for what the case does not ask for)
  dict_<case> [heads,8] float32 what its compute_metrics returned with the case's scale, in the order of DICT_KEYS (the stub LPIPS gives 0.25)
  refdist_<case> [heads,10]     the reference's own distance from this referee in fp32 spacings of the referee's value (NaN where not finite)
The inputs are NOT stored: pools() draws them from np.random.RandomState(SEED) at the largest shape; a case uses the top-left corner.
"""
import functools
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")
SEED = 20270
TH, TW = 16, 32                  # csrc/metrics.h METRICS_TH, METRICS_TW
K, R = 11, 5
OUTS = ("mse", "psnr", "ssim", "mse_masked", "psnr_masked", "ssim_masked", "abs_e", "rmse", "abs_e_scaled", "rmse_scaled")
DICT_KEYS = ("psnr", "ssim", "lpips", "abse_depth", "rmse_depth", "psnr_masked", "ssim_masked", "lpips_masked")
LPIPS = 0.25
BOUND = 1.0                      # fp32 spacings of the referee's value
PB, PH, PW = 2, 96, 128          # the pools' shape
SCALE = 1.37
# the smallest shapes at which the kernel can go wrong: one pixel; smaller than the window; the window; just off it; the tile; a tile
# short of a row and one column over; one row over and two tiles plus a column; a halo that crosses two tiles both ways
SHAPES = ((1, 1), (5, 7), (11, 11), (10, 12), (TH, TW), (TH - 1, TW + 1), (TH + 1, 2 * TW + 1), (2 * TH + 5, TW + 6))
CONTENTS = ("random", "noise", "const", "identical")
MASKS = ("blob", "all", "none", "one", None)
DEPTHS = ("some", "none", None)


def _cases():
    C = {}

    def add(name, H, W, **kw):
        C[name] = dict(dict(B=1, H=H, W=W, content="random", mask="blob", depth="some", scale=SCALE, fine=True), **kw)
    for H, W in SHAPES:
        add(f"s{H}x{W}", H, W)
        add(f"s{H}x{W}_noise_one_head", H, W, content="noise", fine=False, scale=1.0)
    add("big", 96, 128, B=2)
    add("big_noise", 96, 128, B=2, content="noise", mask="all", scale=1.0)
    # contents, masks and depths on a shape below the window, on one with a column of its own in a third tile, and on the crossing halo
    for H, W in ((5, 7), (TH + 1, 2 * TW + 1), (2 * TH + 5, TW + 6)):
        add(f"const{H}x{W}", H, W, content="const")
        add(f"identical{H}x{W}", H, W, content="identical", mask="all")
        add(f"none{H}x{W}", H, W, content="noise", mask="none", depth="none")
        add(f"one{H}x{W}", H, W, mask="one", depth="none", scale=1.0, fine=False)
        add(f"plain{H}x{W}", H, W, mask=None, depth=None)
        add(f"depth_only{H}x{W}", H, W, content="noise", mask=None, scale=1.0)
        add(f"mask_only{H}x{W}", H, W, content="const", depth=None, fine=False)
    return C


CASES = _cases()


def fixture():
    return dict(np.load(FIXTURE))


# ---- the inputs
@functools.lru_cache(maxsize=1)
def pools():
    rs = np.random.RandomState(SEED)
    u = lambda *s: rs.random_sample(s).astype(np.float32)
    p = dict(gt=u(PB, 3, PH, PW), pred=u(PB, 3, PH, PW), fine=u(PB, 3, PH, PW),
             noise=rs.standard_normal((2, PB, 3, PH, PW)).astype(np.float32),
             depth_gt=(0.5 + 3.5 * u(PB, PH, PW)), depth_noise=rs.standard_normal((2, PB, PH, PW)).astype(np.float32), valid=u(PB, PH, PW) < 0.6)
    return p


def pool_check():
    p = pools()
    return np.concatenate([p[k].reshape(-1)[::40009].astype(np.float32) for k in ("gt", "pred", "fine", "noise", "depth_gt", "depth_noise", "valid")])


def blob(B, H, W):
    """an ellipse about the centre: 30-50 % of the pixels once the image is 10 x 12 or larger; one pixel's own decision below"""
    yy, xx = np.mgrid[0:H, 0:W]
    e = ((yy - (H - 1) / 2) / (0.35 * H + 0.2)) ** 2 + ((xx - (W - 1) / 2) / (0.35 * W + 0.2)) ** 2 < 1.0
    return np.broadcast_to(e, (B, H, W)).copy()


def inputs(name):
    """-> dict: pred, fine (None: one head), gt [B,3,H,W] float32; mask [B,H,W] bool or None; depth, depth_fine, depth_gt [B,H W] float32
    and valid [B,H W] bool, or None; scale"""
    c, p = CASES[name], pools()
    B, H, W = c["B"], c["H"], c["W"]
    cut = lambda a: np.ascontiguousarray(a[..., :B, :, :H, :W])              # images [.., B, 3, H, W]
    cut_px = lambda a: np.ascontiguousarray(a[..., :B, :H, :W])              # per-pixel values [.., B, H, W]
    gt, pred, fine = cut(p["gt"]), cut(p["pred"]), cut(p["fine"])
    if c["content"] == "noise":              # ground truth plus clamped noise
        n = cut(p["noise"])
        pred, fine = np.clip(gt + np.float32(0.1) * n[0], 0, 1).astype(np.float32), np.clip(gt + np.float32(0.03) * n[1], 0, 1).astype(np.float32)
    elif c["content"] == "const":            # constant images with one pixel off: sigma ~ 0 everywhere else
        gt = np.full_like(gt, 0.5)
        pred, fine = gt.copy(), gt.copy()
        gt[:, :, H // 2, W // 2] = 0.75
        pred[:, :, (H // 2 + 2) % H, (W // 2 + 3) % W] = 0.25
        fine[:, 1, H // 3, W // 3] = 0.5625
    elif c["content"] == "identical":
        pred, fine = gt.copy(), gt.copy()
    mask = None
    if c["mask"] == "blob":
        mask = blob(B, H, W)
    elif c["mask"] in ("all", "none"):
        mask = np.full((B, H, W), c["mask"] == "all")
    elif c["mask"] == "one":
        mask = np.zeros((B, H, W), dtype=bool)
        mask[:, H // 2, W // 2] = True
    x = dict(B=B, H=H, W=W, pred=pred, fine=fine if c["fine"] else None, gt=gt, mask=mask, depth=None, depth_fine=None, depth_gt=None, valid=None,
             scale=float(np.float32(c["scale"])))
    if c["depth"] is not None:
        dgt, dn = cut_px(p["depth_gt"]).reshape(B, H * W), cut_px(p["depth_noise"]).reshape(2, B, H * W)
        x["depth_gt"] = dgt
        x["depth"] = (dgt / np.float32(1.3) + np.float32(0.2) * dn[0]).astype(np.float32)
        if c["fine"]:
            x["depth_fine"] = (dgt / np.float32(1.4) + np.float32(0.05) * dn[1]).astype(np.float32)
        x["valid"] = cut_px(p["valid"]).reshape(B, H * W) if c["depth"] == "some" else np.zeros((B, H * W), dtype=bool)
    return x


# ---- the referee
def conv(x, window):
    """x [B,3,H,W] float64, window [11,11] (taken to float64) -> the zero-padded correlation, 121 shifted sums in a fixed order"""
    H, W = x.shape[-2:]
    pad = np.zeros(x.shape[:-2] + (H + 2 * R, W + 2 * R))
    pad[..., R:R + H, R:R + W] = x
    w = window.astype(np.float64)
    out = np.zeros_like(x)
    for i in range(K):
        for j in range(K):
            out += w[i, j] * pad[..., i:i + H, j:j + W]
    return out


def ssim_map(img1, img2, window):
    mu1, mu2 = conv(img1, window), conv(img2, window)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sigma1_sq = conv(img1 * img1, window) - mu1_sq
    sigma2_sq = conv(img2 * img2, window) - mu2_sq
    sigma12 = conv(img1 * img2, window) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def want(x, window):
    """-> dict(out [heads,10] float64 in the order of OUTS with NaN for what is off, counts [2])"""
    gt = x["gt"].astype(np.float64)
    heads = [h for h in (("pred", "depth"), ("fine", "depth_fine")) if x[h[0]] is not None]
    out = np.full((len(heads), len(OUTS)), np.nan)
    counts = np.zeros(2, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for h, (pk, dk) in enumerate(heads):
            p = x[pk].astype(np.float64)
            mse = ((p - gt) ** 2).mean()
            out[h, :3] = mse, -10 * np.log10(mse), ssim_map(p, gt, window).mean()
            if x["mask"] is not None:
                m = x["mask"][:, None].astype(np.float64)
                sel = np.broadcast_to(x["mask"][:, None], p.shape)
                p_fg, gt_fg = p * m + (1.0 - m), gt * m + (1.0 - m)
                counts[0] = x["mask"].sum()
                mse_m = np.float64(((p_fg - gt_fg) ** 2)[sel].sum()) / np.float64(sel.sum())
                out[h, 3:6] = mse_m, -10 * np.log10(mse_m), ssim_map(p_fg, gt_fg, window).mean()
            if x[dk] is not None:
                v = x["valid"]
                counts[1] = n = v.sum()
                g, d = x["depth_gt"].astype(np.float64)[v], x[dk].astype(np.float64)[v]
                for j, s in ((6, 1.0), (8, x["scale"])):
                    e = g - s * d
                    out[h, j], out[h, j + 1] = np.abs(e).sum() / (n + 1e-6), np.sqrt(np.float64((e * e).sum()) / np.float64(n))
    if x["depth_gt"] is not None:
        counts[1] = x["valid"].sum()
    return dict(out=out, counts=counts)


def spacings(got, want64):
    """|got - want| in fp32 spacings of the referee's value, elementwise; NaN where the referee's value is not finite"""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    fin = np.isfinite(want64)
    sp = np.spacing(np.abs(np.where(fin, want64, 1.0)).astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(fin, np.abs(got - want64) / sp, np.nan)


def same_pattern(got, want64):
    """NaN and +-inf in the same places"""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    return np.array_equal(np.isnan(got), np.isnan(want64)) and np.array_equal(np.where(np.isinf(got), np.sign(got), 0), np.where(np.isinf(want64), np.sign(want64), 0))
