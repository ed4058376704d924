"""Referee of the correspondence sampler: the case list -- shapes, mask patterns, windows, correspondence values --
and a numpy restatement of base_corres_loss.py:260-269, :323-328, :365-369 and corres_loss.py:139-155 that shares no code with
sparf_amd.  Integer and copy work: every comparison against it is bit for bit, there is no bound to state.

Shapes: the smallest at which each path of the compaction can go wrong (a tile is 256 pixels, one workgroup does up to 4096):
  7 x 9      less than one wave; a partial tile
  16 x 16    exactly one tile
  63 x 65, 64 x 64   4095 and 4096 pixels: the last one-workgroup sizes
  64 x 65    4160 pixels: the first two-launch size, a second chunk of 64 pixels
  96 x 128   12 288 pixels: three full chunks, a base summed over two predecessors
The fixture (tests/golden/matches.npz, written by tests/golden/make_matches_golden.py) holds what the reference's own
compute_loss_pairwise chain did on the cases of FIXTURE_CASES."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "matches.npz")

TILE, CHUNK = 256, 4096
SHAPES = [(7, 9), (16, 16), (63, 65), (64, 64), (64, 65), (96, 128)]
PATTERNS = ("none", "all", "last", "second_chunk", "seams", "alternate", "bernoulli")
WINDOWS = ("whole", "precrop", "one_row", "empty")
PRECROP_FRAC = 0.5
MAX_MATCHES = 50                 # rand_rays // 2 of the cases: below the count of most patterns, above that of `last` and `seams`


def fixture():
    return dict(np.load(FIXTURE))


def mask_of(H, W, pattern):
    """bool [H, W]"""
    n = H * W
    m = np.zeros(n, dtype=bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "last":
        m[-1] = True
    elif pattern == "second_chunk":                      # nothing below 4096: every earlier workgroup counts 0 (none at all up to 4096 pixels)
        m[CHUNK:2 * CHUNK] = True
    elif pattern == "seams":                             # the last lane of a wave and the first of the next; the same for a tile
        for p in (63, 64, TILE - 1, TILE):
            if p < n:
                m[p] = True
    elif pattern == "alternate":
        m[::2] = True
    elif pattern == "bernoulli":
        m = np.random.RandomState(7 * H + W).random_sample(n) < 0.3
    elif pattern != "none":
        raise ValueError(pattern)
    return m.reshape(H, W)


def precrop_window(H, W, frac=PRECROP_FRAC):
    """base_corres_loss.py:264-268, with its - 1"""
    dH, dW = int(H // 2 * frac), int(W // 2 * frac)
    return (H // 2 - dH, H // 2 + dH - 1, W // 2 - dW, W // 2 + dW - 1)


def window_of(H, W, name):
    """(y0, y1, x0, x1) as Python slice bounds, or None"""
    if name == "whole":
        return None
    if name == "precrop":
        return precrop_window(H, W)
    if name == "one_row":
        return (H // 2, H // 2 + 1, 0, W)
    if name == "empty":                                  # dH = 0: the slice H//2 : H//2 - 1
        return precrop_window(H, W, 0.0)[:2] + precrop_window(H, W)[2:]
    raise ValueError(name)


def maps_of(H, W):
    """corres [2, H, W] and conf [1, H, W], float32: correspondences inside the other image, with exact .5 ties (both parities), W - 1
    and H - 1 exactly and -0.0 at pixels that the patterns select (the first ones, the seams, the last one)"""
    rs = np.random.RandomState(1000 * H + W)
    n = H * W
    x = rs.uniform(0, W - 1, n).astype(np.float32)
    y = rs.uniform(0, H - 1, n).astype(np.float32)
    ties = np.floor(rs.uniform(0, min(H, W) - 1, n)).astype(np.float32) + np.float32(0.5)
    tie_at = rs.random_sample(n) < 0.2                   # a fifth of the pixels: x.5, rounded to the even neighbour
    x[tie_at] = ties[tie_at]
    tie_at = rs.random_sample(n) < 0.2
    y[tie_at] = ties[tie_at]
    special = {0: (0.5, 1.5), 1: (2.5, -0.0), 2: (W - 1.0, H - 1.0), 3: (1.5, 0.5), 4: (-0.0, 2.5), 63: (0.5, 0.5), 64: (1.5, 1.5),
               TILE - 1: (2.5, 3.5), TILE: (W - 1.0, 0.5), n - 1: (W - 1.0, H - 1.0), n - 2: (W - 1.5, H - 1.5)}
    for p, (cx, cy) in special.items():
        if 0 <= p < n:
            x[p], y[p] = cx, cy
    conf = rs.uniform(0.5, 1.0, n).astype(np.float32)
    return np.stack([x, y]).reshape(2, H, W), conf.reshape(1, H, W)


def window_mask(mask, window):
    if window is None:
        return mask
    centre = np.zeros_like(mask)
    centre[window[0]:window[1], window[2]:window[3]] = True
    return mask & centre


def select_np(mask, corres, conf, max_matches, window=None, perm=None):
    """mask bool [H,W], corres [2,H,W], conf [1,H,W]; perm: a permutation of range(count), needed when count > max_matches.
    -> dict(pixels_self [k,2] f32, ray_self [k] i64, pixels_other [k,2] f32, ray_other [k] i64, conf [k,1] f32, count, perc f32,
    index [count] i32)"""
    H, W = mask.shape
    index = np.flatnonzero(window_mask(mask, window).reshape(-1))
    count = len(index)
    rows = index
    if count > max_matches:
        rows = index[np.asarray(perm)[:max_matches]]
    cx, cy = corres[0].reshape(-1)[rows], corres[1].reshape(-1)[rows]
    return dict(pixels_self=np.stack([rows % W, rows // W], 1).astype(np.float32), ray_self=rows.astype(np.int64),
                pixels_other=np.stack([cx, cy], 1).astype(np.float32),
                ray_other=np.rint(cy).astype(np.int64) * W + np.rint(cx).astype(np.int64),          # np.rint: half to even
                conf=conf.reshape(-1)[rows].astype(np.float32)[:, None], count=count,
                perc=np.float32(count) / np.float32(H * W + 1e-6), index=index.astype(np.int32))


def perm_of(count, seed=0):
    return np.random.RandomState(seed + count).permutation(count).astype(np.int64)


# ---- what make_matches_golden.py runs the reference on: name -> (H, W, source of the maps, precrop phase, min_nbr_matches)
# `sphere`: the maps of tests/ref_harness.SphereFlowNet through the reference's own compute_correspondences; a pattern: mask_of / maps_of
# (the maps of a pattern case are not stored: maps_of() makes them again, the file stays small)
FIXTURE_CASES = {}
for _H, _W in SHAPES:
    if (_H, _W) in ((16, 16), (64, 65)):
        FIXTURE_CASES[f"sphere_{_H}x{_W}"] = (_H, _W, "sphere", False, 1)
        FIXTURE_CASES[f"sphere_precrop_{_H}x{_W}"] = (_H, _W, "sphere", True, 1)
    FIXTURE_CASES[f"bernoulli_precrop_{_H}x{_W}"] = (_H, _W, "bernoulli", True, 1)
    FIXTURE_CASES[f"all_{_H}x{_W}"] = (_H, _W, "all", False, 1)
    FIXTURE_CASES[f"alternate_precrop_{_H}x{_W}"] = (_H, _W, "alternate", True, 1)
FIXTURE_CASES["seams_64x65"] = (64, 65, "seams", False, 1)
FIXTURE_CASES["second_chunk_96x128"] = (96, 128, "second_chunk", False, 1)
FIXTURE_CASES["too_few_16x16"] = (16, 16, "seams", False, 500)          # below min_nbr_matches: the dictionaries come back untouched
FIXTURE_KEYS = ("mask", "corres", "conf", "window", "perm", "pixels_self", "pixels_other", "ray_self", "ray_other", "conf_values", "perc", "rendered")


def fixture_case(fx, name):
    """the arrays of one fixture case by FIXTURE_KEYS; window None when the case has none, perm None when nothing was drawn"""
    H, W, source = FIXTURE_CASES[name][:3]
    case = {k: fx[f"{name}/{k}"] for k in FIXTURE_KEYS if f"{name}/{k}" in fx}
    if source != "sphere":
        case["corres"], case["conf"] = maps_of(H, W)
    case["window"] = tuple(int(v) for v in case["window"]) if len(case["window"]) else None
    case["perm"] = case["perm"] if len(case["perm"]) else None
    return case
