"""What `Graph.render_batch` launches, decided before anything is launched: no kernels, no allocation, no device queries.

The requests of one call fall into at most two grad-mode BLOCKS, issued grad first, then no_grad.  A block's requests share one ray
buffer: `render` requests first, `render_to_max` requests after them, so that each kind is one contiguous row range.  Inside a
block the order is: the coarse passes, one resampling call per `render` request that has rays (in row order), the fine passes of the
`render` requests on the merged coarse-and-fine depths, the fine passes of the `render_to_max` requests on the coarse depths
(renderer.py:583-592; skipped under `tomax_skip`).  That order is also the order of the random draws, hence part of the bit-for-bit
contract with the separate calls.  The merged depth buffer holds the `render` rows only, and those start the block: both depth
buffers are addressed by the block's row numbers."""
from dataclasses import dataclass, field

from .lib import SparfError


@dataclass(eq=False)
class Member:
    """one request of a render_batch call.  B, R, to_max, nograd, mode are what the planner reads, `off` (first row in its block's ray
    buffer) what it writes, n = B * R its rays; q (the request), draws (its `_draws`, or {}) and pred (its result) are the issuer's"""
    B: int
    R: int
    to_max: bool
    nograd: bool
    mode: str
    q: dict = None
    draws: dict = field(default_factory=dict)
    off: int = 0
    pred: dict = None

    def __post_init__(self):
        self.n = self.B * self.R


@dataclass
class Pass:
    """one launch set: network `fine` (else coarse) over rows [lo, hi) of the block, N samples each, read from the merged depth buffer
    (else the coarse one); segs: [(ray0 - lo, nrays, noise_scale)] of `members`"""
    fine: bool
    N: int
    prec: int
    far: tuple
    lo: int
    hi: int
    merged: bool
    segs: list
    members: list

    @property
    def suffix(self):
        return "_fine" if self.fine else ""

    @property
    def noisy(self):
        return any(s[2] > 0 for s in self.segs)


@dataclass
class Block:
    """the requests of one grad mode in row order, and what runs over them, in issue order: coarse, resample, fine.  merged_rows: rows of
    the merged depth buffer, None if there is none"""
    nograd: bool
    members: list
    rows: int
    coarse: list
    resample: list
    merged_rows: int
    fine: list


def _same_route(a, b):
    """whether a `render` pass at a = (prec, far) and a `render_to_max` pass at b may be one pass.  far = (K, prec) routes the last K
    samples of every ray, (depth, prec) the tiles beyond a depth: never the same route, though 8 == 8.0 (the defaults of both)"""
    return a == b and (a[1] is None or type(a[1][0]) is type(b[1][0]))


def _passes(group, fine, N, merged, reg, max_segments, prec_of, cap_rows):
    """the passes of one network over `group` (consecutive members of a block): by kind where the precisions of the two kinds differ,
    then cut greedily where a pass would hold more than `max_segments` requests or more sample rows than one launch set takes"""
    kinds = sorted({m.to_max for m in group})
    precs = {k: prec_of(k, N) for k in kinds}
    if len(kinds) == 2 and not _same_route(precs[False], precs[True]):
        return [p for k in kinds for p in _passes([m for m in group if m.to_max == k], fine, N, merged, reg, max_segments, prec_of, cap_rows)]
    out = []
    if group:
        prec, far = precs[group[0].to_max]
        cap = cap_rows(prec, sum(m.n for m in group) * N) // N
        part, rows = [], 0
        for m in group + [None]:
            if m is not None and m.n > cap:
                raise SparfError(f"render_batch: one request of {m.n} rays x {N} samples exceeds a launch set; render it with render()")
            if part and (m is None or len(part) == max_segments or rows + m.n > cap):
                lo = part[0].off
                segs = [(x.off - lo, x.n, reg if (x.mode == "train" and reg > 0) else 0.0) for x in part]
                out.append(Pass(fine, N, prec, far, lo, lo + rows, merged, segs, part))
                part, rows = [], 0
            if m is not None:
                part.append(m)
                rows += m.n
    return out


def plan(members, Nc, Nf, fine_on, tomax_skip, reg, max_segments, prec_of, cap_rows, under):
    """-> [Block], in issue order.  members: the requests in the caller's order (their `off` is set here).  prec_of(to_max, N) ->
    (prec, far) of a pass of N samples over requests of one kind; cap_rows(prec, need_rows) -> the sample rows one launch set takes;
    under(nograd): the context in which the two are asked about a block (its grad mode: this module does not look at it)."""
    blocks = []
    for nograd in (False, True):
        mem = sorted((m for m in members if m.nograd == nograd), key=lambda m: m.to_max)
        if not mem:
            continue
        rows = 0
        for m in mem:
            m.off = rows
            rows += m.n
        rend, tomx = [m for m in mem if not m.to_max], [m for m in mem if m.to_max]
        with under(nograd):
            args = (reg, max_segments, prec_of, cap_rows)
            blk = Block(nograd, mem, rows, _passes(mem, False, Nc, False, *args), [], None, [])
            if fine_on:
                if rend:
                    blk.resample, blk.merged_rows = [m for m in rend if m.n > 0], sum(m.n for m in rend)
                blk.fine = _passes(rend, True, Nc + Nf, True, *args) + ([] if tomax_skip else _passes(tomx, True, Nc, False, *args))
        blocks.append(blk)
    return blocks
