"""What Graph.render_batch launches, checked without a GPU.

  * the planner (sparf_amd/batch_plan.py) on seeded random request lists: every request in exactly one pass per network, segment
    tables contiguous and within the table size, passes within the row cap and of one precision, `render` before `render_to_max`;
  * Graph.render_batch itself with the ops it calls replaced by fakes (`record_render_batch`): every pass and resampling call it
    issues, in order, with the sums of the noise and of the fine grids it hands over (which depend on the ORDER of the random draws),
    against tests/golden/render_batch_trace.json -- recorded by the same function on the commit BEFORE the planner existed
    (`python -m tests.test_batch_plan_cpu --record` writes the file; it goes through the public render_batch only).
    One of the ten entries is not that commit's own: in `d_kinds_apart_no_grad` it compared the two kinds' (prec, far) as tuples,
    (8, fp32) == (8.0, fp32), and ran the coarse pass of both kinds as ONE pass of 22 rays on the `render` route; the entry was
    recorded from that commit's render_batch with that one comparison mended (the kind of the route compared too), nothing else."""
import contextlib
import json
import math
import os
import random

import pytest
import torch

from sparf_amd import lib as L
from sparf_amd import ops
from sparf_amd import renderer
from sparf_amd.config import default_opt
from tests.golden.recipe import small_opt

TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_batch_trace.json")
H = W = 8
AMPLE = 1 << 20


def _fsum(x):
    """exactly rounded sum: the same on every machine, whatever order a reduction would take"""
    return None if x is None else math.fsum(x.detach().double().flatten().tolist())


@contextlib.contextmanager
def stubbed(cap, events=None):
    """the ops render_batch calls replaced by fakes that launch nothing (zero results of the right shapes) and, with a list given,
    record what they were handed; max_rows_per_call replaced by the fixed `cap`"""
    def fake_pass(center, dirs, t, noise, white_bg, prec, packed, c2f, params, segs, far=None):
        N = t.shape[1]
        if events is not None:
            assert center.shape == (t.shape[0], 3) and dirs.shape == center.shape and (noise is None or noise.shape == t.shape)
            events.append(dict(call="pass", rows=t.shape[0], N=N, prec=prec, far=None if far is None else list(far[:2]),
                               segs=[list(s) for s in segs], grad=torch.is_grad_enabled(), noise=noise is not None, noise_sum=_fsum(noise)))
        z = torch.zeros
        return [dict(zip(ops.PASS_KEYS, (z(n, 3), z(n), z(n), z(n, N), z(n), z(n), z(n), z(n, N), z(n, N, 3)))) for _, n, _ in segs]

    def fake_coarse(nrays, nsamp, dmin, scale, inverse, device, jitter=None, u_const=0.5, dmax_ray=None, range_dev=None, out=None):
        if events is not None:
            events.append(dict(call="coarse", shape=[nrays, nsamp], to_max=dmax_ray is not None, jitter_sum=_fsum(jitter)))
        return out if out is not None else torch.zeros(nrays, nsamp)

    def fake_fine(weights, t_coarse, u_mid, dmin, dmax, want_unsorted=False, range_dev=None, out=None):
        if events is not None:
            assert weights.shape == t_coarse.shape == (out.shape[0], out.shape[1] - u_mid.numel())
            events.append(dict(call="resample", shape=list(out.shape), grid_sum=_fsum(u_mid)))
        return out, None

    def fake_rays(specs, poses):
        return torch.zeros(2, sum(p.shape[0] * ops.ray_request(p.shape[0], s[1], s[2])[1] for s, p in zip(specs, poses)), 3)

    fakes = [(ops, "nerf_pass_segments", fake_pass), (ops, "ray_gen_many", fake_rays), (ops, "sample_coarse", fake_coarse),
             (ops, "sample_fine", fake_fine), (ops, "pack_weights", lambda params, prec, out=None: torch.zeros(1)),
             (ops, "c2f_weights", lambda *a: torch.zeros(16)), (L, "require_gpu", lambda d: None),
             (renderer, "max_rows_per_call", lambda prec=None, device=None, need=None, far=None: cap)]
    saved = [(mod, name, getattr(mod, name)) for mod, name, _ in fakes]
    try:
        for mod, name, fake in fakes:
            setattr(mod, name, fake)
        yield
    finally:
        for mod, name, real in saved:
            setattr(mod, name, real)


def request(n, mode="val", to_max=False, **kw):
    q = dict(pose=torch.eye(3, 4)[None], H=H, W=W, intr=torch.eye(3)[None], ray_idx=torch.arange(n), mode=mode, **kw)
    q.update(dict(depth_min=1.2, depth_max=torch.ones(1, n)) if to_max else dict(depth_range=[1.2, 5.2]))
    return q


def record_render_batch(opt, requests, cap, iter=None, grad=True, with_draws=False, seed=0):
    """-> the calls one Graph.render_batch(opt, requests(), iter) issues, in order, plus whether it drew any random number; a
    SparfError is recorded by its text alone (how far the call got before it is not part of the contract).  with_draws: every
    request carries the `_draws` a deferred call takes when it is issued (Graph._draw_randoms)."""
    events = []
    with stubbed(cap, events), torch.set_grad_enabled(grad):
        torch.manual_seed(seed)
        graph = renderer.Graph(opt, "cpu")
        reqs = requests()
        if with_draws:
            for q in reqs:
                q["_draws"] = graph._draw_randoms(opt, 1, q["ray_idx"].numel(), q["mode"], graph._fine_on(opt, iter))
        before = torch.get_rng_state()
        try:
            preds = graph.render_batch(opt, reqs, iter=iter)
        except L.SparfError as exc:
            return [dict(call="error", text=str(exc))]
        events.append(dict(call="done", drew=not torch.equal(before, torch.get_rng_state()), keys=[sorted(p.keys()) for p in preds]))
    return json.loads(json.dumps(events))


def eighteen():
    reqs = [request(3 + i % 4, mode="train" if i % 3 == 0 else "val") for i in range(18)]
    reqs.insert(7, request(5, to_max=True, no_grad=True))
    return reqs


def both_kinds():
    return [request(5), request(7, to_max=True), request(4), request(6, to_max=True)]


def _inverse_opt():
    return default_opt(nerf=dict(sample_intvs=32, sample_intvs_fine=32, fine_sampling=True, depth=dict(param="inverse")), hip=dict(precision="bf16x3"))


# name -> keyword arguments of record_render_batch (the case table of the planner's issue, a ... j)
CASES = {
    "a_three_renders": lambda: dict(opt=small_opt(), requests=lambda: [request(5), request(3), request(6)], cap=AMPLE),
    "b_cut_by_rows": lambda: dict(opt=small_opt(nerf=dict(density_noise_reg=0.1)), requests=eighteen, cap=20 * 16),
    "c_cut_by_segments": lambda: dict(opt=small_opt(nerf=dict(density_noise_reg=0.1)), requests=eighteen, cap=AMPLE),
    "d_kinds_apart_no_grad": lambda: dict(opt=_inverse_opt(), requests=both_kinds, cap=AMPLE, grad=False),
    "e_kinds_apart_grad": lambda: dict(opt=_inverse_opt(), requests=both_kinds, cap=AMPLE),
    "f_fine_gated_off": lambda: dict(opt=small_opt(max_iter=100, nerf=dict(ratio_start_fine_sampling_at_x=0.5)), requests=both_kinds, cap=AMPLE, iter=10),
    "g_to_max_fine_skipped": lambda: dict(opt=small_opt(nerf=dict(start_fine_sampling_at_x=100)), requests=both_kinds, cap=AMPLE, iter=10),
    "h_deferred_draws": lambda: dict(opt=small_opt(nerf=dict(density_noise_reg=0.1)), requests=lambda: [request(5, mode="train"), request(4, mode="train")],
                                     cap=AMPLE, with_draws=True),
    "i_zero_rays": lambda: dict(opt=small_opt(nerf=dict(density_noise_reg=0.1)),
                                requests=lambda: [request(4, mode="train"), request(0, mode="train"), request(0, to_max=True), request(3)], cap=AMPLE),
    "j_oversized": lambda: dict(opt=small_opt(), requests=lambda: [request(4), request(30), request(2)], cap=20 * 16),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_render_batch_issues_what_the_recorded_trace_says(name):
    with open(TRACE) as f:
        want = json.load(f)[name]
    got = record_render_batch(**CASES[name]())
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, i, g, w)


def test_the_trace_holds_the_situations_it_is_there_for():
    """the recorded cases do show the two cuts, the split by precision, the skipped fine passes and the deferred draws (a trace
    recorded from a case table that missed them would pin nothing)"""
    with open(TRACE) as f:
        tr = json.load(f)
    passes = {k: [e for e in v if e["call"] == "pass"] for k, v in tr.items()}
    grad_b = [p for p in passes["b_cut_by_rows"] if p["grad"]]
    assert all(len(p["segs"]) < 16 for p in grad_b) and len([p for p in grad_b if p["N"] == 16]) > 2
    assert [len(p["segs"]) for p in passes["c_cut_by_segments"] if p["grad"] and p["N"] == 8] == [16, 2]
    assert any(p["noise"] for p in grad_b) and any(not p["noise"] for p in grad_b)
    for k in ("d_kinds_apart_no_grad", "e_kinds_apart_grad"):
        assert len({json.dumps([p["prec"], p["far"]]) for p in passes[k]}) == 2 and [p["rows"] for p in passes[k] if p["N"] == 32] == [9, 13, 13]
    assert {p["N"] for p in passes["f_fine_gated_off"]} == {8} and len(passes["f_fine_gated_off"]) == 1
    assert [(p["rows"], p["N"]) for p in passes["g_to_max_fine_skipped"]] == [(22, 8), (9, 16)]
    assert tr["h_deferred_draws"][-1]["drew"] is False and all(p["noise"] for p in passes["h_deferred_draws"])
    assert tr["b_cut_by_rows"][-1]["drew"] is True
    assert any(s[1] == 0 for p in passes["i_zero_rays"] for s in p["segs"])
    assert tr["j_oversized"][0]["call"] == "error" and "30 rays" in tr["j_oversized"][0]["text"]


# ------------------------------------------------------------------ the planner on its own
def _random_plan(seed, max_segments, split):
    from sparf_amd.batch_plan import Member, plan
    rnd = random.Random(seed)
    Nc, Nf = 8, 8
    members = [Member(B=rnd.choice((1, 1, 2)), R=rnd.randint(0, 25), to_max=rnd.random() < 0.4, nograd=rnd.random() < 0.4,
                      mode=rnd.choice(("train", "val", "test-optim", None))) for _ in range(rnd.randint(1, 40))]
    members = [m for m in members if m.n <= 50]
    fine_on, tomax_skip, reg = rnd.random() < 0.8, rnd.random() < 0.3, rnd.choice((0.0, 0.1))
    cap = rnd.choice((50 * 16, 64 * 16, 200 * 16, AMPLE))          # (50 rays of Nc + Nf samples: the largest request still fits)

    def prec_of(to_max, N):
        return (L.PREC_X3, (8.0 if to_max else 8, L.PREC_FP32)) if split else (L.PREC_FP32, None)

    blocks = plan(members, Nc, Nf, fine_on, tomax_skip, reg, max_segments, prec_of, lambda prec, need: cap, lambda nograd: contextlib.nullcontext())
    return members, blocks, dict(Nc=Nc, Nf=Nf, fine_on=fine_on, tomax_skip=tomax_skip, reg=reg, cap=cap, split=split)


@pytest.mark.parametrize("split", [False, True], ids=["one_precision", "kinds_differ"])
@pytest.mark.parametrize("max_segments", [16, 3])
def test_plan_properties(max_segments, split):
    for seed in range(60):
        members, blocks, c = _random_plan(seed, max_segments, split)
        assert [b.nograd for b in blocks] == sorted({m.nograd for m in members})                     # grad first, then no_grad
        assert sorted(id(m) for b in blocks for m in b.members) == sorted(id(m) for m in members)
        for b in blocks:
            assert all(m.nograd == b.nograd for m in b.members)
            assert [m.to_max for m in b.members] == sorted(m.to_max for m in b.members)              # render requests first
            off = 0
            for m in b.members:                                                                      # row order, back to back
                assert m.off == off
                off += m.n
            assert b.rows == off
            rend = [m for m in b.members if not m.to_max]
            assert b.resample == ([m for m in rend if m.n > 0] if c["fine_on"] else [])
            assert b.merged_rows == (sum(m.n for m in rend) if c["fine_on"] and rend else None)
            assert all(not p.fine and p.N == c["Nc"] and not p.merged for p in b.coarse)
            for net, passes in (("coarse", b.coarse), ("fine", b.fine)):
                count = {}
                for p in passes:
                    assert 1 <= len(p.members) <= max_segments and len(p.segs) == len(p.members)
                    assert p.hi - p.lo <= c["cap"] // p.N
                    assert (p.lo, p.hi) == (p.members[0].off, p.members[-1].off + p.members[-1].n)
                    at = 0
                    for m, (r0, n, scale) in zip(p.members, p.segs):                                 # contiguous, ascending, from 0
                        assert (r0, n) == (at, m.n) and p.lo + r0 == m.off
                        assert scale == (c["reg"] if (m.mode == "train" and c["reg"] > 0) else 0.0)
                        at += n
                        count[id(m)] = count.get(id(m), 0) + 1
                    assert p.noisy == any(s[2] > 0 for s in p.segs)
                    kinds = {m.to_max for m in p.members}
                    if c["split"]:
                        assert len(kinds) == 1 and (p.prec, p.far) == (L.PREC_X3, (8.0 if p.members[0].to_max else 8, L.PREC_FP32))
                    else:
                        assert (p.prec, p.far) == (L.PREC_FP32, None)
                    if net == "fine":
                        assert p.fine and p.suffix == "_fine" and len(kinds) == 1
                        assert (p.N, p.merged) == ((c["Nc"], False) if p.members[0].to_max else (c["Nc"] + c["Nf"], True))
                want = b.members if net == "coarse" else [m for m in b.members if c["fine_on"] and not (m.to_max and c["tomax_skip"])]
                assert count == {id(m): 1 for m in want}                                              # each exactly once, the empty ones too
                if c["split"] or net == "fine":                                                      # render passes precede render_to_max passes
                    order = [p.members[0].to_max for p in passes]
                    assert order == sorted(order)
                assert [p.lo for p in passes] == sorted(p.lo for p in passes)


def test_plan_rejects_a_request_larger_than_the_cap():
    from sparf_amd.batch_plan import Member, plan
    members = [Member(B=1, R=4, to_max=False, nograd=False, mode="val"), Member(B=1, R=30, to_max=False, nograd=False, mode="val")]
    with pytest.raises(L.SparfError, match="one request of 30 rays x 8 samples exceeds a launch set"):
        plan(members, 8, 8, True, False, 0.0, 16, lambda to_max, N: (L.PREC_FP32, None), lambda prec, need: 20 * 8, lambda nograd: contextlib.nullcontext())


def test_plan_hands_the_callables_what_render_batch_handed_them():
    """prec_of sees the sample count of the pass, cap_rows the precision of the group and ALL its sample rows (need =), both under
    the block's grad mode"""
    from sparf_amd.batch_plan import Member, plan
    members = [Member(B=1, R=5, to_max=False, nograd=False, mode="val"), Member(B=1, R=7, to_max=True, nograd=True, mode="val"),
               Member(B=2, R=3, to_max=False, nograd=True, mode="val")]
    log, mode = [], [None]

    @contextlib.contextmanager
    def under(nograd):
        mode[0] = nograd
        yield
        mode[0] = None

    def prec_of(to_max, N):
        log.append(("prec", mode[0], to_max, N))
        return (7 if to_max else 3), None

    def cap_rows(prec, need):
        log.append(("cap", mode[0], prec, need))
        return AMPLE

    plan(members, 8, 4, True, False, 0.0, 16, prec_of, cap_rows, under)
    assert [x for x in log if x[0] == "cap"] == [("cap", False, 3, 40), ("cap", False, 3, 60),
                                                   ("cap", True, 3, 48), ("cap", True, 7, 56), ("cap", True, 3, 72), ("cap", True, 7, 56)]
    assert {x[1:] for x in log if x[0] == "prec"} == {(False, False, 8), (False, False, 12), (True, False, 8), (True, True, 8), (True, False, 12)}


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--record"]:
        with open(TRACE, "w") as f:
            json.dump({k: record_render_batch(**CASES[k]()) for k in sorted(CASES)}, f, indent=0, sort_keys=True)
            f.write("\n")
