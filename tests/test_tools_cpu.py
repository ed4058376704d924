"""CPU checks of the measurement tooling the committed evidence rests on (no GPU, no compute through the product path)."""
import importlib.util
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_mfma_gap_histogram_counts_instructions_between_mfmas():
    m = _load("tools/mfma_gap_hist.py", "mfma_gap_hist")
    asm = """
	.text
kernel:
	s_load_dword s0, s[0:1], 0x0
	v_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], a[0:15]
	; a comment
	ds_read_b128 v[0:3], v8
	s_waitcnt lgkmcnt(0)
.LBB0_1:
	v_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], a[0:15]
	v_mfma_f32_32x32x16_bf16 a[16:31], v[0:3], v[4:7], a[16:31]
	v_max_i32_e32 v0, 0, v0
	s_endpgm
"""
    assert m.gaps_of(asm) == [2, 0]          # instructions before the first and after the last MFMA do not count


def test_kernel_stream_diff_compares_listings_without_addresses_and_comments():
    m = _load("tools/kernel_stream.py", "kernel_stream_diff")
    head = ["\ts_load_dword s0, s[0:1], 0x0                                // 000000001000:", "\ts_waitcnt lgkmcnt(0)   // 000000001008:"]
    loop = ["\tv_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], a[0:15]   // 000000001010:", "\tds_read_b128 v[0:3], v8   // 000000001018:",
            "\tv_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], a[0:15]   // 000000001020:", "\ts_cbranch_scc1 65529   // 000000001028: <k+0x10>"]
    tail = ["\ts_endpgm   // 00000000102C:", ""]
    a = {"k_same": head + loop + tail, "k_prologue": head + loop + tail, "k_loop": head + loop + tail, "k_gone": head + tail}
    moved = [line.replace("0000000010", "0000000320") for line in head + loop + tail]           # the same code at another address
    shifted = [line.replace("0000000010", "0000000011") for line in head[1:] + loop + tail]
    b = {"k_same": moved,
         "k_prologue": [head[0], "\ts_mov_b32 s1, 0   // 000000001004:"] + shifted,                # one instruction more, before the loop
         "k_loop": head + [loop[0], loop[1].replace("b128 v[0:3]", "b64 v[0:1]")] + loop[2:] + tail,    # one instruction changed between the MFMAs
         "k_new": head + tail}
    assert m.mfma_loops(m.parsed(a["k_loop"])) == [(0x1010, 0x1028)]
    got = {name: (verdict, d) for name, verdict, d in m.compare_listings(a, b)}
    assert {k: v[0] for k, v in got.items()} == {"k_same": "IDENTICAL", "k_prologue": "DIFFER", "k_loop": "DIFFER", "k_gone": "ONLY_A", "k_new": "ONLY_B"}
    d = got["k_prologue"][1]
    assert d["lines"] == (7, 8) and d["hist"] == {"s_mov_b32": [0, 1]} and d["only"] == (0, 1) and d["in_tile_loop"] == (0, 0)
    d = got["k_loop"][1]
    assert d["lines"] == (7, 7) and d["hist"] == {"ds_read_b128": [1, 0], "ds_read_b64": [0, 1]} and d["only"] == (1, 1) and d["in_tile_loop"] == (1, 1)


def test_kernel_stream_diff_pairs_renamed_kernels_and_ignores_the_padding_behind_a_kernel():
    """A refactor that turns kernels into template instances renames them: with a table of `old name = new name` lines the diff
    compares each under its new name; without it they are ONLY_A and ONLY_B.  The s_nop padding behind the last kernel of a section
    belongs to no kernel's code; whatever else follows a kernel's last s_endpgm does."""
    m = _load("tools/kernel_stream.py", "kernel_stream_renames")
    body = ["\ts_load_dword s0, s[0:1], 0x0   // 000000001000:", "\tv_add_f64 v[0:1], v[0:1], v[2:3]   // 000000001008:", "\ts_endpgm   // 000000001010:"]
    pad = ["\ts_nop 0   // 000000001014:", "\ts_nop 0   // 000000001018:"]
    other = body[:1] + ["\tv_mul_f64 v[0:1], v[0:1], v[2:3]   // 000000001008:"] + body[2:]
    a = {"sparf::unit_single_kernel": body + pad, "sparf::unit_finish_kernel": body, "sparf::unit_gather_kernel": body}
    b = {"sparf::sum_single_kernel<sparf::Unit>": body, "sparf::sum_finish_kernel<sparf::Unit>": other, "sparf::unit_gather_kernel": body + pad}
    verdicts = lambda a, b: {name: verdict for name, verdict, _ in m.compare_listings(a, b)}
    assert verdicts(a, b) == {"sparf::unit_single_kernel": "ONLY_A", "sparf::unit_finish_kernel": "ONLY_A", "sparf::unit_gather_kernel": "IDENTICAL",
                              "sparf::sum_single_kernel<sparf::Unit>": "ONLY_B", "sparf::sum_finish_kernel<sparf::Unit>": "ONLY_B"}
    table = m.read_renames("# the two kernels of the sum\n\nsparf::unit_single_kernel = sparf::sum_single_kernel<sparf::Unit>\n"
                           "sparf::unit_finish_kernel = sparf::sum_finish_kernel<sparf::Unit>\n")
    assert table == {"sparf::unit_single_kernel": "sparf::sum_single_kernel<sparf::Unit>", "sparf::unit_finish_kernel": "sparf::sum_finish_kernel<sparf::Unit>"}
    names = m.renamed({k: k for k in a}, table)
    assert verdicts({names[k]: v for k, v in a.items()}, b) == {"sparf::sum_single_kernel<sparf::Unit>": "IDENTICAL",
                                                                "sparf::sum_finish_kernel<sparf::Unit>": "DIFFER", "sparf::unit_gather_kernel": "IDENTICAL"}
    try:
        m.read_renames("sparf::unit_single_kernel sparf::sum_single_kernel")
    except ValueError:
        pass
    else:
        raise AssertionError("a line without ` = ` was accepted")
    # only that padding is dropped: a block the compiler laid out behind the last s_endpgm is the kernel's code and is compared
    tail = ["\tv_mov_b32 v0, 0   // 000000001014:", "\ts_branch 65530   // 000000001018:"]
    moved = [tail[0].replace("v0, 0", "v0, 1"), tail[1]]
    assert verdicts({"k": body + tail + pad}, {"k": body + tail}) == {"k": "IDENTICAL"}
    assert verdicts({"k": body + tail}, {"k": body + moved + pad}) == {"k": "DIFFER"}
    assert verdicts({"k": body + tail}, {"k": body}) == {"k": "DIFFER"}
    (_, _, d), = m.compare_listings({"k": body + tail + pad}, {"k": body + tail})
    assert d["lines"] == (5, 5)


def test_fp8_emulation_matches_torch_casts():
    """tests/tools/save_precision_study.py rounds with its own arithmetic (a per-tile scale, then the 8-bit grid): with the scale
    forced to one the grid must be torch's float8_e4m3fn / float8_e5m2 (round to nearest even, subnormals, saturation)."""
    m = _load("tests/tools/save_precision_study.py", "save_precision_study")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 32, generator=g) * torch.logspace(-4, 2.5, 64)[:, None]
    for dt, (mant, emin, vmax) in ((torch.float8_e4m3fn, (3, -6, 448.0)), (torch.float8_e5m2, (2, -14, 57344.0))):
        xs = x / x.abs().max() * vmax        # amax = vmax -> scale 2^0 (one tile: all rows); magnitudes down to the subnormals
        got = m.q_fp8_tiles(xs, mant, emin, vmax, tile=64)
        ref = xs.to(dt).float()
        assert torch.equal(got, ref)
    # scaled: relative error of an e4m3 grid is <= 2^-4 for values within 2^-6 of the tile's largest
    q = m.q_fp8_tiles(x, 3, -6, 448.0)
    big = x.abs() >= x.abs().reshape(2, -1).amax(dim=1).repeat_interleave(32)[:, None] * 2.0 ** -6
    assert float(((q - x).abs() / x.abs())[big].max()) <= 2.0 ** -4 + 1e-6


def test_emulated_linear_is_the_plain_one_without_rounding():
    m = _load("tests/tools/save_precision_study.py", "save_precision_study2")
    import types
    cfg = types.SimpleNamespace(fwd="fp32", dy="fp32", dgrad_w="fp32", save_x="fp32", save_dy="fp32")
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 5, 8, generator=g, requires_grad=True)
    w = torch.randn(4, 8, generator=g, requires_grad=True)
    b = torch.randn(4, generator=g, requires_grad=True)
    up = torch.randn(3, 5, 4, generator=g)
    got = torch.autograd.grad((m.EmuLinear.apply(x, w, b, cfg) * up).sum(), (x, w, b))
    ref = torch.autograd.grad((torch.nn.functional.linear(x, w, b) * up).sum(), (x, w, b))
    for a, r in zip(got, ref):
        assert torch.allclose(a, r, rtol=1e-5, atol=1e-6)


def test_loss_units_take_ordered_compaction_and_block_sums_from_ordered_h():
    """The loss kernels' two promises -- a selection in torch.where's order bit for bit, sums with the same bits from call to call --
    rest on the wave ballot ranks and the fixed-order block sums of csrc/ordered.h.  The six units call that one copy: each includes
    the header and holds no ballot and no shuffle butterfly of its own, comments included (a seventh loss unit belongs in the list).
    The chunked launch schemes around those routines -- single / partial / finish kernels of a sum, single / counts / write kernels of
    a compaction -- are ordered.h's templates too: no unit defines such a kernel of its own, but reproj.hip, whose strided grid with a
    seeds pass is another scheme."""
    import re
    from sparf_amd import build as B
    assert "ordered.h" in B.HEADERS, "source_hash() does not cover ordered.h"
    header = open(os.path.join(B.CSRC, "ordered.h")).read()
    assert "__ballot" in header and "__shfl_xor" in header
    scheme = re.compile(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(\w+_(?:single|partial|finish|counts|write)_kernel)\s*\(")
    assert {"ordered_sum_single_kernel", "ordered_sum_partial_kernel", "ordered_sum_finish_kernel", "ordered_compact_single_kernel",
            "ordered_compact_counts_kernel", "ordered_compact_write_kernel"} <= set(scheme.findall(header))
    for unit in ("reproj.hip", "dcons.hip", "photo.hip", "matches.hip", "colmap.hip", "depth_err.hip"):
        text = open(os.path.join(B.CSRC, unit)).read()
        assert '#include "ordered.h"' in text, f"{unit} does not include ordered.h"
        for word in ("__ballot", "__shfl_xor"):
            assert word not in text, f"{unit} has a {word} of its own: the routine lives in ordered.h"
        if unit != "reproj.hip":
            assert not scheme.findall(text), f"{unit} defines {scheme.findall(text)}: the chunked launch schemes live in ordered.h"
    assert scheme.findall(open(os.path.join(B.CSRC, "reproj.hip")).read()) == ["reproj_single_kernel", "reproj_partial_kernel"]      # (the pattern finds them)


def test_shipped_kernels_have_no_experiment_or_probe_flag_on():
    """The kernel sources hold the shipped configuration and the instruments still in use.  The switches of settled
    experiments are retired: their names appear in no code file (the documents keep the record).  The switches that stay have the
    shipped value as their guarded default; the probes give WRONG RESULTS by design and must never be defined in the sources or by
    sparf_amd.build."""
    import re
    from sparf_amd import build as B
    src = {f: open(os.path.join(B.CSRC, f)).read() for f in os.listdir(B.CSRC) if f.endswith((".h", ".hip", ".cpp"))}
    text = "\n".join(src.values())
    retired = ("SP_WG_Q8_HALVES", "SP_WG_SPREAD", "SP_WG_NBUF_MAX", "SP_WG_NT", "SP_WG_X3_ROWS", "SP_BWD_STAGGER", "SP_BWD_DEFER", "SP_BWD_SPREAD",
               "SP_DEFER_EPI", "SP_LAZY_ACC_READ", "SP_SLOT_BALANCE", "SP_SPREAD_NUM", "SP_SPREAD_DEN", "SP_X3_PREFETCH", "SP_X3_DGRAD_PREFETCH",
               "SP_SAVE_AUX", "SP_X3_DGRAD_WAVES", "SP_X3_DGRAD_FULL", "SP_X3_SAVE_PLANES", "SP_PROBE_NO_ENCODING", "SP_PROBE_NO_TILE_END",
               "SP_PROBE_HALF_SAVES", "wgrad_q8h_kernel", "launch_wgrad_partials", "launch_wgrad_reduce", "nplanes_of")
    code = dict(src)
    code["build.py"] = open(os.path.join(B.HERE, "build.py")).read()
    tools = os.path.join(ROOT, "tools")
    for d, _, files in os.walk(tools):
        for f in files:
            if not f.endswith((".md", ".rst", ".txt")):
                code[os.path.relpath(os.path.join(d, f), ROOT)] = open(os.path.join(d, f), errors="replace").read()
    for name in retired:
        hits = [f for f, t in code.items() if name in t]
        assert not hits, f"{name} is retired but still named in {hits}"
    expected = {"SP_X3_DGRAD_PARTS": "2", "SP_XYZ_EXACT": "0"}
    for name, val in expected.items():
        m = re.search(r"#ifndef %s\s*\n#define %s (\S+)" % (name, name), text)
        assert m, f"{name}: no guarded default found"
        assert m.group(1) == val, (name, m.group(1), "shipped default is", val)
    for name in ("SP_PROBE_NO_STORES", "SP_PROBE_NO_DMA", "SP_PROBE_NO_BARRIER", "SP_PROF"):
        assert name in text, f"{name}: the instrument is gone from the sources"
        assert not re.search(r"^\s*#\s*define\s+%s\b" % name, text, flags=re.M), f"{name} is defined in the sources"
        assert not any(name in f for f in B.FLAGS), f"{name} is passed by the default build"


# ---- tools/paired_bench.py: the measurement scheme of the eleven comparison benches
PAIRED_TOOLS = ("colmap_depth_bench", "corres_loss_bench", "dcons_front_bench", "depth_cons_bench", "depth_err_bench", "image_metrics_bench",
                "match_select_bench", "photo_loss_bench", "pose_eval_bench", "pose_optim_bench", "test_optim_bench")


def _paired():
    return _load("tools/paired_bench.py", "paired_bench")


def test_paired_bench_alternate_warms_every_leg_up_then_alternates_the_blocks():
    pb = _paired()
    calls = []

    def block(work, iters):
        calls.append((work, iters))
        return len(calls)

    got = pb.alternate({"a": "A", "b": "B", "c": "C"}, blocks=2, iters=7, warmup=3, block=block)
    assert calls == [("A", 3), ("B", 3), ("C", 3)] + [("A", 7), ("B", 7), ("C", 7)] * 2
    assert got == {"a": [4, 7], "b": [5, 8], "c": [6, 9]}
    assert list(got) == ["a", "b", "c"]


def test_paired_bench_records_and_the_leg_against_its_baseline():
    import math
    pb = _paired()
    base, other = [4.0, 1.0, 3.0, 2.0], [0.5, 1.0, 0.25, 0.75]          # an even number of blocks: the median is the mean of the middle two
    assert pb.flat(base) == dict(ms_per_iter_median=2.5, ms_per_iter_min=1.0, ms_per_iter_max=4.0, ms_per_iter_blocks=base)
    assert list(pb.flat(base)) == ["ms_per_iter_median", "ms_per_iter_min", "ms_per_iter_max", "ms_per_iter_blocks"]
    assert pb.summary(other) == dict(median=0.625, min=0.25, max=1.0, blocks=other)
    assert list(pb.summary(other)) == ["median", "min", "max", "blocks"]
    assert pb.versus(base, other) == (0.25, 1.875, True)                   # other.max == base.min: they overlap
    below = [0.5, math.nextafter(1.0, 0.0), 0.25, 0.75]                   # one ulp below: they do not
    assert pb.versus(base, below)[2] is False
    assert pb.versus(base, [5.0, 6.0]) == (2.2, -3.0, True)


def test_paired_bench_activities_sorts_the_names_of_a_traced_window():
    pb = _paired()
    long = "void sparf::ordered_sum_single_kernel<sparf::DepthErr>(" + "x" * 80 + ")"
    device = ["short_kernel", "Memcpy DtoH (Device -> Pinned)", long, "Memcpy HtoD (Pageable -> Device)", "Memset (Device)"]
    host = ["aten::nonzero", "aten::_local_scalar_dense", "hipStreamSynchronize", "aten::_local_scalar_dense", "hipMemcpyWithStream", "hipMemcpyAsync",
            "hipDeviceSynchronize"]
    for every in (False, True):
        t = pb.activities(device, host, every_device_sync=every)
        assert t.kernels == ["short_kernel", long]
        assert t.copies == [device[1], device[3], device[4]]
        assert t.copies_by_label == {device[1]: 1, device[3]: 1, device[4]: 1} and list(t.copies_by_label) == sorted(t.copies)
        assert (t.host_to_device, t.readbacks_by_label, t.readbacks_asked) == (1, 1, 3)
        assert t.host_waits == ["hipMemcpyWithStream", "hipStreamSynchronize"]
        assert t.by_name == {"short_kernel": 1, long[:80]: 1} and [len(k) for k in t.by_name] == [12, 80]
    # no closing synchronise in the list: nothing is removed; the profiler's own second one stays unless every one is asked out
    assert pb.activities([], host[:-1]).host_waits == ["hipMemcpyWithStream", "hipStreamSynchronize"]
    twice = host + ["hipDeviceSynchronize"]
    assert pb.activities([], twice).host_waits == ["hipDeviceSynchronize", "hipMemcpyWithStream", "hipStreamSynchronize"]
    assert pb.activities([], twice, every_device_sync=True).host_waits == ["hipMemcpyWithStream", "hipStreamSynchronize"]
    assert pb.activities(device, []).readbacks_asked == 0                     # a device-only trace asks for none


def test_paired_bench_existing_and_emit(tmp_path, capsys):
    import json
    pb = _paired()
    out = str(tmp_path / "not" / "there" / "doc.json")
    assert pb.existing(out, dict(rows={})) == dict(rows={}) and pb.existing(None, 5) == 5
    doc = dict(tool="t", rows=dict(a=dict(n=1)))
    pb.emit(doc, out)                                                         # the missing directory is created
    text = json.dumps(doc, indent=1)
    assert capsys.readouterr().out == text + "\n" and open(out).read() == text + "\n"
    again = pb.existing(out, dict(rows={}))                                   # a --trace-only style update keeps the keys already there
    again["rows"].setdefault("a", {})["traced"] = dict(kernels=2)
    pb.emit(again, out, one_line=True)
    assert capsys.readouterr().out == json.dumps(again) + "\n" and "\n" not in json.dumps(again)
    assert open(out).read() == json.dumps(again, indent=1) + "\n"
    assert json.load(open(out)) == dict(tool="t", rows=dict(a=dict(n=1, traced=dict(kernels=2))))
    pb.emit(doc, None)                                                        # no --out: stdout alone
    assert capsys.readouterr().out == text + "\n"


def test_paired_bench_diff_prints_what_differs_and_is_no_timing(tmp_path, capsys):
    import copy
    import json
    pb = _paired()
    a = dict(tool="t", label="parent", device="gpu A", blocks=2, legs=["series", "fused"],
             rows=dict(r=dict(series=dict(ms_per_iter_median=1.5, ms_per_iter_blocks=[1.0, 2.0], device_ms_per_iter=dict(median=1.5, blocks=[1.0, 2.0])),
                              fused_over_series=0.5, blocks_overlap=False, result=dict(loss=0.25, count=7),
                              traced=dict(kernels=3, copies_and_memsets=2, by_name={"k": 3}))))
    b = copy.deepcopy(a)
    b.update(label="branch", device="gpu B")
    r = b["rows"]["r"]
    r["series"].update(ms_per_iter_median=1.75, ms_per_iter_blocks=[1.5, 2.0, 2.5], device_ms_per_iter=dict(median=9.0, blocks=[9.0]))
    r.update(fused_over_series=0.75, blocks_overlap=True)
    assert pb.diff(a, b) == []                                                # timings, label and device alone
    paths = {name: str(tmp_path / f"{name}.json") for name in "abc"}
    for name, doc in zip("ab", (a, b)):
        json.dump(doc, open(paths[name], "w"))
    assert pb.main(["diff", paths["a"], paths["b"]]) == 0 and capsys.readouterr().out == ""
    del r["traced"]["by_name"]                                                # a missing key, a new key, two changed counts
    r["traced"]["copies_and_memsets"] = 4
    r["result"].update(count=8, more=1)
    b["legs"].append("body")
    lines = pb.diff(a, b)
    assert lines == ["only in A: rows/r/traced/by_name/k", "only in B: legs/2", "only in B: rows/r/result/more",
                     "differs: rows/r/result/count: 7 != 8", "differs: rows/r/traced/copies_and_memsets: 2 != 4"]
    c = copy.deepcopy(a)                                                      # a second run of A's tree: its count is not the same from run to run
    c["rows"]["r"]["result"]["count"] = 9
    assert pb.diff(a, b, like=c) == [x for x in lines if "result/count" not in x]
    for name, doc in zip("bc", (b, c)):
        json.dump(doc, open(paths[name], "w"))
    assert pb.main(["diff", paths["a"], paths["b"], "--like", paths["c"]]) == 1
    assert capsys.readouterr().out.splitlines() == pb.diff(a, b, like=c)


def test_paired_tools_hold_no_timing_or_profiler_scheme_of_their_own():
    """The eleven comparison benches take their blocks, their records and their profiler pass from tools/paired_bench.py (a twelfth
    bench with legs belongs in the list): none times with device events, opens the profiler or takes a median itself."""
    for tool in PAIRED_TOOLS:
        text = open(os.path.join(ROOT, "tools", tool + ".py")).read()
        assert "import paired_bench" in text, f"{tool} does not import paired_bench"
        for word in ("torch.cuda.Event", "torch.profiler", "statistics."):
            assert word not in text, f"{tool} has a {word} of its own: the scheme lives in tools/paired_bench.py"
    shared = open(os.path.join(ROOT, "tools", "paired_bench.py")).read()
    assert all(word in shared for word in ("torch.cuda.Event", "torch.profiler", "statistics."))


def test_paired_tools_load_and_fail_without_a_device(monkeypatch):
    """A measuring path that finds no GPU fails, it does not fall back: main() ends in the SystemExit that names the tool."""
    import pytest
    from sparf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libsparf_hip.so is not built")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)           # (on a machine with a device: what the tools ask)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    for tool in PAIRED_TOOLS:
        m = _load(f"tools/{tool}.py", tool + "_loaded")
        monkeypatch.setattr("sys.argv", [f"tools/{tool}.py"])
        with pytest.raises(SystemExit) as e:
            m.main()
        assert str(e.value) == f"tools/{tool}.py measures on the GPU: no device found"
