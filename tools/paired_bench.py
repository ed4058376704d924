"""The measurement scheme of the comparison benches under tools/ (*_bench.py with legs), in one place.

    import paired_bench as pb                                   (the tools run as scripts: tools/ is first on sys.path)
    python tools/paired_bench.py diff A.json B.json [--like C.json]

Alternating blocks.  The legs of a row -- the torch series an unmodified trainer runs, and the device unit that replaces it -- run in
ONE process: first a warm-up of every leg, then `blocks` rounds in which each leg in turn runs one block of `iters` iterations, so that
every leg sees the same minutes of the machine.  A block is timed by device events around its iterations, between two synchronises; a
readback stalls the host inside the block, so the figure is wall time as the device saw it.  The host clock around the enqueue of the
same block (before the closing synchronise) is taken too.  Per leg the blocks are reported as median and min ... max, in one of two
spellings (`flat`, `summary`: the documents under profiles/ keep the spelling they were written in), and a leg against its baseline
as `versus`: ratio and difference of the medians, and whether the slowest block of the one reaches the fastest of the other.

The profiler pass.  `traced` runs ONE iteration under torch.profiler, closed by a synchronise inside the profiled region, and
`activities` sorts the names of its events:
  kernel        a device event that is no copy or memset;
  copy, memset  a device event whose label starts with `memcpy` / `memset` (any case); a host-to-device copy has `htod` in its label;
  readback      by label: a copy with `dtoh` in its label; where it is asked for (host events, `host=True`): an `aten::nonzero` (a
                boolean selection reads its count) or an `aten::_local_scalar_dense` (`.item()`, `.tolist()` of one element);
  host wait     a runtime call `hip*` / `cuda*` with `Synchronize` in its name, or `Memcpy` without `Async`, minus the synchronise
                that closes the window.
Each tool reports the fields its document has.

`diff` compares two documents of one tool, e.g. a parent's and a branch's: the keys only one of them has, and the leaves that differ
and are no timings.  With --like C (a second run of A's tree) only those leaves on which A and C agree: what differs between two runs
of one tree is that tree's own run-to-run variation."""
import argparse
import json
import os
import statistics
import sys
import time
import types


def device_block(work, iters):
    """-> (device ms, host ms) per iteration of `iters` iterations of work.iteration()"""
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        work.iteration()
    e1.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, host / iters


def alternate(works, blocks, iters, warmup, block=device_block):
    """-> {leg: [what `block` returned for each of the leg's blocks]}"""
    for w in works.values():                                   # warm-up of every shape the timed window uses
        block(w, warmup)
    out = {k: [] for k in works}
    for _ in range(blocks):                                    # alternating blocks: every leg sees the same minutes of the machine
        for k, w in works.items():
            out[k].append(block(w, iters))
    return out


def device_ms(works, blocks, iters, warmup):
    """alternate() on device_block, the device time alone -> {leg: [ms per iteration of each block]}"""
    return {k: [d for d, _ in t] for k, t in alternate(works, blocks, iters, warmup).items()}


def flat(values):
    return dict(ms_per_iter_median=statistics.median(values), ms_per_iter_min=min(values), ms_per_iter_max=max(values), ms_per_iter_blocks=values)


def summary(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values), blocks=values)


def versus(base, other):
    """the blocks of a leg against its baseline's -> (other over base, base minus other, whether their blocks overlap)"""
    b, o = statistics.median(base), statistics.median(other)
    return o / b, b - o, max(other) >= min(base)


def activities(device_names, host_names, every_device_sync=False):
    """the names of one traced window's device and host events, sorted as the module's text says.  The synchronise that closes the
    window: one `hipDeviceSynchronize` is taken out of the host waits; `every_device_sync`: every `*DeviceSynchronize` is, the
    profiler's own with it."""
    copies = [x for x in device_names if x.lower().startswith(("memcpy", "memset"))]
    kernels = [x for x in device_names if x not in copies]
    waits = [x for x in host_names if x.startswith(("hip", "cuda")) and ("Synchronize" in x or ("Memcpy" in x and "Async" not in x))]
    if every_device_sync:
        waits = [x for x in waits if "DeviceSynchronize" not in x]
    else:
        for own in ("hipDeviceSynchronize", "cudaDeviceSynchronize"):
            if own in waits:
                waits.remove(own)
                break
    by_name = {}
    for x in kernels:
        by_name[x[:80]] = by_name.get(x[:80], 0) + 1
    return types.SimpleNamespace(kernels=kernels, copies=copies, copies_by_label={x: copies.count(x) for x in sorted(set(copies))},
                                 host_to_device=sum("htod" in x.lower() for x in copies), readbacks_by_label=sum("dtoh" in x.lower() for x in copies),
                                 readbacks_asked=sum(x in ("aten::nonzero", "aten::_local_scalar_dense") for x in host_names), host_waits=sorted(waits),
                                 by_name=by_name)


def traced(fn, host=False, **kw):
    """-> activities() of ONE call of fn under the profiler; `host`: the host's events too (readbacks where asked, host waits)"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=([ProfilerActivity.CPU] if host else []) + [ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    events = list(prof.events())
    on_device = lambda e: str(e.device_type).endswith("CUDA")
    return activities([e.name for e in events if on_device(e)], [e.name for e in events if not on_device(e)], **kw)


def parser(doc, blocks=5, iters=20, warmup=5):
    """the arguments every tool has; the tool adds its own"""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=blocks)
    ap.add_argument("--iters", type=int, default=iters)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--label", default=None, help="free text kept in the document (which commit this tree is)")
    return ap


def gpu_or_exit(tool):
    """-> the device; a measuring tool that finds none fails"""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} measures on the GPU: no device found")
    return torch.device("cuda:0")


def existing(out, default):
    """the document already at `out` (a --trace-only run adds its key to it), or `default`"""
    if out and os.path.exists(out):
        with open(out) as f:
            return json.load(f)
    return default


def emit(doc, out, one_line=False):
    """the document on stdout and, with `out`, in that file"""
    text = json.dumps(doc, indent=1)
    print(json.dumps(doc) if one_line else text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


# ---- python tools/paired_bench.py diff
def leaves(doc, path=()):
    """-> {path: leaf} of a document; the list of a leg's blocks is one leaf"""
    if isinstance(doc, list) and not (path and "blocks" in str(path[-1])):
        doc = dict(enumerate(doc))
    if not isinstance(doc, dict) or not doc:
        return {path: doc}
    out = {}
    for k, v in doc.items():
        out.update(leaves(v, path + (k,)))
    return out


def is_timing(path, value):
    keys = [k for k in path if isinstance(k, str)]
    if isinstance(value, list):
        return any("blocks" in k for k in keys)
    return (isinstance(value, float) and any("ms" in k or "_over_" in k for k in keys)) or \
        (isinstance(value, (float, bool)) and any("overlap" in k for k in keys))


def diff(a, b, like=None):
    """-> the lines `diff` prints for documents a and b"""
    a, b, like = leaves(a), leaves(b), None if like is None else leaves(like)
    name = lambda p: "/".join(str(k) for k in p)
    lines = [f"only in {'A' if p in a else 'B'}: {name(p)}" for p in list(a) + list(b) if (p in a) != (p in b)]
    for p, v in a.items():
        if p in b and b[p] != v and p[-1] not in ("label", "device") and not is_timing(p, v) and (like is None or like.get(p, v) == v):
            lines.append(f"differs: {name(p)}: {json.dumps(v)} != {json.dumps(b[p])}")
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", choices=["diff"])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--like", default=None, help="a second run of A's tree: only the leaves on which A and it agree are compared")
    args = ap.parse_args(argv)
    load = lambda p: json.load(open(p))
    lines = diff(load(args.a), load(args.b), like=load(args.like) if args.like else None)
    print("\n".join(lines), end="\n" if lines else "")
    return 1 if lines else 0


if __name__ == "__main__":
    sys.exit(main())
