"""Static instruction-stream figures of the built fused-MLP kernels: what the compiler made of a tile, per wave.

    python tools/kernel_stream.py [translation unit ...]        (default: the two config-1 units of the bf16x3 mode; `all` = every
                                                                 fused MLP kernel unit but the ray-gradient-only ones)
    python tools/kernel_stream.py diff <object dir A> <object dir B> [renames]   (every kernel of every unit both directories hold:
                                                                 IDENTICAL, or DIFFER with what differs; e.g. sparf_amd/csrc_<tag> of
                                                                 tools/build_variant.py against sparf_amd/csrc/build -- a refactor's proof
                                                                 of "same machine code".  renames: a file of `name in A = name in B` lines
                                                                 for kernels the refactor renamed, which are then compared under B's name
                                                                 instead of being listed as ONLY_A and ONLY_B)

Reads the gfx950 code object out of sparf_amd/csrc/build/<unit>.o (compiles the unit into a scratch directory when there is no
object newer than its sources) and prints, per kernel: MFMAs, all other instructions, s_nop, v_readlane_b32 / v_writelane_b32
(scalars parked in VGPR lanes), v_pk_add_f32, 16-byte vector buffer stores, and the code-object notes (registers, spills, scratch, LDS).  The tile body of these
kernels is fully unrolled, so the static counts are per tile and wave; the rest of the kernel (prologue, the 15-iteration
encoding loop counted once) is a few hundred instructions.  tests/test_kernel_stream_cpu.py pins the figures of the two kernels."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparf_amd import build as B                                     # noqa: E402

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
NOTE_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def object_of(unit, workdir):
    """the built object of translation unit `unit` (sparf_amd.build's own, i.e. compiled with its FLAGS: variant builds keep their objects
    in other directories), or a fresh one in `workdir` when that is missing or older than the sources"""
    src = os.path.join(B.CSRC, unit)
    obj = os.path.join(B.CSRC, "build", os.path.splitext(unit)[0] + ".o")
    if not B._newer(obj, sorted(B._deps(src))):
        return obj
    obj = os.path.join(workdir, os.path.splitext(unit)[0] + ".o")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + B.FLAGS + ["-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {unit}:\n{r.stdout}")
    return obj


def code_object(obj, workdir):
    fat, co = os.path.join(workdir, "k.fat"), os.path.join(workdir, os.path.basename(obj) + ".co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat, "--targets=" + TARGET, "--output=" + co])
    return co


def notes_of(co):
    """{kernel name: {note key: int}} from the code object's metadata"""
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
        blk = ".agpr_count:" + blk
        vals = {}
        for k in NOTE_KEYS:
            m = re.search(r"\.%s:\s*(\d+)" % k, blk)
            vals[k] = int(m.group(1)) if m else None
        m = re.search(r"\.name:\s*(\S+)", blk)
        if m:
            out[m.group(1)] = vals
    return out


def count_stream(lines):
    """instruction counts of one kernel's disassembly (up to its last s_endpgm: what follows is alignment padding)"""
    ops = []
    for line in lines:
        t = line.split("//")[0].split()
        if t and re.match(r"^[sv]_|^ds_|^buffer_|^global_|^flat_|^scratch_", t[0]):
            ops.append(t[0])
    last = max((i for i, o in enumerate(ops) if o == "s_endpgm"), default=len(ops) - 1)
    c = collections.Counter(ops[:last + 1])
    mfma = sum(v for k, v in c.items() if k.startswith("v_mfma"))
    return {"mfma": mfma, "other": sum(c.values()) - mfma, "s_nop": c["s_nop"], "v_readlane_b32": c["v_readlane_b32"],
            "v_writelane_b32": c["v_writelane_b32"], "v_pk_add_f32": c["v_pk_add_f32"],
            "buffer_store_dwordx4": c["buffer_store_dwordx4"]}          # 16-byte vector buffer stores: the save / gradient-area traffic of a tile


def listings_of(co):
    """{kernel name: disassembly lines} of the code object"""
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    out, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            cur.append(line)
    return out


def streams_of(co):
    """{kernel name: counts} from the disassembly of the code object"""
    return {k: count_stream(v) for k, v in listings_of(co).items()}


def canonical(lines):
    """a listing as comparable text: leading addresses and `//` comments (addresses, encodings) dropped, empty lines too"""
    return [t for t, _ in parsed(lines)]


def parsed(lines):
    """[(canonical text, address or None)] of a listing (the address: what llvm-objdump prints behind `//`)"""
    out = []
    for line in lines:
        code, _, comment = line.partition("//")
        t = " ".join(re.sub(r"^\s*[0-9a-f]+:?\s+(?=\S)", "", code).split())
        if t and t != "...":                                  # ("...": zero padding)
            m = re.match(r"\s*([0-9A-Fa-f]+):", comment)
            out.append((t, int(m.group(1), 16) if m else None))
    return out


def code_of(listing):
    """a parsed listing without the s_nop lines at its end: the padding behind the last kernel of a section, which moves to another
    kernel when a refactor reorders them.  Everything else stays, blocks laid out behind the last s_endpgm included."""
    end = len(listing)
    while end and listing[end - 1][0].split()[0] == "s_nop":
        end -= 1
    return listing[:end]


def mfma_loops(listing):
    """address ranges [target, branch] of the backward branches that enclose an MFMA: the tile loops"""
    mf = [a for t, a in listing if t.startswith("v_mfma") and a is not None]
    out = []
    for t, a in listing:
        if t.startswith(("s_branch", "s_cbranch")) and a is not None and t.split()[-1].isdigit():
            imm = int(t.split()[-1])
            target = a + 4 + 4 * (imm - 65536 if imm >= 32768 else imm)
            if target <= a and any(target <= m <= a for m in mf):
                out.append((target, a))
    return out


def compare_listings(a, b):
    """[(kernel name, verdict, detail)] over two {kernel name: disassembly lines}: verdict IDENTICAL | DIFFER | ONLY_A | ONLY_B.
    IDENTICAL = the same text once addresses and comments are dropped.  detail of DIFFER: line counts of both sides and, with the
    branch distances masked (they move with every instruction in between), the lines only one side has: how many, how many
    of them inside a loop that holds MFMAs (a tile loop), and their mnemonics ({mnemonic: [in A only, in B only]})."""
    import difflib
    out = []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            out.append((name, "ONLY_A" if name in a else "ONLY_B", None))
            continue
        pa, pb = code_of(parsed(a[name])), code_of(parsed(b[name]))
        if [t for t, _ in pa] == [t for t, _ in pb]:
            out.append((name, "IDENTICAL", {"lines": (len(pa), len(pb))}))
            continue
        mask = lambda t: re.sub(r"^(s_c?branch\S*) \d+$", r"\1 .", t)
        la, lb = [mask(t) for t, _ in pa], [mask(t) for t, _ in pb]
        loops = (mfma_loops(pa), mfma_loops(pb))
        hist, only, in_loop = {}, [0, 0], [0, 0]
        for tag, i0, i1, j0, j1 in difflib.SequenceMatcher(None, la, lb, autojunk=False).get_opcodes():
            if tag == "equal":
                continue
            for side, (lines, addrs, x0, x1) in enumerate(((la, pa, i0, i1), (lb, pb, j0, j1))):
                for x in range(x0, x1):
                    hist.setdefault(lines[x].split()[0], [0, 0])[side] += 1
                    only[side] += 1
                    in_loop[side] += any(addrs[x][1] is not None and lo <= addrs[x][1] <= hi for lo, hi in loops[side])
        out.append((name, "DIFFER", {"lines": (len(pa), len(pb)), "hist": hist, "only": tuple(only), "in_tile_loop": tuple(in_loop)}))
    return out


# the fused MLP kernel units of passes with parameter gradients (the ray-gradient-only ones: tests/test_rays_only_cpu.py)
MLP_UNITS = [u for u in B.FUSED_UNITS if u not in B.RAYS_UNITS]


def figures(unit):
    """{kernel name: counts + notes} of every kernel of translation unit `unit`"""
    with tempfile.TemporaryDirectory() as d:
        co = code_object(object_of(unit, d), d)
        notes, streams = notes_of(co), streams_of(co)
    return {k: dict(streams.get(k, {}), **v) for k, v in notes.items()}


def kernel_names(mangled):
    """{mangled: demangled name without return type and argument list}: `sparf::wgrad_kernel<0, false>` stays the same kernel
    when its argument list changes"""
    mangled = list(mangled)
    if not mangled:
        return {}
    import shutil
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt:
        return {m: m for m in mangled}                       # (no demangler: a changed argument list then shows as two kernels)
    dem = subprocess.check_output([filt] + mangled, text=True).split("\n")
    out = {}
    for m, d in zip(mangled, dem):
        if d.endswith(")"):
            depth, i = 0, len(d)
            while i > 0:
                i -= 1
                depth += d[i] == ")"
                depth -= d[i] == "("
                if depth == 0:
                    break
            d = d[:i]
        out[m] = d[5:] if d.startswith("void ") else d
    return out


def read_renames(text):
    """{name in A: name in B} from lines `old name = new name` (demangled, without return type and argument list, as the diff prints
    them); empty lines and lines that start with # are skipped"""
    out = {}
    for line in text.split("\n"):
        if line.strip() and not line.lstrip().startswith("#"):
            old, sep, new = line.partition(" = ")
            if not sep or not old.strip() or not new.strip():
                raise ValueError(f"not an `old name = new name` line: {line!r}")
            out[old.strip()] = new.strip()
    return out


def renamed(names, renames):
    """{key: kernel name} of side A with the renamed kernels under their names in B"""
    return {k: renames.get(name, name) for k, name in names.items()}


def diff_dirs(dir_a, dir_b, renames=None):
    """print the comparison of every unit (object file name) the two object directories share; renames: {kernel name in A: in B}"""
    renames = renames or {}
    units = lambda d: {f for f in os.listdir(d) if f.endswith(".o")}
    ua, ub = units(dir_a), units(dir_b)
    for f in sorted(ua ^ ub):
        print(f"{f}: only in {dir_a if f in ua else dir_b}")
    with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db:
        for f in sorted(ua & ub):
            try:
                ca, cb = code_object(os.path.join(dir_a, f), da), code_object(os.path.join(dir_b, f), db)
            except subprocess.CalledProcessError:
                print(f"{f}: no gfx950 code object (host-only unit)")
                continue
            # (kernels only -- the names the notes list; not device functions or labels)
            by_name = lambda d, names: {names[k]: v for k, v in d.items() if k in names}
            ka, kb = kernel_names(notes_of(ca)), kernel_names(notes_of(cb))
            ka = renamed(ka, renames)
            na, nb = by_name(notes_of(ca), ka), by_name(notes_of(cb), kb)
            sa, sb = by_name(streams_of(ca), ka), by_name(streams_of(cb), kb)
            for name, verdict, d in compare_listings(by_name(listings_of(ca), ka), by_name(listings_of(cb), kb)):
                if verdict != "DIFFER":
                    print(f"{f}: {name}: {verdict}" + (f" ({d['lines'][0]} lines)" if d else ""))
                    continue
                print(f"{f}: {name}: DIFFER  lines {d['lines'][0]} -> {d['lines'][1]}  mfma {sa[name]['mfma']} -> {sb[name]['mfma']}")
                print(f"    lines only in A / B: {d['only'][0]} / {d['only'][1]}, of them inside a loop with MFMAs (tile loop): {d['in_tile_loop'][0]} / {d['in_tile_loop'][1]}")
                net = {k: v for k, v in sorted(d["hist"].items()) if v[0] != v[1]}
                print("    mnemonics whose counts differ (A/B): " + ("  ".join(f"{k} {v[0]}/{v[1]}" for k, v in net.items()) or "none: operands only"))
                print("    notes: " + "  ".join(f"{k} {na[name][k]} -> {nb[name][k]}" + ("" if na[name][k] == nb[name][k] else " (!)") for k in NOTE_KEYS))


if __name__ == "__main__":
    if sys.argv[1:2] == ["diff"]:
        diff_dirs(sys.argv[2], sys.argv[3], read_renames(open(sys.argv[4]).read()) if sys.argv[4:] else None)
        sys.exit(0)
    for unit in MLP_UNITS if sys.argv[1:] == ["all"] else sys.argv[1:] or ["mlp_fwd_x3_train.hip", "mlp_bwd_x3.hip"]:
        for name, f in figures(unit).items():
            print(f"{unit}: {name}")
            print("    " + "  ".join(f"{k} {v}" for k, v in f.items()))
