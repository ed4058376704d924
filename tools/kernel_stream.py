"""Static instruction-stream figures of the built fused-MLP kernels: what the compiler made of a tile, per wave.

    python tools/kernel_stream.py [translation unit ...]        (default: the two config-1 units of the bf16x3 mode; `all` = every
                                                                 unit built from mlp_fwd_impl.h / mlp_bwd_impl.h)

Reads the gfx950 code object out of sparf_amd/csrc/build/<unit>.o (compiles the unit into a scratch directory when there is no
object newer than its sources) and prints, per kernel: MFMAs, all other instructions, s_nop, v_readlane_b32 / v_writelane_b32
(scalars parked in VGPR lanes), v_pk_add_f32, and the code-object notes (registers, spills, scratch, LDS).  The tile body of these
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
            "v_writelane_b32": c["v_writelane_b32"], "v_pk_add_f32": c["v_pk_add_f32"]}


def streams_of(co):
    """{kernel name: counts} from the disassembly of the code object"""
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    out, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            cur.append(line)
    return {k: count_stream(v) for k, v in out.items()}


# every translation unit built from mlp_dev.h + mlp_fwd_impl.h / mlp_bwd_impl.h
MLP_UNITS = [u for u in B.SOURCES if u.startswith(("mlp_fwd_", "mlp_bwd"))]


def figures(unit):
    """{kernel name: counts + notes} of every kernel of translation unit `unit`"""
    with tempfile.TemporaryDirectory() as d:
        co = code_object(object_of(unit, d), d)
        notes, streams = notes_of(co), streams_of(co)
    return {k: dict(streams.get(k, {}), **v) for k, v in notes.items()}


if __name__ == "__main__":
    for unit in MLP_UNITS if sys.argv[1:] == ["all"] else sys.argv[1:] or ["mlp_fwd_x3_train.hip", "mlp_bwd_x3.hip"]:
        for name, f in figures(unit).items():
            print(f"{unit}: {name}")
            print("    " + "  ".join(f"{k} {v}" for k, v in f.items()))
