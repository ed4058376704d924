"""A stand-in for the loaded library under ops.pick_pixels and ops.unseen_pose (tests/fake_lib.Recorder over their two entry points).
The tensors are host memory here, so a call can answer through its pointers.  Without `host`, sparf_unseen_pose leaves k + 1 on the
diagonal of its k-th matrix and ID_OTHER, and sparf_pick_pixels writes nothing.  With `host` -- csrc/pick.h built for the host
(tools/pick_host_lib.cpp, `build_host()`) -- both answer with what the kernels compute, so the glue above them can be held to the fixture
without a GPU.  `installed()` also makes the route predicate of sparf_amd.losses blind to the device."""
import ctypes
import os
import shutil
import subprocess

from tests import fake_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {
    "sparf_pick_pixels": ("perm_a", "n_a", "perm_b", "n_b", "a_w", "a_h", "b_x0", "b_y0", "b_w", "b_h", "W", "patch", "pixels", "rays"),
    "sparf_unseen_pose": ("poses_w2c", "row_floats", "B", "id_self", "w", "one_minus_w", "pose_w2c_ref", "pose_c2w_ref", "pose_c2w_other",
                          "pose_w2c_at_unseen", "id_other"),
}
ID_OTHER = 3
POSE_OUTS = CALLS["sparf_unseen_pose"][6:10]


def build_host(directory):
    """csrc/pick.h as a shared library of host code in `directory`, by the system's C++ compiler -> the loaded library"""
    from sparf_amd import lib as L
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler on this machine"
    out = os.path.join(str(directory), "libpick_host.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "sparf_amd", "csrc"), os.path.join(ROOT, "tools", "pick_host_lib.cpp"),
                    "-o", out], check=True, capture_output=True, text=True, timeout=300)
    lib = ctypes.CDLL(out)
    for name in CALLS:
        fn = getattr(lib, name.replace("sparf_", "host_"))
        fn.restype, fn.argtypes = ctypes.c_int, L.EXPORTS[name][1][:-1]           # the entry point's arguments without the stream
    return lib


class PickFakeLib(fake_lib.Recorder):
    def __init__(self, host=None):
        super().__init__(CALLS)
        self.host = host

    def after(self, name, raw, rec):
        if self.host is not None:
            assert getattr(self.host, name.replace("sparf_", "host_"))(*[raw[k] for k in CALLS[name]]) == 0
        elif name == "sparf_unseen_pose":
            for k, out in enumerate(POSE_OUTS):
                (ctypes.c_float * 16).from_address(raw[out])[:] = [float(k + 1) if i % 5 == 0 else 0.0 for i in range(16)]
            ctypes.c_int32.from_address(raw["id_other"]).value = ID_OTHER


def installed(host=None):
    from sparf_amd import losses
    return fake_lib.installed(PickFakeLib(host), (losses, "_on_gpu", lambda device: True))
