"""A stand-in for the loaded library under ops.ray_depth_err (tests/fake_lib.Recorder over its one entry point).  The tensors are host
memory here, so the call answers through its `out` and `count` pointers with OUT and COUNT.  The workspace query answers as the library
does and is not recorded.  `installed()` also makes the route predicate of sparf_amd.metrics blind to the device."""
import ctypes

from tests import fake_lib

CALLS = {
    "sparf_ray_depth_err": ("depth_gt", "valid", "img_idx", "ray_idx", "per_image", "B_maps", "B", "HW", "N", "depth", "depth_fine", "scale",
                            "scale_dev", "out", "count", "workspace"),
}
CHUNK, NACC = 4096, 5            # csrc/depth_err.h DEPTH_ERR_CHUNK, DEPTH_ERR_NACC
OUT, COUNT = (0.5, 0.75, 0.25, 0.375), 29


def workspace_bytes(rows):
    return (rows + CHUNK - 1) // CHUNK * NACC * 8 if CHUNK < rows <= 1 << 30 else 0


class DepthErrFakeLib(fake_lib.Recorder):
    def __init__(self):
        super().__init__(CALLS)

    def sparf_ray_depth_err_workspace_bytes(self, rows):
        return workspace_bytes(rows)

    def after(self, name, raw, rec):
        (ctypes.c_float * 4).from_address(raw["out"])[:] = OUT
        ctypes.c_int32.from_address(raw["count"]).value = COUNT


def installed():
    from sparf_amd import metrics
    return fake_lib.installed(DepthErrFakeLib(), (metrics, "_on_gpu", lambda device: True))
