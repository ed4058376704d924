"""A stand-in for the loaded library under ops.DconsProject / DconsSelect / DconsLoss (tests/fake_lib.Recorder over the five entry points
of the depth-consistency loss).  The tensors are host memory here, so project and select answer through their `count` pointer as a call that keeps `keep` of its points (default: all) would:
the glue's one readback then reads a number.  The workspace query answers as the library does and is not recorded."""
import ctypes

from tests import fake_lib

_FORMS = ("points_w", "pixels_ref", "depth_ref", "K_ref", "pose_c2w_ref", "ref_rows", "pose_w2c_unseen", "unseen_rows", "K_unseen", "n")
DCONS_CALLS = {
    "sparf_dcons_project": _FORMS + ("H", "W", "depth_min", "depth_min_dev", "uv", "z", "dst", "src", "count", "workspace"),
    "sparf_dcons_project_backward": _FORMS + ("dst", "d_uv", "d_z", "d_points_w", "d_depth_ref"),
    "sparf_dcons_select": ("vis", "uv", "z", "m", "thresh", "uv_out", "z_out", "vis_out", "dst", "src", "count", "workspace"),
    "sparf_dcons_select_backward": ("dst", "d_uv", "d_z", "m", "d_uv_in", "d_z_in"),
    "sparf_dcons_loss": ("z_pseudo", "vis", "depth", "opacity", "depth_fine", "opacity_fine", "m", "loss_type", "out", "d_z_pseudo", "d_depth",
                         "d_depth_fine", "workspace"),
}
CHUNK = 4096                     # csrc/dcons.h DCONS_CHUNK
BYTES_PER_CHUNK = 4 * 8          # DCONS_NACC doubles


def workspace_bytes(n):
    return (n + CHUNK - 1) // CHUNK * BYTES_PER_CHUNK if n > CHUNK else 0


class DconsFakeLib(fake_lib.Recorder):
    def __init__(self):
        super().__init__(DCONS_CALLS)
        self.keep = None         # how many points project / select report as kept (None: all)

    def sparf_dcons_workspace_bytes(self, n):
        return workspace_bytes(n)

    def after(self, name, raw, rec):
        if "count" in raw:
            n = rec.get("n", rec.get("m"))
            ctypes.c_int32.from_address(raw["count"]).value = n if self.keep is None else min(self.keep, n)


def installed():
    return fake_lib.installed(DconsFakeLib())
