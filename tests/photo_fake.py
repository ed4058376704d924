"""A stand-in for the loaded library under ops.PhotoReguLoss (tests/fake_lib.Recorder over its one entry point).  The tensors are host
memory here, so the call answers through its `out` pointer with five recognisable numbers.  The workspace query answers as the library does and is not recorded."""
import ctypes

from tests import fake_lib

PHOTO_CALLS = {
    "sparf_photo_regu_loss": ("image", "fg_mask", "ray_idx", "per_image", "B", "HW", "N", "rgb", "rgb_fine", "opacity", "opacity_fine", "depth",
                              "depth_fine", "kind", "delta", "patch", "charbonnier", "out", "d_rgb", "d_rgb_fine", "d_opacity", "d_opacity_fine",
                              "d_depth", "d_depth_fine", "workspace"),
}
CHUNK = 4096                     # csrc/photo.h PHOTO_CHUNK
BYTES_PER_CHUNK = 8 * 8          # PHOTO_NACC doubles
OUT = (1.0, 2.0, 3.0, 4.0, 5.0)  # what a call leaves in out[5]


def workspace_bytes(rows):
    return (rows + CHUNK - 1) // CHUNK * BYTES_PER_CHUNK if rows > CHUNK else 0


class PhotoFakeLib(fake_lib.Recorder):
    def __init__(self):
        super().__init__(PHOTO_CALLS)

    def sparf_photo_regu_workspace_bytes(self, rows):
        return workspace_bytes(rows)

    def after(self, name, raw, rec):
        (ctypes.c_float * 5).from_address(raw["out"])[:] = OUT


def installed():
    return fake_lib.installed(PhotoFakeLib())
