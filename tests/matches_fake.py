"""A stand-in for the loaded library under ops.match_compact / ops.match_gather (tests/fake_lib.Recorder over the sampler's two entry
points).  The tensors are host memory here, so compact answers through its `count` pointer as a call that keeps
`keep` pixels (default: every pixel) would -- the glue's one readback then reads a number -- and through `perc`.  The workspace query
answers as the library does and is not recorded."""
import ctypes

from tests import fake_lib

MATCH_CALLS = {
    "sparf_match_compact": ("mask", "H", "W", "y0", "y1", "x0", "x1", "index", "count", "perc", "workspace"),
    "sparf_match_gather": ("index", "count", "sel", "k", "H", "W", "corres", "corres_channel_stride", "conf", "pixels_self", "ray_self",
                           "pixels_other", "ray_other", "conf_out"),
}
CHUNK = 4096                     # csrc/matches.h MATCH_CHUNK
BYTES_PER_CHUNK = 4              # one int32


def workspace_bytes(n):
    return (n + CHUNK - 1) // CHUNK * BYTES_PER_CHUNK if n > CHUNK else 0


class MatchFakeLib(fake_lib.Recorder):
    def __init__(self):
        super().__init__(MATCH_CALLS)
        self.keep = None         # how many pixels compact reports as kept (None: all)

    def sparf_match_workspace_bytes(self, n):
        return workspace_bytes(n)

    def after(self, name, raw, rec):
        if name == "sparf_match_compact":
            n = rec["H"] * rec["W"]
            kept = n if self.keep is None else min(self.keep, n)
            ctypes.c_int32.from_address(raw["count"]).value = kept
            if raw["perc"]:
                ctypes.c_float.from_address(raw["perc"]).value = kept / (n + 1e-6)


def installed():
    return fake_lib.installed(MatchFakeLib())
