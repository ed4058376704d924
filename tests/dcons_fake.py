"""A stand-in for the loaded library under ops.DconsProject / DconsSelect / DconsLoss (the pattern of tests/reproj_fake.py), for tests
that run the depth-consistency glue on CPU tensors: it launches nothing and records every call of the five entry points as
(name, {argument: True / False for a pointer given / NULL, the integer, or the float}); the stream is left out.  The tensors are host
memory here, so project and select answer through their `count` pointer as a call that keeps `keep` of its points (default: all) would:
the glue's one readback then reads a number.  The workspace query answers as the library does and is not recorded."""
import contextlib
import ctypes

from sparf_amd import lib as L

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


class DconsFakeLib:
    def __init__(self):
        self.calls = []
        self.keep = None         # how many points project / select report as kept (None: all)

    def sparf_dcons_workspace_bytes(self, n):
        return workspace_bytes(n)

    def __getattr__(self, name):
        if name not in DCONS_CALLS:
            raise AttributeError(name)           # the depth-consistency functions enter nothing else

        def call(*args):
            names, types = DCONS_CALLS[name], L.EXPORTS[name][1]
            assert len(args) == len(types) == len(names) + 1, (name, len(args))
            rec, raw = {}, {}
            for n, t, v in zip(names, types, args):
                if t is ctypes.c_void_p:
                    v = v.value if isinstance(v, ctypes.c_void_p) else v
                    rec[n], raw[n] = v is not None and v != 0, v
                else:
                    rec[n] = float(v) if t is ctypes.c_float else int(v)
            self.calls.append((name, rec))
            if "count" in raw:
                n = rec.get("n", rec.get("m"))
                ctypes.c_int32.from_address(raw["count"]).value = n if self.keep is None else min(self.keep, n)
            return 0
        return call

    def names(self):
        return [c[0] for c in self.calls]


@contextlib.contextmanager
def installed():
    lib = DconsFakeLib()
    fakes = [(L, "load", lambda: lib), (L, "require_gpu", lambda d: d), (L, "on", lambda d: contextlib.nullcontext()),
             (L, "stream_ptr", lambda d: None)]
    saved = [(obj, name, getattr(obj, name)) for obj, name, _ in fakes]
    try:
        for obj, name, f in fakes:
            setattr(obj, name, f)
        yield lib
    finally:
        for obj, name, real in saved:
            setattr(obj, name, real)
