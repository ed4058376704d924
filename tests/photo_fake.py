"""A stand-in for the loaded library under ops.PhotoReguLoss (the pattern of tests/dcons_fake.py), for tests that run the photometric
glue on CPU tensors: it launches nothing and records every call of the entry point as (name, {argument: True / False for a pointer
given / NULL, the integer, or the float}); the stream is left out.  The tensors are host memory here, so the call answers through its
`out` pointer with five recognisable numbers.  The workspace query answers as the library does and is not recorded."""
import contextlib
import ctypes

from sparf_amd import lib as L

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


class PhotoFakeLib:
    def __init__(self):
        self.calls = []

    def sparf_photo_regu_workspace_bytes(self, rows):
        return workspace_bytes(rows)

    def __getattr__(self, name):
        if name not in PHOTO_CALLS:
            raise AttributeError(name)           # the photometric functions enter nothing else

        def call(*args):
            names, types = PHOTO_CALLS[name], L.EXPORTS[name][1]
            assert len(args) == len(types) == len(names) + 1, (name, len(args))
            rec, raw = {}, {}
            for n, t, v in zip(names, types, args):
                if t is ctypes.c_void_p:
                    v = v.value if isinstance(v, ctypes.c_void_p) else v
                    rec[n], raw[n] = v is not None and v != 0, v
                else:
                    rec[n] = float(v) if t is ctypes.c_float else int(v)
            self.calls.append((name, rec))
            (ctypes.c_float * 5).from_address(raw["out"])[:] = OUT
            return 0
        return call

    def names(self):
        return [c[0] for c in self.calls]


@contextlib.contextmanager
def installed():
    lib = PhotoFakeLib()
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
