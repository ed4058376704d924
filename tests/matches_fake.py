"""A stand-in for the loaded library under ops.match_compact / ops.match_gather (the pattern of tests/dcons_fake.py), for tests that run
the sampler's glue on CPU tensors: it launches nothing and records every call of the two entry points as (name, {argument: True / False
for a pointer given / NULL, the integer}); the stream is left out.  `raw` holds the same calls with the addresses themselves, for tests
of which tensor a pointer is.  The tensors are host memory here, so compact answers through its `count` pointer as a call that keeps
`keep` pixels (default: every pixel) would -- the glue's one readback then reads a number -- and through `perc`.  The workspace query
answers as the library does and is not recorded."""
import contextlib
import ctypes

from sparf_amd import lib as L

MATCH_CALLS = {
    "sparf_match_compact": ("mask", "H", "W", "y0", "y1", "x0", "x1", "index", "count", "perc", "workspace"),
    "sparf_match_gather": ("index", "count", "sel", "k", "H", "W", "corres", "corres_channel_stride", "conf", "pixels_self", "ray_self",
                           "pixels_other", "ray_other", "conf_out"),
}
CHUNK = 4096                     # csrc/matches.h MATCH_CHUNK
BYTES_PER_CHUNK = 4              # one int32


def workspace_bytes(n):
    return (n + CHUNK - 1) // CHUNK * BYTES_PER_CHUNK if n > CHUNK else 0


class MatchFakeLib:
    def __init__(self):
        self.calls, self.raw = [], []
        self.keep = None         # how many pixels compact reports as kept (None: all)

    def sparf_match_workspace_bytes(self, n):
        return workspace_bytes(n)

    def __getattr__(self, name):
        if name not in MATCH_CALLS:
            raise AttributeError(name)           # the sampler enters nothing else

        def call(*args):
            names, types = MATCH_CALLS[name], L.EXPORTS[name][1]
            assert len(args) == len(types) == len(names) + 1, (name, len(args))
            rec, raw = {}, {}
            for n, t, v in zip(names, types, args):
                if t is ctypes.c_void_p:
                    v = v.value if isinstance(v, ctypes.c_void_p) else v
                    rec[n], raw[n] = v is not None and v != 0, v
                else:
                    rec[n] = raw[n] = int(v)
            self.calls.append((name, rec))
            self.raw.append((name, raw))
            if name == "sparf_match_compact":
                n = rec["H"] * rec["W"]
                kept = n if self.keep is None else min(self.keep, n)
                ctypes.c_int32.from_address(raw["count"]).value = kept
                if raw["perc"]:
                    ctypes.c_float.from_address(raw["perc"]).value = kept / (n + 1e-6)
            return 0
        return call

    def names(self):
        return [c[0] for c in self.calls]


@contextlib.contextmanager
def installed():
    lib = MatchFakeLib()
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
