"""A stand-in for the loaded library under ops.ReprojLoss / ReprojPairLoss (the pattern of tests/pose_fake.py), for tests that run the
correspondence-loss glue on CPU tensors: it launches nothing and records every call of the two entry points as
(name, {argument: True / False for a pointer given / NULL, the integer, or the float}); the stream is left out.  The workspace query
answers as the library does (host arithmetic) and is not recorded."""
import contextlib
import ctypes

from sparf_amd import lib as L

_OPTS = ("n", "loss_type", "pix_check", "pix_thresh", "depth_check", "depth_thresh")
REPROJ_CALLS = {
    "sparf_reproj_loss": ("pixels_i", "depth_i", "K_i", "pixels_j", "depth_j", "K_j", "T_itoj", "weights") + _OPTS +
                         ("out", "d_depth_i", "d_T", "valid", "workspace"),
    "sparf_reproj_pair_loss": ("pixels_self", "pixels_other", "depth_self", "depth_other", "depth_fine_self", "depth_fine_other", "K_self",
                               "K_other", "pose_self", "pose_other", "weights") + _OPTS +
                              ("out", "d_depth_self", "d_depth_other", "d_depth_fine_self", "d_depth_fine_other", "d_pose_self", "d_pose_other",
                               "workspace"),
}
SINGLE_MAX = 4096                # csrc/reproj.h REPROJ_SINGLE_MAX
WORKSPACE_BYTES = 4 * 64 * 21 * 8


class ReprojFakeLib:
    def __init__(self):
        self.calls = []

    def sparf_reproj_workspace_bytes(self, n):
        return WORKSPACE_BYTES if n > SINGLE_MAX else 0

    def __getattr__(self, name):
        if name not in REPROJ_CALLS:
            raise AttributeError(name)           # the loss functions enter nothing else

        def call(*args):
            names, types = REPROJ_CALLS[name], L.EXPORTS[name][1]
            assert len(args) == len(types) == len(names) + 1, (name, len(args))
            rec = {}
            for n, t, v in zip(names, types, args):
                if t is ctypes.c_void_p:
                    v = v.value if isinstance(v, ctypes.c_void_p) else v
                    rec[n] = v is not None and v != 0
                else:
                    rec[n] = float(v) if t is ctypes.c_float else int(v)
            self.calls.append((name, rec))
            return 0
        return call

    def names(self):
        return [c[0] for c in self.calls]


@contextlib.contextmanager
def installed():
    lib = ReprojFakeLib()
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
