"""A stand-in for the loaded library under ops.Se3Pose / ComposePose / D9Pose (the pattern of tests/glue_fake.py), for tests that run
the pose glue on CPU tensors: it launches nothing and records every call of the six pose entry points as
(name, {argument: True / False for a pointer given / NULL, or the integer}); the stream is left out."""
import contextlib
import ctypes

from sparf_amd import lib as L

POSE_CALLS = {
    "sparf_pose_se3_forward": ("xi", "base", "n", "refine_out", "pose_out"),
    "sparf_pose_se3_backward": ("xi", "base", "n", "d_pose", "d_refine", "d_xi", "d_base"),
    "sparf_pose_compose_forward": ("a", "b", "n", "out"),
    "sparf_pose_compose_backward": ("a", "b", "n", "d_out", "d_a", "d_b"),
    "sparf_pose_d9_forward": ("d9", "invert", "n", "pose_out"),
    "sparf_pose_d9_backward": ("d9", "invert", "n", "d_pose", "d_d9"),
}


class PoseFakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in POSE_CALLS:
            raise AttributeError(name)           # the pose functions enter nothing else

        def call(*args):
            names, types = POSE_CALLS[name], L.EXPORTS[name][1]
            assert len(args) == len(types) == len(names) + 1, (name, len(args))
            rec = {}
            for n, t, v in zip(names, types, args):
                if t is ctypes.c_void_p:
                    v = v.value if isinstance(v, ctypes.c_void_p) else v
                    rec[n] = v is not None and v != 0
                else:
                    rec[n] = int(v)
            self.calls.append((name, rec))
            return 0
        return call

    def names(self):
        return [c[0] for c in self.calls]


@contextlib.contextmanager
def installed():
    lib = PoseFakeLib()
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
