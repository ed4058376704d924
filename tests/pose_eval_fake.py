"""A stand-in for the loaded library under sparf_amd.pose_eval (the pattern of tests/metrics_fake.py), for tests that run the glue on CPU
tensors: it launches nothing and records every call of the two entry points -- sparf_pose_eval as a dict of the struct's fields (a pointer
as its address, None for NULL), sparf_pose_backtrack as a dict of its arguments; the stream is left out.  The tensors are host memory
here, so a call answers through its output pointers with recognisable numbers."""
import ctypes

from sparf_amd import lib as L
from tests import fake_lib

STATS = (0.5, 1.5, 2.5, 3.5)     # what a call leaves in every row of stats
BEST = 1
FILL = 0.25                      # ... and in every other float output; the backtrack leaves its input poses + 1


def _floats(addr, n):
    return (ctypes.c_float * n).from_address(addr)


class PoseEvalFakeLib:
    def __init__(self):
        self.calls = []

    def sparf_pose_eval(self, ref, stream):
        a = ref._obj
        assert isinstance(a, L.PoseEval)
        rec = {name: getattr(a, name) for name, _ in L.PoseEval._fields_}
        rec["entry"] = "sparf_pose_eval"
        self.calls.append(rec)
        S, B = a.S, a.B
        assert all(rec[k] for k in ("pose", "pose_gt", "stats", "errors", "aligned", "sim3", "best", "scores"))
        _floats(a.stats, S * 4)[:] = STATS * S
        for name, n in (("errors", S * 2 * B * 2), ("aligned", S * B * 12), ("sim3", S * L.POSE_EVAL_SIM3), ("scores", S * L.POSE_EVAL_MAX_PAIRS * 3)):
            _floats(rec[name], n)[:] = (FILL,) * n
        (ctypes.c_int32 * S).from_address(a.best)[:] = (BEST if a.flags & L.POSE_EVAL_ALIGN else -1,) * S
        return 0

    def sparf_pose_backtrack(self, gt, n, sim3, stride, out, stream):
        gt, sim3, out = (getattr(p, "value", p) for p in (gt, sim3, out))
        self.calls.append(dict(entry="sparf_pose_backtrack", pose_gt_w2c=gt, n=n, sim3=sim3, sim3_stride=stride, out=out,
                               sim3_values=tuple(_floats(sim3, L.POSE_EVAL_SIM3))))
        _floats(out, n * 12)[:] = [v + 1.0 for v in _floats(gt, n * 12)]
        return 0

    def __getattr__(self, name):
        raise AttributeError(name)               # the pose-evaluation functions enter nothing else


def installed():
    """the stand-in under sparf_amd.lib, and the route predicate of sparf_amd.pose_eval blind to the device (the tensors are on the CPU)"""
    import torch
    from sparf_amd import pose_eval
    on_device = lambda *ts: all(t.dtype == torch.float32 and t.layout == torch.strided for t in ts)
    return fake_lib.installed(PoseEvalFakeLib(), (pose_eval, "_on_device", on_device))
