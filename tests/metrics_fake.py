"""A stand-in for the loaded library under ops.image_metrics (the pattern of tests/photo_fake.py), for tests that run the metrics glue on
CPU tensors: it launches nothing and records every call of the entry point as a dict of the struct's fields -- a pointer as its address
(None for NULL), a stride array as a tuple, integers and the scale as they are; the stream is left out.  The tensors are host memory
here, so the call answers through its `out` and `counts` pointers with recognisable numbers.  The workspace query answers as the
library does and is not recorded."""
import ctypes

from sparf_amd import lib as L
from tests import fake_lib

TH, TW, NACC = 16, 32, 18        # csrc/metrics.h METRICS_TH, METRICS_TW, METRICS_NACC
OUT = tuple(float(i) + 0.5 for i in range(20))           # what a call leaves in out[2][10]
COUNTS = (7, 11)


def workspace_bytes(B, H, W):
    if B < 1 or H < 1 or W < 1:
        return 0
    return B * ((H + TH - 1) // TH) * ((W + TW - 1) // TW) * NACC * 8


class MetricsFakeLib:
    def __init__(self):
        self.calls = []

    def sparf_image_metrics_workspace_bytes(self, B, H, W):
        return workspace_bytes(B, H, W)

    def sparf_image_metrics(self, ref, stream):
        a = ref._obj
        assert isinstance(a, L.ImageMetrics)
        rec = {}
        for name, ctype in L.ImageMetrics._fields_:
            v = getattr(a, name)
            rec[name] = tuple(v) if name.endswith("_stride") else v
        self.calls.append(rec)
        assert rec["workspace"] and rec["workspace_bytes"] == workspace_bytes(a.B, a.H, a.W)
        (ctypes.c_float * 20).from_address(rec["out"])[:] = OUT
        (ctypes.c_int32 * 2).from_address(rec["counts"])[:] = COUNTS
        return 0

    def __getattr__(self, name):
        raise AttributeError(name)               # the metrics functions enter nothing else


def installed():
    """the stand-in under sparf_amd.lib, and the route predicate of sparf_amd.metrics blind to the device (the tensors are on the CPU)"""
    from sparf_amd import metrics
    lib = MetricsFakeLib()
    real_takes = metrics._takes_kernel

    class _OnGpu:                                  # a tensor's device as the predicate reads it
        type = "cuda"

    def takes(pred, gt, pred_fine, fg_mask, depths, depth_gt, valid_depth_gt):
        wrap = lambda t: None if t is None else _View(t)
        return real_takes(wrap(pred), wrap(gt), wrap(pred_fine), wrap(fg_mask), tuple(wrap(d) for d in depths), wrap(depth_gt), wrap(valid_depth_gt))

    class _View:
        def __init__(self, t):
            self.t = t
            self.device, self.layout, self.dtype, self.shape = _OnGpu, t.layout, t.dtype, t.shape

        def dim(self):
            return self.t.dim()

        def numel(self):
            return self.t.numel()

    return fake_lib.installed(lib, (metrics, "_takes_kernel", takes))
