"""A stand-in for the loaded library under ops.NerfPass / ops.RenderFn, for tests that run the Python glue on CPU tensors: it launches
nothing, sizes areas with the real library's host arithmetic, and records what the C ABI is handed.

  * `lib.fwd` / `lib.bwd`: (prec, nsamp, has save | has grad_params) of every pass call (tests/test_rays_only_cpu.py);
  * `lib.trace`: every recorded C-ABI call in order with every scalar argument or struct field, the segment entries and far fields
    included, and every pointer as "p<k>", k counting the distinct addresses in the order they first appear: equal addresses get equal
    numbers and null stays None, so aliasing is part of the trace and raw addresses are not (tests/test_glue_trace_cpu.py).

While the stand-in is installed every tensor whose address is taken stays alive (Tensor.data_ptr keeps it), so no address that
reached the trace is handed out again within a test."""
import ctypes

import pytest
import torch

from sparf_amd import lib as L
from tests import fake_lib

# the flat calls that are recorded, with their argument names (include/sparf_hip.h; the stream, last, is left out)
FLAT_CALLS = {
    "sparf_save_bytes": ("prec", "rows"),
    "sparf_bwd_workspace_bytes": ("prec", "nrays", "nsamp", "pose"),
    "sparf_sample_coarse": ("jitter", "u_const", "dmax_ray", "range_dev", "dmin", "scale", "inverse", "nrays", "nsamp", "out"),
    "sparf_sample_fine": ("weights", "t_coarse", "u_mid", "range_dev", "dmin", "dmax", "nrays", "n_coarse", "n_fine", "t_fine", "out"),
    "sparf_sample_fine_hostgrid": ("weights", "t_coarse", "u_mid", "range_dev", "dmin", "dmax", "nrays", "n_coarse", "n_fine", "t_fine", "out"),
    "sparf_c2f_weights": ("progress", "n", "start", "end", "out"),
}
SIZE_CALLS = ("sparf_save_bytes", "sparf_bwd_workspace_bytes")


class FakeLib:
    def __init__(self):
        self.real = L.load()
        self.fwd, self.bwd, self.trace = [], [], []
        self._ids = {}

    def reset(self):
        self.fwd, self.bwd, self.trace, self._ids = [], [], [], {}

    def _ptr(self, p):
        p = p.value if isinstance(p, ctypes.c_void_p) else p
        if p is None:
            return None
        assert p != 0
        return "p%d" % self._ids.setdefault(int(p), len(self._ids))

    def _struct(self, a):
        out = {}
        for name, ctype in a._fields_:
            v = getattr(a, name)
            if name == "seg":
                out[name] = [self._struct(a.seg[i]) for i in range(a.nseg)]
            else:
                out[name] = self._ptr(v) if ctype is ctypes.c_void_p else v
        return out

    def __getattr__(self, name):
        if name not in FLAT_CALLS:
            return lambda *a: 0

        def call(*args):
            names, ctypes_ = FLAT_CALLS[name], L.EXPORTS[name][1]
            ret = getattr(self.real, name)(*args) if name in SIZE_CALLS else 0
            rec = {n: self._ptr(v) if t is ctypes.c_void_p else v for n, t, v in zip(names, ctypes_, args)}
            self.trace.append(dict(call=name, args=rec, **({"ret": ret} if name in SIZE_CALLS else {})))
            return ret
        return call

    def sparf_pass_forward(self, a, stream):
        self.fwd.append((a._obj.prec, a._obj.nsamp, a._obj.save is not None))
        self.trace.append(dict(call="sparf_pass_forward", args=self._struct(a._obj)))
        return 0

    def sparf_pass_backward(self, a, stream):
        assert self.real.sparf_bwd_workspace_bytes(a._obj.prec, a._obj.nrays, a._obj.nsamp, 1) > 0
        self.bwd.append((a._obj.prec, a._obj.nsamp, a._obj.grad_params is not None))
        self.trace.append(dict(call="sparf_pass_backward", args=self._struct(a._obj)))
        return 0


def installed():
    """-> the FakeLib, standing in for the library (and for the GPU checks, the device guard, the stream and the static tables of
    sparf_amd.lib) until the block ends"""
    lib, tables, keep = FakeLib(), {}, []
    real_data_ptr = torch.Tensor.data_ptr

    def data_ptr(t):
        keep.append(t)
        return real_data_ptr(t)

    # (the tables: cached per precision and device, as the real ones are; Tensor.data_ptr is inherited: the class goes back to having none of its own)
    return fake_lib.installed(lib, (L, "tables_device", lambda prec, d: tables.setdefault((prec, str(d)), torch.zeros(4, dtype=torch.int32))),
                              (torch.Tensor, "data_ptr", data_ptr))


@pytest.fixture
def fake():
    with installed() as lib:
        yield lib
