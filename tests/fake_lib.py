"""What every stand-in for the loaded library shares (tests/*_fake.py), for tests that run the Python glue on CPU tensors: `installed()`
puts a stand-in under sparf_amd.lib, and `Recorder` is the stand-in of a family of flat entry points -- it launches nothing and records
what the C ABI is handed.  A family's module holds what is its own: the table of argument names, the workspace formula and the few
lines that answer through an output pointer."""
import contextlib
import ctypes

from sparf_amd import lib as L
from sparf_amd.patcher import Patcher


@contextlib.contextmanager
def installed(lib, *extra):
    """-> `lib`, standing in for the library -- and for the GPU check, the device guard and the stream of sparf_amd.lib -- until the
    block ends; `extra`: further (obj, name, replacement) patches for the same time.  A name `obj` only inherits (Tensor.data_ptr)
    goes back to being inherited."""
    patches = Patcher("tests.fake_lib.installed", "__exit__")
    try:
        for obj, name, new in [(L, "load", lambda: lib), (L, "require_gpu", lambda d: d), (L, "on", lambda d: contextlib.nullcontext()),
                               (L, "stream_ptr", lambda d: None), *extra]:
            patches.put(obj, name, new)
        yield lib
    finally:
        patches.restore()


class Recorder:
    """The entry points of `table` = {name: argument names, the stream (last) left out}; any other name is an AttributeError: the
    family enters nothing else.  Every call is checked for its arity against L.EXPORTS and appended to `calls` as (name, {argument:
    True / False for a pointer given / NULL, the integer, or the float}) and to `raw` as the same with the addresses themselves (None
    for NULL), for tests of which tensor a pointer is; then `after(name, raw, rec)` may answer through an output pointer (the tensors
    are host memory here).  Every call returns 0."""

    def __init__(self, table):
        self.table, self.calls, self.raw = table, [], []

    def __getattr__(self, name):
        if name not in self.table:
            raise AttributeError(name)

        def call(*args):
            names, types = self.table[name], L.EXPORTS[name][1]
            assert len(args) == len(types) == len(names) + 1, (name, len(args))
            rec, raw = {}, {}
            for n, t, v in zip(names, types, args):
                if t is ctypes.c_void_p:
                    v = v.value if isinstance(v, ctypes.c_void_p) else v
                    rec[n], raw[n] = v is not None and v != 0, v
                else:
                    rec[n] = raw[n] = float(v) if t is ctypes.c_float else int(v)
            self.calls.append((name, rec))
            self.raw.append((name, raw))
            self.after(name, raw, rec)
            return 0
        return call

    def after(self, name, raw, rec):
        pass

    def names(self):
        return [c[0] for c in self.calls]
