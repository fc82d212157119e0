"""What the loaders of the libraries beside libhiprz.so share (query.py, order.py, bake.py): loading a library after libhiprz.so and binding
its entry points, and the handle a class of theirs owns.  As with _lib.py there is no fallback: a missing library raises."""
import ctypes as C
import os

from . import _abi, _lib
from ._lib import HiprzError

_HERE = os.path.dirname(os.path.abspath(__file__))
_loaded = {}


def lib_path(env, name):
    """the library `name` beside libhiprz.so, or wherever the environment variable `env` says"""
    return os.environ.get(env) or os.path.join(_HERE, "csrc", name)


def load(path, entry_points):
    lib = _loaded.get(path)
    if lib is None:
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
                "rayzath_amd has no CPU fallback.")
        _lib.load()  # libhiprz.so first: these libraries read contexts through its hiprz_device_view (the order also sorts through it)
        lib = C.CDLL(path)
        for name, (restype, argtypes) in entry_points.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _loaded[path] = lib
    return lib


class Handle:
    """Owns one handle of the library `lib`, made by hiprz_<kind>_create for the hiprz_ctx `ctx_ptr`; close it before the context."""

    def __init__(self, lib, kind, ctx_ptr):
        self.lib = lib
        self._handle = C.c_void_p()
        self._destroy, self._last_error = getattr(lib, f"hiprz_{kind}_destroy"), getattr(lib, f"hiprz_{kind}_last_error")
        rc = getattr(lib, f"hiprz_{kind}_create")(C.byref(self._handle), ctx_ptr)
        if rc != _abi.OK:
            raise HiprzError(rc, (self._last_error(None) or b"").decode())

    def _check(self, rc):
        if rc != _abi.OK:
            raise HiprzError(rc, (self._last_error(self._handle) or b"").decode())

    def close(self):
        if self._handle:
            self._destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
