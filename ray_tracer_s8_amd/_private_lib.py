"""What the bindings of the private libraries (_film_lib.py, _history_lib.py) share: the status error and the load.

A private library is a build.Library beside the product, no part of the tile ABI (include/rt_tile.h, _abi.py): every function of it
returns an int status, and one of them, <prefix>_version(uint32_t*), reports the version its binding must match.  This module imports
without torch and loads nothing."""
from __future__ import annotations

import ctypes as C

from . import build as _build


class StatusError(RuntimeError):
    """A non-zero status of a private library's function.  A binding subclasses it with its own STATUS names."""
    STATUS: dict = {}

    def __init__(self, what: str, status: int):
        super().__init__(f"{what}: {self.STATUS.get(status, status)}")
        self.status = status


def load(library: _build.Library, signatures: dict, version: int, error: type, rebuild: str, build_if_missing: bool = True) -> C.CDLL:
    """Open the library (building it with hipcc only if the file is missing), give every function of `signatures` ({name: argument
    types}) its types, and compare the library's version with the binding's.  Raises if it cannot: there is no fall-back."""
    path = library.path
    if build_if_missing and not path.exists():
        path = _build.ensure(library)
    lib = C.CDLL(str(path))
    for name, argtypes in signatures.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, C.c_int
    name = next(n for n in signatures if n.endswith("_version"))
    v = C.c_uint32(0)
    status = getattr(lib, name)(C.byref(v))
    if status != 0:
        raise error(name, status)
    if v.value != version:
        raise RuntimeError(f"{path} is version {v.value}, this binding is version {version}: rebuild it ({rebuild})")
    return lib
