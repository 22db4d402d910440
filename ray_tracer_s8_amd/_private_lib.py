"""What the bindings of the private libraries (_film_lib.py, _history_lib.py, _sampler_lib.py, _upsample_lib.py, _robust_lib.py,
_display_lib.py, and _jpeg_lib.py and _bloom_lib.py, whose libraries build.JPEG and build.BLOOM are held beside build.PRIVATE) share: one Binding each, which owns the status error, the check and the lazy load.

A private library is a member of build.PRIVATE beside the product, no part of the tile ABI (include/rt_tile.h, _abi.py): every
function of it returns an int status, and one of them, <prefix>_version(uint32_t*), reports the version its binding must match.  This
module imports without torch and loads nothing."""
from __future__ import annotations

import ctypes as C

from . import build as _build


class StatusError(RuntimeError):
    """A non-zero status of a private library's function.  A Binding subclasses it with its own STATUS names."""
    STATUS: dict = {}

    def __init__(self, what: str, status: int):
        super().__init__(f"{what}: {self.STATUS.get(status, status)}")
        self.status = status


class Binding:
    """The binding of one private library: `signatures` ({name: argument types}, every function returning int) over `library`,
    whose exports all begin with `prefix` ("rtf") and whose <prefix>_version must report `version`.  Nothing is loaded before the
    first load()."""

    def __init__(self, library: _build.Library, prefix: str, version: int, status: dict, signatures: dict):
        self.library, self.prefix, self.version, self.signatures = library, prefix, version, signatures
        self.Error = type(f"{prefix.capitalize()}Error", (StatusError,), {"STATUS": status})
        self._lib = None

    @property
    def loaded(self) -> bool:
        return self._lib is not None

    def check(self, what: str, status: int) -> None:
        if status != 0:
            raise self.Error(what, status)

    def load(self, build_if_missing: bool = True) -> C.CDLL:
        """Open the library (building it with hipcc only if the file is missing), give every function its types, and compare the
        library's version with the binding's.  Raises if it cannot: there is no fall-back."""
        if self._lib is None:
            path = self.library.path
            if build_if_missing and not path.exists():
                path = _build.ensure(self.library)
            lib = C.CDLL(str(path))
            for name, argtypes in self.signatures.items():
                fn = getattr(lib, name)
                fn.argtypes, fn.restype = argtypes, C.c_int
            name = f"{self.prefix}_version"
            v = C.c_uint32(0)
            self.check(name, getattr(lib, name)(C.byref(v)))
            if v.value != self.version:
                key = self.library.src_dir.name.removesuffix("_csrc")
                raise RuntimeError(f"{path} is version {v.value}, this binding is version {self.version}: rebuild it "
                                   f"(build.ensure(build.{key.upper()}, force=True))")
            self._lib = lib
        return self._lib
