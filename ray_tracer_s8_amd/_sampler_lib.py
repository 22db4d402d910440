"""The binding of lib/librt_sampler.so, the film-sampler library (sampler_csrc/rt_sampler.h): a ctypes table and a
lazy load().

Private to film_sampler.py: the library holds the selection, compaction, gather, fold and normalisation of rt.FilmSampler, is no part
of the tile ABI (include/rt_tile.h, _abi.py), of the film library or of the history library, and exports only rts_* names.  Every
function returns an int status, which `check` turns into an RtsError.  This module imports without torch; the library is loaded by
FilmSampler after a Film exists, so that it binds to the HIP runtime torch and librt_s8.so use."""
from __future__ import annotations

import ctypes as C

from . import _private_lib, build as _build

RTS_VERSION = 1
RTS_OK = 0
STATUS = {1: "RTS_ERR_BAD_ARG", 2: "RTS_ERR_LIMIT", 3: "RTS_ERR_HIP", 4: "RTS_ERR_INTERNAL", 5: "RTS_ERR_SCRATCH"}


class SelectArgs(C.Structure):
    _fields_ = [("W", C.c_uint32), ("R", C.c_uint32), ("Hs", C.c_uint32), ("dilate", C.c_uint32), ("reserved", C.c_uint32),
                ("threshold", C.c_float), ("eps", C.c_float), ("reserved2", C.c_uint32),
                ("moments", C.c_void_p), ("counts", C.c_void_p), ("err", C.c_void_p), ("active", C.c_void_p),
                ("strip_counts", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_uint64)]


class GatherArgs(C.Structure):
    _fields_ = [("n_active", C.c_uint32), ("k", C.c_uint32), ("pixels", C.c_uint32), ("reserved", C.c_uint32),
                ("active", C.c_void_p), ("rays", C.c_void_p), ("states", C.c_void_p), ("out_rays", C.c_void_p),
                ("out_states", C.c_void_p)]


class FoldArgs(C.Structure):
    _fields_ = [("n_active", C.c_uint32), ("k", C.c_uint32), ("pixels", C.c_uint32), ("reserved", C.c_uint32),
                ("active", C.c_void_p), ("rgb", C.c_void_p), ("accum", C.c_void_p), ("moments", C.c_void_p), ("counts", C.c_void_p)]


class NormaliseArgs(C.Structure):
    _fields_ = [("W", C.c_uint32), ("R", C.c_uint32), ("e0", C.c_uint32), ("reserved", C.c_uint32),
                ("accum", C.c_void_p), ("moments", C.c_void_p), ("counts", C.c_void_p), ("out_accum", C.c_void_p),
                ("out_moments", C.c_void_p)]


assert C.sizeof(SelectArgs) == 88 and C.sizeof(GatherArgs) == 56 and C.sizeof(FoldArgs) == 56 and C.sizeof(NormaliseArgs) == 56

# name: argument types (every function returns int)
SIGNATURES = {
    "rts_version": [C.POINTER(C.c_uint32)],
    "rts_scratch_bytes": [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)],
    "rts_select": [C.POINTER(SelectArgs), C.c_void_p],
    "rts_gather": [C.POINTER(GatherArgs), C.c_void_p],
    "rts_fold": [C.POINTER(FoldArgs), C.c_void_p],
    "rts_normalise": [C.POINTER(NormaliseArgs), C.c_void_p],
}

BINDING = _private_lib.Binding(_build.PRIVATE["sampler"], "rts", RTS_VERSION, STATUS, SIGNATURES)
load, check, RtsError = BINDING.load, BINDING.check, BINDING.Error


def scratch_bytes(W: int, R: int, Hs: int) -> int:
    """rts_scratch_bytes: the bytes of rts_select's scratch.  Host arithmetic."""
    n = C.c_uint64(0)
    check("rts_scratch_bytes", load().rts_scratch_bytes(W, R, Hs, C.byref(n)))
    return n.value
