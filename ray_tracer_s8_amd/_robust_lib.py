"""The binding of lib/librt_robust.so, the robust-film library (robust_csrc/rt_robust.h): a ctypes table and a lazy
load().

Private to film_robust.py: the library holds the bucket fold and the median-of-means resolve of rt.FilmRobust, is no part of the tile
ABI (include/rt_tile.h, _abi.py) or of the film, history, sampler and upsample libraries, and exports only rtr_* names.  Every function
returns an int status, which `check` turns into an RtrError.  This module imports without torch; the library is loaded by FilmRobust
after a Film exists, so that it binds to the HIP runtime torch and librt_s8.so use."""
from __future__ import annotations

import ctypes as C

from . import _private_lib, build as _build

RTR_VERSION = 1
RTR_OK = 0
MIN_BUCKETS, MAX_BUCKETS = 3, 15
MODES = {"gini": 0, "trim": 1}                    # RTR_GINI, RTR_TRIM
STATUS = {1: "RTR_ERR_BAD_ARG", 2: "RTR_ERR_LIMIT", 3: "RTR_ERR_HIP", 4: "RTR_ERR_INTERNAL"}


class FoldArgs(C.Structure):
    _fields_ = [("pixels", C.c_uint32), ("n", C.c_uint32), ("first", C.c_uint32), ("K", C.c_uint32), ("bucket_stride", C.c_uint64),
                ("records", C.c_void_p), ("buckets", C.c_void_p)]


class ResolveArgs(C.Structure):
    _fields_ = [("W", C.c_uint32), ("R", C.c_uint32), ("K", C.c_uint32), ("samples", C.c_uint32), ("mode", C.c_uint32),
                ("c", C.c_uint32), ("buckets", C.c_void_p),
                ("out_linear", C.c_void_p), ("out_gini", C.c_void_p), ("out_kept", C.c_void_p), ("out_variance", C.c_void_p),
                ("out_accum", C.c_void_p), ("out_moments", C.c_void_p)]


assert C.sizeof(FoldArgs) == 40 and C.sizeof(ResolveArgs) == 80

# name: argument types (every function returns int)
SIGNATURES = {
    "rtr_version": [C.POINTER(C.c_uint32)],
    "rtr_fold": [C.POINTER(FoldArgs), C.c_void_p],
    "rtr_resolve": [C.POINTER(ResolveArgs), C.c_void_p],
}

BINDING = _private_lib.Binding(_build.PRIVATE["robust"], "rtr", RTR_VERSION, STATUS, SIGNATURES)
load, check, RtrError = BINDING.load, BINDING.check, BINDING.Error
