"""The binding of lib/librt_film.so, the film library (film_csrc/rt_film.h): a ctypes table and a lazy load().

Private to film.py: the library holds the moments fold, the variance-guided resolve and the regression resolve of rt.Film, is no part of the tile ABI
(include/rt_tile.h, _abi.py) and exports only rtf_* names.  Every function returns an int status, which `check` turns into an
RtfError.  This module imports without torch; the library is loaded by Film after _abi.check_single_hip_runtime(), so that it binds
to the HIP runtime torch and librt_s8.so use."""
from __future__ import annotations

import ctypes as C

from . import _private_lib, build as _build

RTF_VERSION = 2
RTF_OK = 0
STATUS = {1: "RTF_ERR_BAD_ARG", 2: "RTF_ERR_LIMIT", 3: "RTF_ERR_SCRATCH", 4: "RTF_ERR_HIP", 5: "RTF_ERR_INTERNAL"}
MAX_ITERATIONS = 8
LDS_PLAN = 0xFFFFFFFF                 # lds_max_step: the plan's own choice
RESOLVE_ATROUS, RESOLVE_REGRESS = 0, 1         # rtf_resolve_args.kind
REGRESS_RECORD = 32                   # the floats of a node's record in `model`


class ResolveArgs(C.Structure):
    _fields_ = [("W", C.c_uint32), ("R", C.c_uint32), ("samples", C.c_uint32), ("iterations", C.c_uint32),
                ("lds_max_step", C.c_uint32), ("kind", C.c_uint32),
                ("sigma_l", C.c_float), ("var_eps", C.c_float), ("k_normal", C.c_float), ("k_depth", C.c_float),
                ("accum", C.c_void_p), ("moments", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("hits", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_uint64),
                ("out_rgb", C.c_void_p), ("out_f32", C.c_void_p), ("out_linear", C.c_void_p), ("out_variance", C.c_void_p),
                ("albedo", C.c_void_p), ("aov_samples", C.c_uint32), ("albedo_eps", C.c_float), ("ridge", C.c_float),
                ("reserved", C.c_uint32), ("model", C.c_void_p), ("model_bytes", C.c_uint64)]


# name: argument types (every function returns int)
SIGNATURES = {
    "rtf_version": [C.POINTER(C.c_uint32)],
    "rtf_fold_moments": [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p],
    "rtf_resolve_scratch_bytes": [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)],
    "rtf_resolve": [C.POINTER(ResolveArgs), C.c_void_p],
}

BINDING = _private_lib.Binding(_build.PRIVATE["film"], "rtf", RTF_VERSION, STATUS, SIGNATURES)
load, check, RtfError = BINDING.load, BINDING.check, BINDING.Error


def resolve_scratch_bytes(width: int, rows: int) -> int:
    b = C.c_uint64(0)
    check("rtf_resolve_scratch_bytes", load().rtf_resolve_scratch_bytes(width, rows, C.byref(b)))
    return b.value
