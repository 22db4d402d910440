"""The binding of lib/librt_upsample.so, the film-upsampler library (upsample_csrc/rt_upsample.h): a ctypes table and a
lazy load().

Private to film_upsampler.py: the library holds the joint-bilateral upsampling kernel of rt.FilmUpsampler, is no part of the tile ABI
(include/rt_tile.h, _abi.py) or of the film, history and sampler libraries, and exports only rtu_* names.  Every function returns an
int status, which `check` turns into an RtuError.  This module imports without torch; the library is loaded by FilmUpsampler after a
Film exists, so that it binds to the HIP runtime torch and librt_s8.so use."""
from __future__ import annotations

import ctypes as C

from . import _private_lib, build as _build

RTU_VERSION = 1
RTU_OK = 0
MIN_SCALE, MAX_SCALE = 2, 4
STATUS = {1: "RTU_ERR_BAD_ARG", 2: "RTU_ERR_LIMIT", 3: "RTU_ERR_HIP", 4: "RTU_ERR_INTERNAL"}
PLANES = ("albedo", "normal", "depth", "hits", "index")           # the fields of rtu_planes, in its order


class Planes(C.Structure):
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("hits", C.c_void_p), ("index", C.c_void_p),
                ("samples", C.c_uint32), ("reserved", C.c_uint32)]


class UpsampleArgs(C.Structure):
    _fields_ = [("Wl", C.c_uint32), ("Rl", C.c_uint32), ("Hl", C.c_uint32), ("y0l", C.c_uint32),
                ("Wh", C.c_uint32), ("Rh", C.c_uint32), ("Hh", C.c_uint32), ("y0h", C.c_uint32),
                ("scale", C.c_uint32), ("form", C.c_uint32), ("k_depth", C.c_float), ("k_normal", C.c_float),
                ("eps", C.c_float), ("reserved", C.c_uint32),
                ("linear", C.c_void_p), ("lo", Planes), ("hi", Planes),
                ("out_linear", C.c_void_p), ("out_f32", C.c_void_p), ("out_rgb", C.c_void_p), ("out_class", C.c_void_p)]


assert C.sizeof(Planes) == 48 and C.sizeof(UpsampleArgs) == 192

# name: argument types (every function returns int)
SIGNATURES = {
    "rtu_version": [C.POINTER(C.c_uint32)],
    "rtu_upsample": [C.POINTER(UpsampleArgs), C.c_void_p],
}

BINDING = _private_lib.Binding(_build.PRIVATE["upsample"], "rtu", RTU_VERSION, STATUS, SIGNATURES)
load, check, RtuError = BINDING.load, BINDING.check, BINDING.Error
