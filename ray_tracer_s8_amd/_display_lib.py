"""The binding of lib/librt_display.so, the display library (display_csrc/rt_display.h): a ctypes table and a lazy
load().

Private to film_display.py: the library holds the luminance histogram, the exposure record and the tone curves of rt.FilmDisplay, is
no part of the tile ABI (include/rt_tile.h, _abi.py) or of the film, history, sampler, upsample and robust libraries, and exports only
rtd_* names.  Every function returns an int status, which `check` turns into an RtdError.  This module imports without torch; the
library is loaded by FilmDisplay after a Film exists, so that it binds to the HIP runtime torch and librt_s8.so use."""
from __future__ import annotations

import ctypes as C

from . import _private_lib, build as _build

RTD_VERSION = 1
RTD_OK = 0
HIST_WORDS, RECORD_WORDS = 257, 8
MODES = {"auto": 0, "manual": 1}                  # RTD_AUTO, RTD_MANUAL
CURVES = {"none": 0, "reinhard": 1, "filmic": 2}  # RTD_NONE, RTD_REINHARD, RTD_FILMIC
FORMS = {"wave": 0, "match": 1}                   # RTD_HIST_WAVE, RTD_HIST_MATCH
RECORD_FIELDS = ("scale", "white", "target", "bin_key", "bin_white", "counted", "excluded", "frames")      # the first three f32
STATUS = {1: "RTD_ERR_BAD_ARG", 2: "RTD_ERR_LIMIT", 3: "RTD_ERR_HIP", 4: "RTD_ERR_INTERNAL"}


class MeterArgs(C.Structure):
    _fields_ = [("W", C.c_uint32), ("R", C.c_uint32), ("form", C.c_uint32), ("reserved", C.c_uint32),
                ("linear", C.c_void_p), ("hist", C.c_void_p)]


class ExposeArgs(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("key", C.c_float), ("key_q16", C.c_uint32), ("white_q16", C.c_uint32), ("rate", C.c_float),
                ("scale_min", C.c_float), ("scale_max", C.c_float), ("scale", C.c_float), ("white", C.c_float),
                ("reserved", C.c_uint32), ("hist", C.c_void_p), ("record", C.c_void_p)]


class ApplyArgs(C.Structure):
    _fields_ = [("W", C.c_uint32), ("R", C.c_uint32), ("curve", C.c_uint32), ("dither", C.c_uint32),
                ("linear", C.c_void_p), ("record", C.c_void_p), ("out_f32", C.c_void_p), ("out_rgb", C.c_void_p)]


assert C.sizeof(MeterArgs) == 32 and C.sizeof(ExposeArgs) == 56 and C.sizeof(ApplyArgs) == 48

# name: argument types (every function returns int)
SIGNATURES = {
    "rtd_version": [C.POINTER(C.c_uint32)],
    "rtd_meter": [C.POINTER(MeterArgs), C.c_void_p],
    "rtd_expose": [C.POINTER(ExposeArgs), C.c_void_p],
    "rtd_apply": [C.POINTER(ApplyArgs), C.c_void_p],
}

BINDING = _private_lib.Binding(_build.PRIVATE["display"], "rtd", RTD_VERSION, STATUS, SIGNATURES)
load, check, RtdError = BINDING.load, BINDING.check, BINDING.Error
