"""The binding of lib/librt_history.so, the film-history library (history_csrc/rt_history.h): a ctypes table and a
lazy load().

Private to film_history.py: the library holds the reprojection and blend of rt.FilmHistory, is no part of the tile ABI
(include/rt_tile.h, _abi.py) or of the film library, and exports only rth_* names.  Every function returns an int status, which `check`
turns into an RthError.  This module imports without torch; the library is loaded by FilmHistory after a Film exists, so that it binds
to the HIP runtime torch and librt_s8.so use."""
from __future__ import annotations

import ctypes as C

from . import _private_lib, build as _build
from ._abi import Camera, TileRequest

RTH_VERSION = 2
RTH_OK = 0
CLIP_FORM_STAGED, CLIP_FORM_DIRECT = 1, 2            # clip_form, for tests and tools; 0 is the library's choice
STATUS = {1: "RTH_ERR_BAD_ARG", 2: "RTH_ERR_LIMIT", 3: "RTH_ERR_HIP", 4: "RTH_ERR_INTERNAL"}


class State(C.Structure):
    _fields_ = [("accum", C.c_void_p), ("moments", C.c_void_p), ("length", C.c_void_p), ("depth", C.c_void_p), ("index", C.c_void_p),
                ("normal", C.c_void_p)]


class AccumulateArgs(C.Structure):
    _fields_ = [("W", C.c_uint32), ("R", C.c_uint32), ("have_prev", C.c_uint32), ("reserved", C.c_uint32),
                ("alpha", C.c_float), ("n_max", C.c_float), ("k_depth", C.c_float), ("k_normal", C.c_float),
                ("request", C.POINTER(TileRequest)), ("camera", C.POINTER(Camera)),
                ("prev_request", C.POINTER(TileRequest)), ("prev_camera", C.POINTER(Camera)),
                ("accum", C.c_void_p), ("moments", C.c_void_p), ("depth", C.c_void_p), ("hits", C.c_void_p), ("index", C.c_void_p),
                ("normal", C.c_void_p), ("prev", State), ("next", State),
                ("clip_gamma", C.c_float), ("clip_radius", C.c_uint32), ("samples", C.c_uint32), ("clip_form", C.c_uint32),
                ("clip_amount", C.c_void_p)]


assert C.sizeof(State) == 48 and C.sizeof(AccumulateArgs) == 232

# name: argument types (every function returns int)
SIGNATURES = {
    "rth_version": [C.POINTER(C.c_uint32)],
    "rth_accumulate": [C.POINTER(AccumulateArgs), C.c_void_p],
}

BINDING = _private_lib.Binding(_build.PRIVATE["history"], "rth", RTH_VERSION, STATUS, SIGNATURES)
load, check, RthError = BINDING.load, BINDING.check, BINDING.Error
