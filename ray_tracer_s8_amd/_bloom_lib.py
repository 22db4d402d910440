"""The binding of lib/librt_bloom.so, the bloom library (bloom_csrc/rt_bloom.h): a ctypes table and a lazy load().

Private to film_bloom.py: the library holds the pyramid bloom of rt.FilmBloom, is no part of the tile ABI (include/rt_tile.h, _abi.py)
or of the film, history, sampler, upsample, robust, display and JPEG libraries, and exports only rtb_* names.  Every function returns an
int status, which `check` turns into an RtbError.  This module imports without torch; the library is loaded by FilmBloom after a Film
exists, so that it binds to the HIP runtime torch and librt_s8.so use."""
from __future__ import annotations

import ctypes as C
import struct

from . import _private_lib, build as _build

RTB_VERSION = 1
RTB_OK = 0
MAX_LEVELS = 8
MODES = {"mix": 0, "add": 1}                      # RTB_MIX, RTB_ADD
FORMS = {"levels": 0, "tail": 1}                  # RTB_FORM_LEVELS, RTB_FORM_TAIL
STATUS = {1: "RTB_ERR_BAD_ARG", 2: "RTB_ERR_LIMIT", 3: "RTB_ERR_HIP", 4: "RTB_ERR_INTERNAL"}


class ApplyArgs(C.Structure):
    _fields_ = [("W", C.c_uint32), ("R", C.c_uint32), ("levels", C.c_uint32), ("mode", C.c_uint32), ("form", C.c_uint32),
                ("reserved", C.c_uint32), ("spread", C.c_float), ("strength", C.c_float), ("norm", C.c_float), ("cap", C.c_float),
                ("T", C.c_float), ("K", C.c_float), ("inp", C.c_void_p), ("out", C.c_void_p), ("out_bloom", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_uint64)]


assert C.sizeof(ApplyArgs) == 88

# name: argument types (every function returns int)
SIGNATURES = {
    "rtb_version": [C.POINTER(C.c_uint32)],
    "rtb_scratch_bytes": [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)],
    "rtb_apply": [C.POINTER(ApplyArgs), C.c_void_p],
}


def f32(v: float) -> float:
    """The f32 nearest to v."""
    return struct.unpack("f", struct.pack("f", v))[0]


def norm_of(spread: float, levels: int) -> float:
    """The `norm` of a call: the f32 nearest to 1 / (spread^0 + ... + spread^(levels - 1)), the sum taken in double from k = 0 up, of
    the f32 spread the library sees."""
    s = f32(spread)
    total, term = 0.0, 1.0
    for _ in range(levels):
        total += term
        term *= s
    return f32(1.0 / total)


def knee_of(threshold: float, knee: float) -> float:
    """The K of a call: the f32 product of the f32 threshold and the f32 knee."""
    return f32(f32(threshold) * f32(knee))


BINDING = _private_lib.Binding(_build.BLOOM, "rtb", RTB_VERSION, STATUS, SIGNATURES)
load, check, RtbError = BINDING.load, BINDING.check, BINDING.Error
