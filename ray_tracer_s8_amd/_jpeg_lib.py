"""The binding of lib/librt_jpeg.so, the JPEG library (jpeg_csrc/rt_jpeg.h): a ctypes table and a lazy load().

Private to frame_encoder.py: the library holds the baseline JPEG encoder of rt.FrameEncoder, is no part of the tile ABI
(include/rt_tile.h, _abi.py) or of the film, history, sampler, upsample, robust and display libraries, and exports only rtj_* names.
Every function returns an int status, which `check` turns into an RtjError.  This module imports without torch; the library is loaded
by FrameEncoder after a Film exists, so that it binds to the HIP runtime torch and librt_s8.so use."""
from __future__ import annotations

import ctypes as C

from . import _private_lib, build as _build

RTJ_VERSION = 1
RTJ_OK = 0
HEADER_LEN, RECORD_WORDS, MAX_INTERVAL, MAX_SIDE = 629, 8, 65535, 65535
RECORD_FIELDS = ("total", "raw", "stuffed", "intervals", "overflow")           # the first five words; the others are zero
STATUS = {1: "RTJ_ERR_BAD_ARG", 2: "RTJ_ERR_LIMIT", 3: "RTJ_ERR_HIP", 4: "RTJ_ERR_INTERNAL"}


class EncodeArgs(C.Structure):
    _fields_ = [("W", C.c_uint32), ("R", C.c_uint32), ("quality", C.c_uint32), ("interval", C.c_uint32),
                ("tables", C.c_void_p), ("rgb", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_uint64),
                ("out", C.c_void_p), ("capacity", C.c_uint64), ("header_len", C.c_uint32), ("reserved", C.c_uint32),
                ("record", C.c_void_p)]


assert C.sizeof(EncodeArgs) == 80

# name: argument types (every function returns int)
SIGNATURES = {
    "rtj_version": [C.POINTER(C.c_uint32)],
    "rtj_header": [C.POINTER(EncodeArgs), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)],
    "rtj_bound": [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)],
    "rtj_scratch_bytes": [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)],
    "rtj_encode": [C.POINTER(EncodeArgs), C.c_void_p],
}

BINDING = _private_lib.Binding(_build.JPEG, "rtj", RTJ_VERSION, STATUS, SIGNATURES)
load, check, RtjError = BINDING.load, BINDING.check, BINDING.Error
