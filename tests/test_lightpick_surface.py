"""Light selection by power, the part that needs no GPU: rt_tile.h declares RT_FLAG_LIGHTS_BY_POWER (bit 15, beside no other flag),
_abi.py mirrors it, the header no longer states the limit the flag lifts, and the call refuses a NULL scene before anything else.
(The declaration of rt_scene_light_table, the binding's argument list, the exports and the ABI version: tests/test_surface.py.
capacity < M needs a scene with emitters: tests/test_gpu_lightpick.py.)"""
import ctypes as C
import re

import numpy as np

from ray_tracer_s8_amd import _abi

from _surface import HEADER, check_abi_version_unchanged, check_exports


def test_header_declares_the_flag_and_the_entry_point():
    assert re.search(r"RT_FLAG_LIGHTS_BY_POWER\s*=\s*1u\s*<<\s*15\b", HEADER)
    bits = [int(b) for b in re.findall(r"RT_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", HEADER)]
    assert sorted(bits) == list(range(16))                                 # every bit once: the new flag shares none
    assert HEADER.index("RT_API int rt_scene_light_count") < HEADER.index("RT_API int rt_scene_light_table") < HEADER.index("RT_API int rt_scene_direct(")
    assert "additions only: light selection by power" in HEADER
    assert "not by power" not in HEADER                                    # the limit of both sections is gone
    assert HEADER.count("RT_FLAG_LIGHTS_BY_POWER") >= 4


def test_binding_mirrors_the_header():
    assert _abi.RT_FLAG_LIGHTS_BY_POWER == 1 << 15
    flags = {n: getattr(_abi, n) for n in dir(_abi) if n.startswith("RT_FLAG_") and n != "RT_FLAG_NONE"}
    assert sorted(flags.values()) == [1 << b for b in range(16)]
    lib = _abi.load()
    u32 = C.c_uint32
    assert lib.rt_scene_light_table.argtypes == [C.c_void_p, u32, C.POINTER(u32), C.POINTER(C.c_float), u32]
    assert lib.rt_scene_light_table.restype is C.c_int
    import ray_tracer_s8_amd as rt
    assert callable(rt.Scene.light_table)


def test_libraries_export_the_entry_point():
    check_exports(["rt_scene_light_table"])


def test_abi_version_unchanged():
    check_abi_version_unchanged()


def test_light_table_checks_its_scene_without_a_device():
    lib = _abi.load()
    wi, p = np.full(4, 7, np.uint32), np.full(4, 7, np.float32)
    args = (wi.ctypes.data_as(C.POINTER(C.c_uint32)), p.ctypes.data_as(C.POINTER(C.c_float)), 4)
    for flags in (0, _abi.RT_FLAG_LIGHTS_BY_POWER):
        assert lib.rt_scene_light_table(None, flags, *args) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_last_error()
    # zeroed memory that is no scene has no emitters: nothing is written, with or without output arrays, whatever the capacity
    dummy = (C.c_uint8 * 4096)()
    for flags in (0, _abi.RT_FLAG_LIGHTS_BY_POWER):
        assert lib.rt_scene_light_table(C.cast(dummy, C.c_void_p), flags, *args) == _abi.RT_OK
        assert lib.rt_scene_light_table(C.cast(dummy, C.c_void_p), flags, None, None, 0) == _abi.RT_OK
    assert np.all(wi == 7) and np.all(p == 7) and not any(bytes(dummy))
