"""Cone sampling of sphere lights, the part that needs no GPU: rt_tile.h states the contract in both sections and the limit it lifts,
the package mirrors the binding, the RT_FLAG_* set is as it was (the switch is a property of the scene, not a flag), and the calls
refuse a NULL scene and a value above RT_LIGHTS_CONE before anything else.  (RT_LIGHTS_AREA / RT_LIGHTS_CONE, the declarations of
rt_scene_set_light_sampling / rt_scene_light_sampling, the binding's argument lists, the exports and the ABI version:
tests/test_surface.py.)"""
import ctypes as C
import re

import pytest

from ray_tracer_s8_amd import _abi

from _surface import HEADER, check_abi_version_unchanged, check_exports


def test_header_declares_the_enum_and_the_entry_points():
    assert HEADER.index("RT_API int rt_scene_direct_device") < HEADER.index("RT_API int rt_scene_set_light_sampling") < \
        HEADER.index("RT_API int rt_scene_light_sampling") < HEADER.index("typedef struct rt_nee_request")
    assert "additions only: cone sampling of sphere lights" in HEADER
    assert HEADER.count("Cone sampling of sphere lights:") == 2            # the direct-lighting section and the NEE section
    assert HEADER.count("limit is lifted") >= 2 and "rt_scene_set_light_sampling must not race" in HEADER
    for phrase in ("q >= 0x1p-10f && q < 1.0f", "omc = q / (1 + ctm)", "copysignf(1, w.z)", "W = (cs * (omc + omc)) * ip", "W <= 2 * ip",
                   "ts = dc * ct - sqrt(h)", "W' = (cs' * (omc' + omc')) * ip_j", "RT_DIRECT_OCCLUDED although"):
        assert phrase in HEADER, phrase


def test_flag_set_and_abi_version_are_unchanged():
    bits = [int(b) for b in re.findall(r"RT_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", HEADER)]
    assert sorted(bits) == list(range(16))
    flags = {n: getattr(_abi, n) for n in dir(_abi) if n.startswith("RT_FLAG_") and n != "RT_FLAG_NONE"}
    assert sorted(flags.values()) == [1 << b for b in range(16)]
    check_abi_version_unchanged()


def test_binding_mirrors_the_header():
    assert (_abi.RT_LIGHTS_AREA, _abi.RT_LIGHTS_CONE) == (0, 1)
    lib = _abi.load()
    assert lib.rt_scene_set_light_sampling.argtypes == [C.c_void_p, C.c_uint32]
    assert lib.rt_scene_light_sampling.argtypes == [C.c_void_p, C.POINTER(C.c_uint32)]
    assert lib.rt_scene_set_light_sampling.restype is C.c_int and lib.rt_scene_light_sampling.restype is C.c_int
    import ray_tracer_s8_amd as rt
    assert (rt.RT_LIGHTS_AREA, rt.RT_LIGHTS_CONE) == (0, 1)
    assert callable(rt.Scene.set_light_sampling) and isinstance(rt.Scene.light_sampling, property) and rt.Scene.light_sampling.fset is None


def test_libraries_export_the_entry_points():
    check_exports(["rt_scene_set_light_sampling", "rt_scene_light_sampling"])


def test_calls_check_their_arguments_without_a_device():
    lib = _abi.load()
    out = C.c_uint32(7)
    for sampling in (_abi.RT_LIGHTS_AREA, _abi.RT_LIGHTS_CONE, 2):
        assert lib.rt_scene_set_light_sampling(None, sampling) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_last_error()
    assert lib.rt_scene_light_sampling(None, C.byref(out)) == _abi.RT_ERR_BAD_ARG and out.value == 7
    # a scene pointer that is merely non-NULL (zeroed memory that is no scene): a value above RT_LIGHTS_CONE is refused and nothing is
    # written; the default of zeroed memory reads as RT_LIGHTS_AREA; a NULL output is refused
    dummy = (C.c_uint8 * 4096)()
    h = C.cast(dummy, C.c_void_p)
    for bad in (2, 3, 0xFFFFFFFF):
        assert lib.rt_scene_set_light_sampling(h, bad) == _abi.RT_ERR_BAD_ARG
        assert b"RT_LIGHTS" in lib.rt_last_error()
    assert not any(bytes(dummy))
    assert lib.rt_scene_light_sampling(h, None) == _abi.RT_ERR_BAD_ARG
    assert lib.rt_scene_light_sampling(h, C.byref(out)) == _abi.RT_OK and out.value == _abi.RT_LIGHTS_AREA


class _Recorder:
    def __init__(self):
        self.calls = []

    def rt_scene_set_light_sampling(self, h, v):
        self.calls.append(("set", v))
        return _abi.RT_ERR_BAD_ARG if v > 1 else _abi.RT_OK

    def rt_scene_light_sampling(self, h, out):
        out._obj.value = 1
        return _abi.RT_OK

    def rt_last_error(self):
        return b"sampling is neither RT_LIGHTS_AREA nor RT_LIGHTS_CONE"


def test_python_wrapper_passes_the_value_and_raises_on_a_refusal():
    import ray_tracer_s8_amd as rt
    sc = object.__new__(rt.Scene)
    sc._lib, sc._h = _Recorder(), None
    try:
        sc.set_light_sampling(_abi.RT_LIGHTS_CONE)
        assert sc._lib.calls == [("set", 1)] and sc.light_sampling == 1
        with pytest.raises(Exception):
            sc.set_light_sampling(2)
        with pytest.raises(AttributeError):
            sc.light_sampling = 1
    finally:
        sc._h = None
