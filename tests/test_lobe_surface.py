"""Light samples at glossy hits, the part that needs no GPU: a C99 client of the two calls compiles against rt_tile.h, the header states
the contract in the next-event-estimation section, the package mirrors the binding, the RT_FLAG_* set and rt_nee_request's documented
size are as they were (the switch is a property of the scene), and the calls refuse a NULL scene and a value above RT_GLOSSY_MIS
before anything else.  (RT_GLOSSY_BOUNCE / RT_GLOSSY_MIS, the declarations of rt_scene_set_glossy_sampling /
rt_scene_glossy_sampling, the binding's argument lists, the exports and the ABI version: tests/test_surface.py.)"""
import ctypes as C
import re
import shutil
import subprocess

import pytest

from ray_tracer_s8_amd import _abi

from _surface import HEADER, ROOT, check_abi_version_unchanged, check_exports


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "rt_tile.h"\n'
                   "int use(rt_scene* s) { uint32_t v = RT_GLOSSY_BOUNCE; int rc = rt_scene_set_glossy_sampling(s, RT_GLOSSY_MIS);\n"
                   "  return rc ? rc : rt_scene_glossy_sampling(s, &v); }\n")
    r = subprocess.run([shutil.which("gcc"), "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", "-c", str(src), "-o",
                        str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_declares_the_enum_and_the_entry_points():
    assert HEADER.index("RT_API int rt_scene_trace_nee_device") < HEADER.index("RT_API int rt_scene_set_glossy_sampling") < \
        HEADER.index("RT_API int rt_scene_glossy_sampling")
    assert "additions only: light samples at glossy hits" in HEADER
    assert HEADER.count("Light samples at glossy hits:") == 1 and "rt_scene_set_glossy_sampling must not race" in HEADER
    for phrase in ("0 < rho && rho < 1 && gn >= 0", "kappa = rho * (rho * gg + (r + r) * gn)", "D = b * b - kappa", "b > 0 && D > 0",
                   "cg = (b * b + D) / ((r + r) * sqrt(D))", "!(W < inf)", "((cg * cl) * ((4 * (r_l*r_l)) * ip)) / d2",
                   "((cg * cl) * (A * ip)) / (PI * d2)", "(cg * (omc + omc)) * ip", "W' = inf gives wb = 1", "Rim:", "m = r * (c.us + r)", "t = sqrt(kappa + (m + m))",
                   "cgb = ((kappa + m) * (kappa + m) + m * m) / (((r + r) * |m|) * t)", "iff cgb > 0",
                   "advances the RNG by the light sample's draws"):
        assert phrase in HEADER, phrase


def test_flag_set_request_and_abi_version_are_unchanged():
    bits = [int(b) for b in re.findall(r"RT_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", HEADER)]
    assert sorted(bits) == list(range(16))
    check_abi_version_unchanged()
    assert C.sizeof(_abi.NeeRequest) == 32 and re.search(r"\}\s*rt_nee_request;\s*/\* 32 bytes \*/", HEADER)
    assert re.search(r"enum\s*\{\s*RT_NEE_LIGHT_ONLY\s*=\s*0u\s*,\s*RT_NEE_MIS\s*=\s*1u\s*\}", HEADER)


def test_binding_mirrors_the_header():
    assert (_abi.RT_GLOSSY_BOUNCE, _abi.RT_GLOSSY_MIS) == (0, 1)
    lib = _abi.load()
    assert lib.rt_scene_set_glossy_sampling.argtypes == [C.c_void_p, C.c_uint32]
    assert lib.rt_scene_glossy_sampling.argtypes == [C.c_void_p, C.POINTER(C.c_uint32)]
    assert lib.rt_scene_set_glossy_sampling.restype is C.c_int and lib.rt_scene_glossy_sampling.restype is C.c_int
    import ray_tracer_s8_amd as rt
    assert (rt.RT_GLOSSY_BOUNCE, rt.RT_GLOSSY_MIS) == (0, 1)
    assert {"RT_GLOSSY_BOUNCE", "RT_GLOSSY_MIS"} <= set(rt.__all__)
    assert callable(rt.Scene.set_glossy_sampling) and isinstance(rt.Scene.glossy_sampling, property) and rt.Scene.glossy_sampling.fset is None


def test_libraries_export_the_entry_points():
    check_exports(["rt_scene_set_glossy_sampling", "rt_scene_glossy_sampling"])


def test_calls_check_their_arguments_without_a_device():
    lib = _abi.load()
    out = C.c_uint32(7)
    for sampling in (_abi.RT_GLOSSY_BOUNCE, _abi.RT_GLOSSY_MIS, 2):
        assert lib.rt_scene_set_glossy_sampling(None, sampling) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_last_error()
    assert lib.rt_scene_glossy_sampling(None, C.byref(out)) == _abi.RT_ERR_BAD_ARG and out.value == 7
    # a scene pointer that is merely non-NULL (zeroed memory that is no scene): a value above RT_GLOSSY_MIS is refused and nothing is
    # written; the default of zeroed memory reads as RT_GLOSSY_BOUNCE; a NULL output is refused
    dummy = (C.c_uint8 * 4096)()
    h = C.cast(dummy, C.c_void_p)
    for bad in (2, 3, 0xFFFFFFFF):
        assert lib.rt_scene_set_glossy_sampling(h, bad) == _abi.RT_ERR_BAD_ARG
        assert b"RT_GLOSSY" in lib.rt_last_error()
    assert not any(bytes(dummy))
    assert lib.rt_scene_glossy_sampling(h, None) == _abi.RT_ERR_BAD_ARG
    assert lib.rt_scene_glossy_sampling(h, C.byref(out)) == _abi.RT_OK and out.value == _abi.RT_GLOSSY_BOUNCE
    assert lib.rt_scene_light_sampling(h, C.byref(out)) == _abi.RT_OK and out.value == _abi.RT_LIGHTS_AREA   # its own field


class _Recorder:
    def __init__(self):
        self.calls = []

    def rt_scene_set_glossy_sampling(self, h, v):
        self.calls.append(("set", v))
        return _abi.RT_ERR_BAD_ARG if v > 1 else _abi.RT_OK

    def rt_scene_glossy_sampling(self, h, out):
        out._obj.value = 1
        return _abi.RT_OK

    def rt_last_error(self):
        return b"sampling is neither RT_GLOSSY_BOUNCE nor RT_GLOSSY_MIS"


def test_python_wrapper_passes_the_value_and_raises_on_a_refusal():
    import ray_tracer_s8_amd as rt
    sc = object.__new__(rt.Scene)
    sc._lib, sc._h = _Recorder(), None
    try:
        sc.set_glossy_sampling(_abi.RT_GLOSSY_MIS)
        assert sc._lib.calls == [("set", 1)] and sc.glossy_sampling == 1
        with pytest.raises(rt.RtError):
            sc.set_glossy_sampling(2)
        assert sc._lib.calls[-1] == ("set", 2)
        with pytest.raises(AttributeError):
            sc.glossy_sampling = 1
    finally:
        sc._h = None
