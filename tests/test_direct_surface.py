"""Direct lighting of caller rays, the part that needs no GPU: rt_tile.h declares rt_scene_light_count / rt_scene_direct /
rt_scene_direct_device with the argument lists the binding uses, both libraries export them, rt_direct_request is 16 bytes and
rt_direct 32 with the documented offsets (as are the binding's twins), the ABI they were added to is unchanged (RT_ABI_VERSION 4),
every argument check of the contract refuses before any device work, and Scene.direct checks its arguments before it calls.  (The
limit of 2^23 emitters is the plan's: tests/test_direct_host.py.)"""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

from ray_tracer_s8_amd import _abi

from test_trace_surface import HEADER, ROOT, _declared_params, _exported, _header_struct_fields

ENTRY_POINTS = {
    "rt_scene_light_count": ["rt_scene*", "uint32_t*"],
    "rt_scene_direct": ["rt_scene*", "const rt_direct_request*", "const rt_hit*", "uint32_t", "uint64_t*", "const uint32_t*", "uint32_t",
                        "rt_direct*", "rt_tile_stats*"],
    "rt_scene_direct_device": ["rt_scene*", "const rt_direct_request*", "const void*", "uint32_t", "void*", "const void*", "const void*",
                               "void*", "void*"],
}
REQUEST_FIELDS = [("uint32_t", "flags", 0), ("uint32_t", "reserved", 4), ("float", "t_min", 8), ("float", "t_max", 12)]
DIRECT_FIELDS = [("float", "r", 0), ("float", "g", 4), ("float", "b", 8), ("uint32_t", "light", 12), ("float", "lx", 16),
                 ("float", "ly", 20), ("float", "lz", 24), ("uint32_t", "status", 28)]
STATUSES = ("LIT", "OCCLUDED", "FACING_AWAY", "NO_LIGHTS", "SKIPPED")


def test_header_declares_the_direct_entry_points():
    for name, params in ENTRY_POINTS.items():
        assert _declared_params(name) == params, name
    assert re.search(r"\s*,\s*".join(rf"RT_DIRECT_{s}\s*=\s*{k}u" for k, s in enumerate(STATUSES)), HEADER)
    assert HEADER.index("RT_API int rt_scene_bounce_device") < HEADER.index("typedef struct rt_direct_request") < HEADER.index("typedef struct rt_aov_planes")
    assert "additions only: direct lighting" in HEADER


def test_binding_argtypes_match_the_header():
    lib = _abi.load()
    vp, u32, u32p = C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)
    assert lib.rt_scene_light_count.argtypes == [vp, u32p]
    assert lib.rt_scene_direct.argtypes == [vp, C.POINTER(_abi.DirectRequest), C.POINTER(_abi.Hit), u32, C.POINTER(C.c_uint64), u32p, u32,
                                            C.POINTER(_abi.Direct), C.POINTER(_abi.TileStats)]
    assert lib.rt_scene_direct_device.argtypes == [vp, C.POINTER(_abi.DirectRequest), vp, u32] + [vp] * 5
    assert all(getattr(lib, n).restype is C.c_int for n in ENTRY_POINTS)


def test_libraries_export_the_direct_entry_points():
    from ray_tracer_s8_amd import build
    _abi.load()
    _abi.load_debug()
    for path in (build.LIB_PATH, build.DEBUG_LIB_PATH):
        exported = _exported(path)
        for name in ENTRY_POINTS:
            assert name in exported, (path, name)
    declared = set(re.findall(r"RT_API\s+[\w\s\*]*?\b(rt_\w+)\s*\(", HEADER))
    assert {s for s in _exported(build.LIB_PATH) if s.startswith("rt_")} == declared


def test_struct_layouts():
    assert _header_struct_fields("rt_direct_request") == [(t, n) for t, n, _ in REQUEST_FIELDS]
    assert _header_struct_fields("rt_direct") == [(t, n) for t, n, _ in DIRECT_FIELDS]
    assert C.sizeof(_abi.DirectRequest) == 16 and C.sizeof(_abi.Direct) == 32 == _abi.DIRECT_DTYPE.itemsize
    for cls, fields in ((_abi.DirectRequest, REQUEST_FIELDS), (_abi.Direct, DIRECT_FIELDS)):
        assert [n for n, _ in cls._fields_] == [n for _, n, _ in fields]
        for t, n, off in fields:
            f = getattr(cls, n)
            assert f.offset == off and f.size == 4, n
    assert [(n, _abi.DIRECT_DTYPE.fields[n][1]) for n in _abi.DIRECT_DTYPE.names] == [(n, off) for _, n, off in DIRECT_FIELDS]
    for t, n, _ in DIRECT_FIELDS:
        assert _abi.DIRECT_DTYPE[n] == (np.uint32 if t == "uint32_t" else np.float32), n
    assert tuple(getattr(_abi, f"RT_DIRECT_{s}") for s in STATUSES) == (0, 1, 2, 3, 4)
    import ray_tracer_s8_amd as rt
    assert rt.DIRECT_DTYPE is _abi.DIRECT_DTYPE and rt.DirectRequest is _abi.DirectRequest
    assert hasattr(rt.Scene, "direct") and hasattr(rt.Scene, "direct_device") and isinstance(rt.Scene.n_lights, property)


def test_header_layout_compiles_as_c():
    """sizeof and offsetof as a C compiler sees the header."""
    gcc = shutil.which("gcc")
    assert gcc
    src = ("#include <stddef.h>\n#include \"rt_tile.h\"\n"
           "_Static_assert(sizeof(rt_direct) == 32 && offsetof(rt_direct, light) == 12 && offsetof(rt_direct, lx) == 16, \"rt_direct\");\n"
           "_Static_assert(offsetof(rt_direct, status) == 28, \"rt_direct.status\");\n"
           "_Static_assert(sizeof(rt_direct_request) == 16 && offsetof(rt_direct_request, reserved) == 4, \"rt_direct_request\");\n"
           "_Static_assert(offsetof(rt_direct_request, t_min) == 8 && offsetof(rt_direct_request, t_max) == 12, \"window\");\n"
           "_Static_assert(RT_DIRECT_LIT == 0 && RT_DIRECT_OCCLUDED == 1 && RT_DIRECT_FACING_AWAY == 2, \"status\");\n"
           "_Static_assert(RT_DIRECT_NO_LIGHTS == 3 && RT_DIRECT_SKIPPED == 4, \"status\");\n"
           "_Static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 32 && sizeof(rt_tile_stats) == 64 && sizeof(rt_bounce) == 16, \"abi 4\");\n")
    r = subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_abi_version_unchanged():
    assert re.search(r"#define\s+RT_ABI_VERSION\s+4u", HEADER)
    assert _abi.RT_ABI_VERSION == 4 and _abi.load().rt_abi_version() == 4


def bad_arg_calls(lib, scene):
    """Every RT_ERR_BAD_ARG case of the contract as (what, status) pairs, for a scene handle (None: the NULL scene itself is the
    error, as on a machine without a device).  Shared with tests/test_gpu_direct.py, which passes a live scene."""
    n = 4
    hits = (_abi.Hit * n)()
    st = (C.c_uint64 * (4 * n))()
    out_ = (_abi.Direct * n)()
    cnt = C.c_uint32(7)
    act = (C.c_uint32 * n)(0, 1, 2, 3)
    bad = (C.c_uint32 * n)(0, 1, 2, n)

    def rq(**kw):
        r = _abi.DirectRequest(0, 0, 0.001, 1000.0)
        for k, v in kw.items():
            setattr(r, k, v)
        return C.byref(r)

    def host(req=None, scene_=scene, hits_=hits, n_=n, st_=st, act_=None, n_act=0, o_=out_, null_req=False):
        return lib.rt_scene_direct(scene_, None if null_req else (req or rq()), hits_, n_, st_, act_, n_act, o_, None)

    v = lambda a: C.cast(a if isinstance(a, C.Array) else C.pointer(a), C.c_void_p)

    def dev(req=None, scene_=scene, hits_=v(hits), n_=n, st_=v(st), act_=None, n_act=None, o_=v(out_), null_req=False):
        return lib.rt_scene_direct_device(scene_, None if null_req else (req or rq()), hits_, n_, st_, act_, n_act, o_, None)

    out = []
    for name, f in (("host", host), ("device", dev)):
        out += [((name, "scene"), f(scene_=None)), ((name, "request"), f(null_req=True)), ((name, "hits"), f(hits_=None)),
                ((name, "states"), f(st_=None)), ((name, "out"), f(o_=None)), ((name, "n == 0"), f(n_=0)),
                ((name, "reserved"), f(req=rq(reserved=1)))]
    out += [(("host", "index >= n"), host(act_=bad, n_act=n)), (("host", "n_active > n"), host(act_=act, n_act=n + 1)),
            (("host", "n_active without active"), host(n_act=2)),
            (("device", "active without n_active"), dev(act_=v(act))), (("device", "n_active without active"), dev(n_act=v(cnt)))]
    m = C.c_uint32(9)
    out += [(("count", "scene"), lib.rt_scene_light_count(None, C.byref(m))), (("count", "out"), lib.rt_scene_light_count(scene, None))]
    assert cnt.value == 7 and m.value == 9 and not any(bytes(out_)) and not any(bytes(st))
    return out


def test_direct_entry_points_check_arguments_without_a_device():
    """Without a scene every call is refused for that alone.  With a scene pointer that is merely non-NULL (zeroed memory that is
    no scene: any use of it would need a device) every other case is still refused, so the checks come before any device work.
    The same cases run on the GPU with a live scene (tests/test_gpu_direct.py, through bad_arg_calls too)."""
    lib = _abi.load()
    for what, status in bad_arg_calls(lib, None):
        assert status == _abi.RT_ERR_BAD_ARG, what
    dummy = (C.c_uint8 * 4096)()
    for what, status in bad_arg_calls(lib, C.cast(dummy, C.c_void_p)):
        assert status == _abi.RT_ERR_BAD_ARG, what
        assert lib.rt_last_error(), what
    assert not any(bytes(dummy))
    # the light count of a scene is a host-side value: zeroed memory has none
    m = C.c_uint32(9)
    assert lib.rt_scene_light_count(C.cast(dummy, C.c_void_p), C.byref(m)) == _abi.RT_OK and m.value == 0


class _NoLibrary:
    """Stands in for the library behind a Scene: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


def test_python_argument_handling():
    """Scene.direct refuses malformed arrays itself, before the library is called."""
    import ray_tracer_s8_amd as rt
    sc = object.__new__(rt.Scene)
    sc._lib, sc._h = _NoLibrary(), None
    hits = np.zeros(5, _abi.HIT_DTYPE)
    states = np.ones((5, 4), np.uint64)
    try:
        with pytest.raises(ValueError):
            sc.direct(hits.reshape(5, 1), states)
        with pytest.raises(ValueError):
            sc.direct(hits, None)
        with pytest.raises(ValueError):
            sc.direct(hits, states[:-1])
        with pytest.raises(ValueError):
            sc.direct(hits, states.reshape(4, 5))
        with pytest.raises(AssertionError):                                # well-formed arguments do reach the library
            sc.direct(hits, states, active=[0, 2])
    finally:
        sc._h = None                                                       # (nothing for close() to destroy)
