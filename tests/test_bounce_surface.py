"""Path steps of caller rays, the part that needs no GPU: rt_tile.h declares rt_scene_bounce / rt_scene_bounce_device with the argument
lists the binding uses, both libraries export them, rt_bounce is 16 bytes and rt_bounce_request 24 with the documented offsets (as
are the binding's twins), the ABI they were added to is unchanged (RT_ABI_VERSION 4), and every argument check of the contract
refuses before any device work."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np

from ray_tracer_s8_amd import _abi

from test_trace_surface import HEADER, ROOT, _declared_params, _exported, _header_struct_fields

ENTRY_POINTS = {
    "rt_scene_bounce": ["rt_scene*", "const rt_bounce_request*", "rt_ray*", "uint32_t", "uint64_t*", "const uint32_t*", "uint32_t",
                        "rt_bounce*", "rt_hit*", "uint32_t*", "uint32_t*", "rt_tile_stats*"],
    "rt_scene_bounce_device": ["rt_scene*", "const rt_bounce_request*", "void*", "uint32_t", "void*", "const void*", "const void*",
                               "void*", "void*", "void*", "void*", "void*"],
}
REQUEST_FIELDS = [("uint32_t", "flags", 0), ("uint32_t", "ray_form", 4), ("uint32_t", "seed_states", 8), ("uint32_t", "reserved", 12),
                  ("uint64_t", "seed", 16)]
BOUNCE_FIELDS = [("float", "r", 0), ("float", "g", 4), ("float", "b", 8), ("uint32_t", "status", 12)]


def test_header_declares_the_bounce_entry_points():
    for name, params in ENTRY_POINTS.items():
        assert _declared_params(name) == params, name
    assert re.search(r"RT_BOUNCE_SCATTERED\s*=\s*0u\s*,\s*RT_BOUNCE_EMITTED\s*=\s*1u\s*,\s*RT_BOUNCE_MISSED\s*=\s*2u", HEADER)
    assert HEADER.index("RT_API int rt_scene_trace_device") < HEADER.index("typedef struct rt_bounce ") < HEADER.index("typedef struct rt_aov_planes")


def test_binding_argtypes_match_the_header():
    lib = _abi.load()
    vp, u32, u32p = C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)
    assert lib.rt_scene_bounce.argtypes == [vp, C.POINTER(_abi.BounceRequest), C.POINTER(_abi.Ray), u32, C.POINTER(C.c_uint64), u32p, u32,
                                            C.POINTER(_abi.Bounce), C.POINTER(_abi.Hit), u32p, u32p, C.POINTER(_abi.TileStats)]
    assert lib.rt_scene_bounce_device.argtypes == [vp, C.POINTER(_abi.BounceRequest), vp, u32] + [vp] * 8
    assert lib.rt_scene_bounce.restype is C.c_int and lib.rt_scene_bounce_device.restype is C.c_int


def test_libraries_export_the_bounce_entry_points():
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
    assert _header_struct_fields("rt_bounce_request") == [(t, n) for t, n, _ in REQUEST_FIELDS]
    assert _header_struct_fields("rt_bounce") == [(t, n) for t, n, _ in BOUNCE_FIELDS]
    assert C.sizeof(_abi.BounceRequest) == 24 and C.sizeof(_abi.Bounce) == 16 == _abi.BOUNCE_DTYPE.itemsize
    for cls, fields in ((_abi.BounceRequest, REQUEST_FIELDS), (_abi.Bounce, BOUNCE_FIELDS)):
        assert [n for n, _ in cls._fields_] == [n for _, n, _ in fields]
        for t, n, off in fields:
            f = getattr(cls, n)
            assert f.offset == off and f.size == (8 if t == "uint64_t" else 4), n
    assert [(n, _abi.BOUNCE_DTYPE.fields[n][1]) for n in _abi.BOUNCE_DTYPE.names] == [(n, off) for _, n, off in BOUNCE_FIELDS]
    assert _abi.BOUNCE_DTYPE["status"] == np.uint32 and _abi.BOUNCE_DTYPE["r"] == np.float32
    assert (_abi.RT_BOUNCE_SCATTERED, _abi.RT_BOUNCE_EMITTED, _abi.RT_BOUNCE_MISSED) == (0, 1, 2)
    import ray_tracer_s8_amd as rt
    assert rt.BOUNCE_DTYPE is _abi.BOUNCE_DTYPE and rt.BounceRequest is _abi.BounceRequest and rt.RT_BOUNCE_MISSED == 2
    assert hasattr(rt.Scene, "bounce") and hasattr(rt.Scene, "bounce_device")


def test_header_layout_compiles_as_c():
    """sizeof and offsetof as a C compiler sees the header."""
    gcc = shutil.which("gcc")
    assert gcc
    src = ("#include <stddef.h>\n#include \"rt_tile.h\"\n"
           "_Static_assert(sizeof(rt_bounce) == 16 && offsetof(rt_bounce, g) == 4 && offsetof(rt_bounce, status) == 12, \"rt_bounce\");\n"
           "_Static_assert(sizeof(rt_bounce_request) == 24, \"rt_bounce_request\");\n"
           "_Static_assert(offsetof(rt_bounce_request, ray_form) == 4 && offsetof(rt_bounce_request, seed_states) == 8, \"a\");\n"
           "_Static_assert(offsetof(rt_bounce_request, reserved) == 12 && offsetof(rt_bounce_request, seed) == 16, \"b\");\n"
           "_Static_assert(RT_BOUNCE_SCATTERED == 0 && RT_BOUNCE_EMITTED == 1 && RT_BOUNCE_MISSED == 2, \"status\");\n"
           "_Static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 32 && sizeof(rt_tile_stats) == 64, \"abi 4\");\n")
    r = subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_abi_version_unchanged():
    assert re.search(r"#define\s+RT_ABI_VERSION\s+4u", HEADER)
    assert _abi.RT_ABI_VERSION == 4 and _abi.load().rt_abi_version() == 4


def bad_arg_calls(lib, scene):
    """Every RT_ERR_BAD_ARG case of the contract as (what, status) pairs, for a scene handle (None: the NULL scene itself is the
    error, as on a machine without a device).  Shared with tests/test_gpu_bounce.py, which passes a live scene."""
    n = 4
    rays = (_abi.Ray * n)()
    st = (C.c_uint64 * (4 * n))()
    bnc = (_abi.Bounce * n)()
    nxt = (C.c_uint32 * n)()
    cnt = C.c_uint32(7)
    act = (C.c_uint32 * n)(0, 1, 2, 3)
    bad = (C.c_uint32 * n)(0, 1, 2, n)

    def rq(**kw):
        r = _abi.BounceRequest(0, 0, 0, 0, 0)
        for k, v in kw.items():
            setattr(r, k, v)
        return C.byref(r)

    def host(req=None, scene_=scene, rays_=rays, n_=n, st_=st, act_=None, n_act=0, bnc_=bnc, nxt_=None, cnt_=None, null_req=False):
        return lib.rt_scene_bounce(scene_, None if null_req else (req or rq()), rays_, n_, st_, act_, n_act, bnc_, None, nxt_, cnt_, None)

    v = lambda a: C.cast(a if isinstance(a, C.Array) else C.pointer(a), C.c_void_p)

    def dev(req=None, scene_=scene, rays_=v(rays), n_=n, st_=v(st), act_=None, n_act=None, bnc_=v(bnc), nxt_=None, cnt_=None,
            null_req=False):
        return lib.rt_scene_bounce_device(scene_, None if null_req else (req or rq()), rays_, n_, st_, act_, n_act, bnc_, None, nxt_, cnt_,
                                          None)

    out = []
    for name, f in (("host", host), ("device", dev)):
        out += [((name, "scene"), f(scene_=None)), ((name, "request"), f(null_req=True)), ((name, "rays"), f(rays_=None)),
                ((name, "states"), f(st_=None)), ((name, "out_bounce"), f(bnc_=None)), ((name, "n == 0"), f(n_=0)),
                ((name, "ray_form"), f(req=rq(ray_form=2))), ((name, "reserved"), f(req=rq(reserved=1))),
                ((name, "seed_states"), f(req=rq(seed_states=2))),
                ((name, "next without n_next"), f(nxt_=nxt if name == "host" else v(nxt)))]
    out += [(("host", "index >= n"), host(act_=bad, n_act=n)), (("host", "n_active > n"), host(act_=act, n_act=n + 1)),
            (("device", "active without n_active"), dev(act_=v(act))), (("device", "n_active without active"), dev(n_act=v(cnt)))]
    assert cnt.value == 7 and not any(bytes(bnc)) and not any(bytes(nxt))
    return out


def test_bounce_entry_points_check_arguments_without_a_device():
    """Without a scene every call is refused for that alone.  With a scene pointer that is merely non-NULL (zeroed memory that is
    no scene: any use of it would need a device) every other case is still refused, so the checks come before any device work.
    The same cases run on the GPU with a live scene (tests/test_gpu_bounce.py, through bad_arg_calls too)."""
    lib = _abi.load()
    for what, status in bad_arg_calls(lib, None):
        assert status == _abi.RT_ERR_BAD_ARG, what
    dummy = (C.c_uint8 * 4096)()
    for what, status in bad_arg_calls(lib, C.cast(dummy, C.c_void_p)):
        assert status == _abi.RT_ERR_BAD_ARG, what
        assert lib.rt_last_error(), what
    assert not any(bytes(dummy))
