"""Path tracing of caller rays, the part that needs no GPU: rt_tile.h declares rt_scene_trace / rt_scene_trace_device with the
argument lists the binding uses, both libraries export them (and the product library still exports exactly what the header
declares), rt_trace_request is 24 bytes with the documented offsets (as is the binding's TraceRequest), the ABI it was added to is
unchanged (RT_ABI_VERSION 4), and the argument checks refuse before any device work."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

from ray_tracer_s8_amd import _abi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "rt_tile.h").read_text()

TRACE_ENTRY_POINTS = {
    "rt_scene_trace": ["rt_scene*", "const rt_trace_request*", "const rt_ray*", "uint32_t", "uint64_t*", "float*", "uint32_t*",
                       "rt_tile_stats*"],
    "rt_scene_trace_device": ["rt_scene*", "const rt_trace_request*", "const void*", "uint32_t", "void*", "void*", "void*", "void*"],
}
REQUEST_FIELDS = [("uint32_t", "spp", 0), ("uint32_t", "max_bounces", 4), ("uint64_t", "seed", 8), ("uint32_t", "flags", 16),
                  ("uint32_t", "ray_form", 20)]


def _declared_params(name):
    m = re.search(r"RT_API\s+int\s+" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in rt_tile.h"
    types = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        t = re.sub(r"\s*\b\w+$", "", arg)
        types.append(re.sub(r"\s*\*", "*", t))
    return types


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def _header_struct_fields(name):
    m = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", HEADER, re.S)
    assert m, f"{name} is not defined in rt_tile.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(typ, n.strip()) for n in names.split(",")]
    return fields


def test_header_declares_the_trace_entry_points():
    for name, params in TRACE_ENTRY_POINTS.items():
        assert _declared_params(name) == params, name
    assert re.search(r"RT_TRACE_RAY_NEW\s*=\s*0u\s*,\s*RT_TRACE_RAY_AS_GIVEN\s*=\s*1u", HEADER)


def test_binding_argtypes_match_the_header():
    lib = _abi.load()
    vp, u32 = C.c_void_p, C.c_uint32
    assert lib.rt_scene_trace.argtypes == [vp, C.POINTER(_abi.TraceRequest), C.POINTER(_abi.Ray), u32, C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(_abi.TileStats)]
    assert lib.rt_scene_trace.restype is C.c_int
    assert lib.rt_scene_trace_device.argtypes == [vp, C.POINTER(_abi.TraceRequest), vp, u32, vp, vp, vp, vp]
    assert lib.rt_scene_trace_device.restype is C.c_int


def test_libraries_export_the_trace_entry_points_and_the_product_exactly_the_header():
    from ray_tracer_s8_amd import build
    _abi.load()
    _abi.load_debug()
    for path in (build.LIB_PATH, build.DEBUG_LIB_PATH):
        exported = _exported(path)
        for name in TRACE_ENTRY_POINTS:
            assert name in exported, (path, name)
    declared = set(re.findall(r"RT_API\s+[\w\s\*]*?\b(rt_\w+)\s*\(", HEADER))
    product = {s for s in _exported(build.LIB_PATH) if s.startswith("rt_")}
    assert product == declared, (product ^ declared)


def test_trace_request_layout():
    assert _header_struct_fields("rt_trace_request") == [(t, n) for t, n, _ in REQUEST_FIELDS]
    assert C.sizeof(_abi.TraceRequest) == 24
    for t, n, off in REQUEST_FIELDS:
        f = getattr(_abi.TraceRequest, n)
        assert f.offset == off and f.size == (8 if t == "uint64_t" else 4), n
    assert [n for n, _ in _abi.TraceRequest._fields_] == [n for _, n, _ in REQUEST_FIELDS]
    assert (_abi.RT_TRACE_RAY_NEW, _abi.RT_TRACE_RAY_AS_GIVEN) == (0, 1)


def test_header_layout_compiles_as_c():
    """sizeof and offsetof as a C compiler sees the header."""
    gcc = shutil.which("gcc")
    assert gcc
    src = ("#include <stddef.h>\n#include \"rt_tile.h\"\n"
           "_Static_assert(sizeof(rt_trace_request) == 24, \"rt_trace_request\");\n"
           "_Static_assert(offsetof(rt_trace_request, max_bounces) == 4 && offsetof(rt_trace_request, seed) == 8, \"a\");\n"
           "_Static_assert(offsetof(rt_trace_request, flags) == 16 && offsetof(rt_trace_request, ray_form) == 20, \"b\");\n"
           "_Static_assert(RT_TRACE_RAY_NEW == 0 && RT_TRACE_RAY_AS_GIVEN == 1, \"forms\");\n"
           "_Static_assert(sizeof(rt_ray) == 32 && sizeof(rt_tile_stats) == 64, \"abi 4\");\n")
    r = subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_abi_version_unchanged():
    assert re.search(r"#define\s+RT_ABI_VERSION\s+4u", HEADER)
    assert _abi.RT_ABI_VERSION == 4 and _abi.load().rt_abi_version() == 4


def test_trace_entry_points_check_arguments_without_a_device():
    """No scene: refused before anything else is looked at (the same checks come first on the GPU: test_gpu_trace.py)."""
    lib = _abi.load()
    rq = _abi.TraceRequest(1, 10, 0, 0, 0)
    rays = (_abi.Ray * 2)()
    rgb = (C.c_float * 6)()
    assert lib.rt_scene_trace(None, C.byref(rq), rays, 2, None, rgb, None, None) == _abi.RT_ERR_BAD_ARG
    assert lib.rt_scene_trace_device(None, C.byref(rq), C.cast(rays, C.c_void_p), 2, None, C.cast(rgb, C.c_void_p), None,
                                     None) == _abi.RT_ERR_BAD_ARG
