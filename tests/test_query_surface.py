"""Ray queries, the part that needs no GPU: rt_tile.h declares rt_scene_intersect / rt_scene_intersect_device with the argument
lists the binding uses, both libraries export them, rt_ray and rt_hit are 32 bytes with the documented offsets (as are the
binding's Ray / Hit and their numpy twins), the ABI they were added to is unchanged (RT_ABI_VERSION 4, 64-byte request and stats),
and the argument checks refuse before any device work."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np

from ray_tracer_s8_amd import _abi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "rt_tile.h").read_text()

QUERY_ENTRY_POINTS = {
    "rt_scene_intersect": ["rt_scene*", "const rt_ray*", "uint32_t", "uint32_t", "uint32_t", "rt_hit*", "rt_tile_stats*"],
    "rt_scene_intersect_device": ["rt_scene*", "const void*", "uint32_t", "uint32_t", "uint32_t", "void*", "void*"],
}
RAY_FIELDS = ["ox", "oy", "oz", "t_min", "dx", "dy", "dz", "t_max"]
HIT_FIELDS = ["px", "py", "pz", "distance", "nx", "ny", "nz", "index"]


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
    m = re.search(r"typedef\s+struct\s+" + name + r"\s*\{([^}]*)\}\s*" + name + r"\s*;", HEADER)
    assert m, f"{name} is not defined in rt_tile.h"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(typ, n.strip()) for n in names.split(",")]
    return fields


def test_header_declares_the_query_entry_points():
    for name, params in QUERY_ENTRY_POINTS.items():
        assert _declared_params(name) == params, name
    assert re.search(r"#define\s+RT_HIT_NONE\s+0xffffffffu", HEADER)
    assert re.search(r"RT_QUERY_CLOSEST\s*=\s*0u\s*,\s*RT_QUERY_ANY\s*=\s*1u", HEADER)


def test_binding_argtypes_match_the_header():
    lib = _abi.load()
    vp, u32 = C.c_void_p, C.c_uint32
    assert lib.rt_scene_intersect.argtypes == [vp, C.POINTER(_abi.Ray), u32, u32, u32, C.POINTER(_abi.Hit), C.POINTER(_abi.TileStats)]
    assert lib.rt_scene_intersect.restype is C.c_int
    assert lib.rt_scene_intersect_device.argtypes == [vp, vp, u32, u32, u32, vp, vp]
    assert lib.rt_scene_intersect_device.restype is C.c_int


def test_product_and_test_libraries_export_the_query_entry_points():
    from ray_tracer_s8_amd import build
    _abi.load()
    _abi.load_debug()
    for path in (build.LIB_PATH, build.DEBUG_LIB_PATH):
        exported = _exported(path)
        for name in QUERY_ENTRY_POINTS:
            assert name in exported, (path, name)


def test_ray_and_hit_layouts():
    assert _header_struct_fields("rt_ray") == [("float", n) for n in RAY_FIELDS]
    assert _header_struct_fields("rt_hit") == [("float", n) for n in HIT_FIELDS[:-1]] + [("uint32_t", "index")]
    assert C.sizeof(_abi.Ray) == 32 and C.sizeof(_abi.Hit) == 32
    for i, n in enumerate(RAY_FIELDS):
        assert getattr(_abi.Ray, n).offset == 4 * i and _abi.RAY_DTYPE.fields[n][1] == 4 * i, n
    for i, n in enumerate(HIT_FIELDS):
        assert getattr(_abi.Hit, n).offset == 4 * i and _abi.HIT_DTYPE.fields[n][1] == 4 * i, n
    assert [n for n, _ in _abi.Ray._fields_] == RAY_FIELDS and [n for n, _ in _abi.Hit._fields_] == HIT_FIELDS
    assert _abi.RAY_DTYPE.itemsize == _abi.HIT_DTYPE.itemsize == 32
    assert _abi.HIT_DTYPE["index"] == np.dtype("<u4") and _abi.Hit.index.size == 4
    assert _abi.RT_HIT_NONE == 0xFFFFFFFF and (_abi.RT_QUERY_CLOSEST, _abi.RT_QUERY_ANY) == (0, 1)


def test_header_layout_compiles_as_c():
    """sizeof and offsetof as a C compiler sees the header."""
    gcc = shutil.which("gcc")
    assert gcc
    src = ("#include <stddef.h>\n#include \"rt_tile.h\"\n"
           "_Static_assert(sizeof(rt_ray) == 32, \"rt_ray\");\n_Static_assert(sizeof(rt_hit) == 32, \"rt_hit\");\n"
           "_Static_assert(offsetof(rt_ray, t_min) == 12 && offsetof(rt_ray, dx) == 16 && offsetof(rt_ray, t_max) == 28, \"ray\");\n"
           "_Static_assert(offsetof(rt_hit, distance) == 12 && offsetof(rt_hit, nx) == 16 && offsetof(rt_hit, index) == 28, \"hit\");\n"
           "_Static_assert(sizeof(rt_tile_request) == 64 && sizeof(rt_tile_stats) == 64, \"abi 4\");\n")
    r = subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_abi_version_and_struct_sizes_unchanged():
    assert re.search(r"#define\s+RT_ABI_VERSION\s+4u", HEADER)
    assert _abi.RT_ABI_VERSION == 4 and _abi.load().rt_abi_version() == 4
    assert C.sizeof(_abi.TileRequest) == 64 and C.sizeof(_abi.TileStats) == 64


def test_query_entry_points_check_arguments_without_a_device():
    """No scene: refused before anything else is looked at (the same checks come first on the GPU: test_gpu_query.py)."""
    lib = _abi.load()
    rays = (_abi.Ray * 2)()
    hits = (_abi.Hit * 2)()
    assert lib.rt_scene_intersect(None, rays, 2, 0, 0, hits, None) == _abi.RT_ERR_BAD_ARG
    assert lib.rt_scene_intersect_device(None, C.cast(rays, C.c_void_p), 2, 0, 0, C.cast(hits, C.c_void_p), None) == _abi.RT_ERR_BAD_ARG
