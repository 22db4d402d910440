"""Progressive passes, the part that needs no GPU: rt_tile.h declares the two pass entry points with the argument lists the
binding uses, the product library exports them, and the ABI they were added to is unchanged (RT_ABI_VERSION 4, 64-byte
rt_tile_request)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from ray_tracer_s8_amd import _abi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "rt_tile.h").read_text()

PASS_ENTRY_POINTS = {
    "rt_scene_render_tile_pass": ["rt_scene*", "const rt_tile_request*", "uint32_t", "uint32_t", "float*", "uint8_t*", "size_t",
                                  "float*", "rt_tile_stats*"],
    "rt_scene_render_tiles_pass_device": ["rt_scene*", "const rt_tile_request*", "uint32_t", "uint32_t", "uint32_t", "void* const*",
                                          "void* const*", "size_t", "void* const*", "void*"],
}


def _declared_params(name):
    m = re.search(r"RT_API\s+int\s+" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in rt_tile.h"
    types = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        t = re.sub(r"\s*\b\w+$", "", arg)                 # drop the parameter name
        types.append(re.sub(r"\s*\*", "*", t))
    return types


def test_header_declares_the_pass_entry_points():
    for name, params in PASS_ENTRY_POINTS.items():
        assert _declared_params(name) == params, name


def test_binding_argtypes_match_the_header():
    lib = _abi.load()
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    req, stats = C.POINTER(_abi.TileRequest), C.POINTER(_abi.TileStats)
    assert lib.rt_scene_render_tile_pass.argtypes == [vp, req, u32, u32, f32p, u8p, sz, f32p, stats]
    assert lib.rt_scene_render_tile_pass.restype is C.c_int
    assert lib.rt_scene_render_tiles_pass_device.argtypes == [vp, req, u32, u32, u32, C.POINTER(vp), C.POINTER(vp), sz,
                                                              C.POINTER(vp), vp]
    assert lib.rt_scene_render_tiles_pass_device.restype is C.c_int


def test_product_library_exports_the_pass_entry_points():
    from ray_tracer_s8_amd import build
    _abi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in PASS_ENTRY_POINTS:
        assert name in exported, name


def test_abi_version_and_request_layout_unchanged():
    assert re.search(r"#define\s+RT_ABI_VERSION\s+4u", HEADER)
    assert _abi.RT_ABI_VERSION == 4 and _abi.load().rt_abi_version() == 4
    assert C.sizeof(_abi.TileRequest) == 64


def test_pass_entry_points_check_arguments_without_a_device():
    """No scene: refused before anything else is looked at (this container has no GPU)."""
    lib = _abi.load()
    rq = _abi.default_request(width=16, height=4, divisions=1, spp=8)
    acc = (C.c_float * (16 * 4 * 3))()
    out = (C.c_uint8 * (16 * 4 * 3))()
    assert lib.rt_scene_render_tile_pass(None, C.byref(rq), 0, 8, acc, out, len(out), None, None) == _abi.RT_ERR_BAD_ARG
    ptrs = (C.c_void_p * 1)(None)
    assert lib.rt_scene_render_tiles_pass_device(None, C.byref(rq), 1, 0, 8, ptrs, ptrs, len(out), None, None) == _abi.RT_ERR_BAD_ARG
