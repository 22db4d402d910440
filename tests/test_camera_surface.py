"""The placed camera, the part that needs no GPU: rt_tile.h declares rt_camera and its entry points with the argument lists the
binding uses, both libraries export them, rt_camera is 44 bytes with the documented offsets, the ABI it was added to is unchanged,
and the argument checks refuse before any device work."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "rt_tile.h").read_text()

INT_ENTRY_POINTS = {
    "rt_scene_set_camera": ["rt_scene*", "const rt_camera*"],
    "rt_frame_ctx_set_camera": ["rt_frame_ctx*", "const rt_camera*"],
    "rt_scene_camera_rays": ["rt_scene*", "const rt_tile_request*", "uint32_t", "uint32_t", "rt_ray*", "uint64_t*", "rt_tile_stats*"],
    "rt_scene_camera_rays_device": ["rt_scene*", "const rt_tile_request*", "uint32_t", "uint32_t", "void*", "void*", "void*"],
}


def _declared_params(name, ret="int"):
    m = re.search(r"RT_API\s+" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
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


def test_header_declares_the_camera_entry_points():
    for name, params in INT_ENTRY_POINTS.items():
        assert _declared_params(name) == params, name
    assert _declared_params("rt_camera_defaults", "void") == ["rt_camera*"]
    assert re.search(r"#define\s+RT_ABI_VERSION\s+4u", HEADER)
    assert "rt_scene_set_camera must not race" in HEADER


def test_binding_argtypes_match_the_header():
    lib = _abi.load()
    vp, u32, cam, rq = C.c_void_p, C.c_uint32, C.POINTER(_abi.Camera), C.POINTER(_abi.TileRequest)
    assert lib.rt_camera_defaults.argtypes == [cam] and lib.rt_camera_defaults.restype is None
    assert lib.rt_scene_set_camera.argtypes == [vp, cam] and lib.rt_scene_set_camera.restype is C.c_int
    assert lib.rt_frame_ctx_set_camera.argtypes == [vp, cam] and lib.rt_frame_ctx_set_camera.restype is C.c_int
    assert lib.rt_scene_camera_rays.argtypes == [vp, rq, u32, u32, C.POINTER(_abi.Ray), C.POINTER(C.c_uint64), C.POINTER(_abi.TileStats)]
    assert lib.rt_scene_camera_rays_device.argtypes == [vp, rq, u32, u32, vp, vp, vp]
    assert lib.rt_scene_camera_rays.restype is C.c_int and lib.rt_scene_camera_rays_device.restype is C.c_int
    assert rt.Camera is _abi.Camera and "Camera" in rt.__all__


def test_product_and_test_libraries_export_the_camera_entry_points():
    from ray_tracer_s8_amd import build
    _abi.load()
    _abi.load_debug()
    for path in (build.LIB_PATH, build.DEBUG_LIB_PATH):
        exported = _exported(path)
        for name in list(INT_ENTRY_POINTS) + ["rt_camera_defaults"]:
            assert name in exported, (path, name)


def test_camera_layout():
    assert C.sizeof(_abi.Camera) == 44
    assert [(n, getattr(_abi.Camera, n).offset) for n, _ in _abi.Camera._fields_] == \
        [("origin", 0), ("target", 12), ("up", 24), ("flags", 36), ("reserved", 40)]
    gcc = shutil.which("gcc")
    assert gcc
    src = ("#include <stddef.h>\n#include \"rt_tile.h\"\n"
           "_Static_assert(sizeof(rt_camera) == 44, \"rt_camera\");\n"
           "_Static_assert(offsetof(rt_camera, target) == 12 && offsetof(rt_camera, up) == 24 && offsetof(rt_camera, flags) == 36 && "
           "offsetof(rt_camera, reserved) == 40, \"camera\");\n"
           "_Static_assert(sizeof(rt_tile_request) == 64 && sizeof(rt_tile_stats) == 64 && sizeof(rt_frame_stats) == 232, \"abi 4\");\n")
    r = subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_defaults_are_the_reference_camera():
    lib = _abi.load()
    c = _abi.Camera()
    c.flags = c.reserved = 7
    lib.rt_camera_defaults(C.byref(c))
    assert (list(c.origin), list(c.target), list(c.up), c.flags, c.reserved) == ([0, 0, 0], [0, 0, -1], [0, 1, 0], 0, 0)
    lib.rt_camera_defaults(None)                                                     # tolerated, like the other *_defaults
    assert bytes(c) == bytes(_abi.Camera.defaults())
    d = _abi.Camera.look_at((1, 2, 3), (4, 5, 6), up=(0, 0, 1))
    assert (list(d.origin), list(d.target), list(d.up)) == ([1, 2, 3], [4, 5, 6], [0, 0, 1])


def test_camera_entry_points_check_arguments_without_a_device():
    """No scene or context: refused before anything else is looked at (the same checks come first on the GPU)."""
    lib = _abi.load()
    cam = _abi.Camera.defaults()
    rq = _abi.default_request(width=8, height=4, divisions=1, spp=2)
    rays = (_abi.Ray * 64)()
    assert lib.rt_scene_set_camera(None, C.byref(cam)) == _abi.RT_ERR_BAD_ARG
    assert lib.rt_scene_set_camera(None, None) == _abi.RT_ERR_BAD_ARG
    assert lib.rt_frame_ctx_set_camera(None, C.byref(cam)) == _abi.RT_ERR_BAD_ARG
    assert lib.rt_scene_camera_rays(None, C.byref(rq), 0, 2, rays, None, None) == _abi.RT_ERR_BAD_ARG
    assert lib.rt_scene_camera_rays_device(None, C.byref(rq), 0, 2, C.cast(rays, C.c_void_p), None, None) == _abi.RT_ERR_BAD_ARG
    assert b"scene is NULL" in lib.rt_last_error()
