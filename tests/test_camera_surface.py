"""The placed camera, the part that needs no GPU: rt_tile.h states the race rule, the package's names, the defaults, and the argument
checks refuse before any device work.  (The declarations of rt_camera's entry points, the binding's argument lists, rt_camera's
layout, the exports and the ABI version: tests/test_surface.py.)"""
import ctypes as C

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

from _surface import HEADER, check_exports


def test_header_declares_the_camera_entry_points():
    assert "rt_scene_set_camera must not race" in HEADER


def test_package_exports_the_camera():
    assert rt.Camera is _abi.Camera and "Camera" in rt.__all__


def test_product_and_test_libraries_export_the_camera_entry_points():
    check_exports(["rt_scene_set_camera", "rt_frame_ctx_set_camera", "rt_scene_camera_rays", "rt_scene_camera_rays_device",
                   "rt_camera_defaults"])


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
