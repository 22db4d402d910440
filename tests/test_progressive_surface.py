"""Progressive passes, the part that needs no GPU: the argument checks of the two pass entry points refuse before any device work.
(Their declarations, the binding's argument lists, the exports, the ABI version and the 64-byte rt_tile_request:
tests/test_surface.py.)"""
import ctypes as C

from ray_tracer_s8_amd import _abi

from _surface import check_abi_version_unchanged, check_exports


def test_product_library_exports_the_pass_entry_points():
    check_exports(["rt_scene_render_tile_pass", "rt_scene_render_tiles_pass_device"], debug=False)


def test_abi_version_and_request_layout_unchanged():
    check_abi_version_unchanged()
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
