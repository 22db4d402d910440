"""Ray queries, the part that needs no GPU: the argument checks of rt_scene_intersect / rt_scene_intersect_device refuse before any
device work.  (Their declarations, the binding's argument lists, the layouts of rt_ray and rt_hit and of their numpy twins, the
exports, the ABI version and the 64-byte request and stats: tests/test_surface.py.)"""
import ctypes as C

from ray_tracer_s8_amd import _abi

from _surface import check_abi_version_unchanged, check_exports


def test_product_and_test_libraries_export_the_query_entry_points():
    check_exports(["rt_scene_intersect", "rt_scene_intersect_device"])


def test_abi_version_and_struct_sizes_unchanged():
    check_abi_version_unchanged()
    assert C.sizeof(_abi.TileRequest) == 64 and C.sizeof(_abi.TileStats) == 64


def test_query_entry_points_check_arguments_without_a_device():
    """No scene: refused before anything else is looked at (the same checks come first on the GPU: test_gpu_query.py)."""
    lib = _abi.load()
    rays = (_abi.Ray * 2)()
    hits = (_abi.Hit * 2)()
    assert lib.rt_scene_intersect(None, rays, 2, 0, 0, hits, None) == _abi.RT_ERR_BAD_ARG
    assert lib.rt_scene_intersect_device(None, C.cast(rays, C.c_void_p), 2, 0, 0, C.cast(hits, C.c_void_p), None) == _abi.RT_ERR_BAD_ARG
