"""The a-trous denoiser, the part that needs no GPU: rt_tile.h documents the contract, the defaults, and the argument checks refuse
before any device work.  (The declarations of the entry points, RT_DENOISE_MAX_ITERATIONS, the binding's argument lists,
rt_denoise_request's layout in C and in ctypes, the exports and the ABI version: tests/test_surface.py.)"""
import ctypes as C

import numpy as np

import _denoise_np as dn
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

from _surface import HEADER, check_abi_version_unchanged, check_exports


def test_header_documents_the_contract():
    text = " ".join(HEADER[HEADER.index("denoiser: edge-avoiding"):].split())
    for phrase in ("Dammertz", "B3-spline", "dy outer, dx inner", "g_q != g_p", "the centre tap (0, 0) has t = 1",
                   "unless n_p and n_q are both 0", "t = 1 - x if that is > 0, else +0", "the dyadic product first",
                   "r_{i+1} = Sc / Sw", "m = albedo ? r_I * d : r_I", "bit for bit", "seams", "not limited to 64",
                   "rt_denoise_scratch_bytes(W, R)", "RT_ERR_LIMIT", "engine reports 0", "rt_scene_collect"):
        assert phrase in text, phrase
    version_comment = " ".join(HEADER[:HEADER.index("status codes")].split())
    assert "(4, additions only: the edge-avoiding a-trous denoiser rt_scene_denoise / rt_scene_denoise_device" in version_comment


def test_libraries_export_the_entry_points_and_the_product_exactly_the_header():
    check_exports(["rt_scene_denoise", "rt_scene_denoise_device", "rt_denoise_request_defaults", "rt_denoise_scratch_bytes"],
                  exactly=True)


def test_abi_version_unchanged():
    check_abi_version_unchanged()


def test_defaults():
    d = rt.DenoiseRequest.defaults()
    assert (d.color_samples, d.aov_samples, d.iterations, d.flags, d.reserved) == (1, 1, 5, 0, 0)
    assert d.color_step_scale == 4.0 and d.albedo_eps == 2.0 ** -8
    want = dn.defaults()
    assert (d.iterations, d.k_color, d.color_step_scale, d.k_normal, d.k_depth, d.albedo_eps) == (
        want["iterations"], want["k_color"], want["color_step_scale"], want["k_normal"], want["k_depth"], want["albedo_eps"])
    assert rt.DenoiseRequest.defaults(iterations=2, k_color=0.5).iterations == 2
    assert rt.denoise_scratch_bytes(3840, 2160) >= 48 * 3840 * 2160
    assert rt.denoise_scratch_bytes(1, 1) == 3 * 256


def test_entry_points_check_arguments_without_a_device():
    """No scene: refused before anything else is looked at (the other checks on the GPU: test_gpu_denoise.py)."""
    lib = _abi.load()
    vp = C.c_void_p
    rq = _abi.default_request(width=8, height=4, divisions=1, spp=2)
    dq = _abi.DenoiseRequest.defaults(color_samples=2)
    acc = (C.c_float * 96)()
    out = (C.c_uint8 * 96)()
    pl = _abi.AovPlanes()
    accp = (vp * 1)(C.cast(acc, vp).value)
    outp = (vp * 1)(C.cast(out, vp).value)
    assert lib.rt_scene_denoise(None, C.byref(rq), 1, C.byref(dq), accp, C.byref(pl), outp, 96, None, None, None) == _abi.RT_ERR_BAD_ARG
    scratch = (C.c_uint8 * 1024)()
    assert lib.rt_scene_denoise_device(None, C.byref(rq), 1, C.byref(dq), accp, C.byref(pl), outp, 96, None, None,
                                       C.cast(scratch, vp), 1024, None) == _abi.RT_ERR_BAD_ARG
    assert all(v == 0 for v in out)
