"""The a-trous denoiser, the part that needs no GPU: rt_tile.h declares rt_denoise_request, RT_DENOISE_MAX_ITERATIONS and the entry
points with the argument lists the binding uses and documents the contract, both libraries export the new symbols (and the product
library still exports exactly what the header declares), rt_denoise_request is 40 bytes with the documented offsets in C and in
ctypes, the ABI is unchanged (RT_ABI_VERSION 4), the defaults, and the argument checks refuse before any device work."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np

import _denoise_np as dn
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "rt_tile.h").read_text()

ENTRY_POINTS = {
    "rt_scene_denoise": ["rt_scene*", "const rt_tile_request*", "uint32_t", "const rt_denoise_request*", "const float* const*",
                         "const rt_aov_planes*", "uint8_t* const*", "size_t", "float* const*", "float* const*", "rt_tile_stats*"],
    "rt_scene_denoise_device": ["rt_scene*", "const rt_tile_request*", "uint32_t", "const rt_denoise_request*", "const void* const*",
                                "const rt_aov_planes*", "void* const*", "size_t", "void* const*", "void* const*", "void*", "size_t",
                                "void*"],
}
FIELDS = [("uint32_t", "color_samples", 0), ("uint32_t", "aov_samples", 4), ("uint32_t", "iterations", 8), ("uint32_t", "flags", 12),
          ("float", "k_color", 16), ("float", "color_step_scale", 20), ("float", "k_normal", 24), ("float", "k_depth", 28),
          ("float", "albedo_eps", 32), ("uint32_t", "reserved", 36)]


def _declared_params(name):
    m = re.search(r"RT_API\s+\w+\s+" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in rt_tile.h"
    types = []
    for arg in m.group(1).split(","):
        arg = " ".join(re.sub(r"/\*.*?\*/", "", arg).split())
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
        decl = " ".join(decl.split())
        if decl:
            typ, name_ = decl.rsplit(" ", 1)
            fields.append((typ.replace(" ", ""), name_))
    return fields


def test_header_declares_the_entry_points():
    for name, params in ENTRY_POINTS.items():
        assert _declared_params(name) == params, name
    assert _declared_params("rt_denoise_request_defaults") == ["rt_denoise_request*"]
    assert _declared_params("rt_denoise_scratch_bytes") == ["uint32_t", "uint32_t"]
    assert re.search(r"RT_API\s+size_t\s+rt_denoise_scratch_bytes", HEADER)
    assert re.search(r"#define\s+RT_DENOISE_MAX_ITERATIONS\s+8u", HEADER)


def test_header_documents_the_contract():
    text = " ".join(HEADER[HEADER.index("denoiser: edge-avoiding"):].split())
    for phrase in ("Dammertz", "B3-spline", "dy outer, dx inner", "g_q != g_p", "the centre tap (0, 0) has t = 1",
                   "unless n_p and n_q are both 0", "t = 1 - x if that is > 0, else +0", "the dyadic product first",
                   "r_{i+1} = Sc / Sw", "m = albedo ? r_I * d : r_I", "bit for bit", "seams", "not limited to 64",
                   "rt_denoise_scratch_bytes(W, R)", "RT_ERR_LIMIT", "engine reports 0", "rt_scene_collect"):
        assert phrase in text, phrase
    version_comment = " ".join(HEADER[:HEADER.index("status codes")].split())
    assert "(4, additions only: the edge-avoiding a-trous denoiser rt_scene_denoise / rt_scene_denoise_device" in version_comment


def test_binding_argtypes_match_the_header():
    lib = _abi.load()
    vp, u32 = C.c_void_p, C.c_uint32
    P = C.POINTER
    assert lib.rt_scene_denoise.argtypes == [vp, P(_abi.TileRequest), u32, P(_abi.DenoiseRequest), P(vp), P(_abi.AovPlanes), P(vp),
                                             C.c_size_t, P(vp), P(vp), P(_abi.TileStats)]
    assert lib.rt_scene_denoise_device.argtypes == [vp, P(_abi.TileRequest), u32, P(_abi.DenoiseRequest), P(vp), P(_abi.AovPlanes),
                                                    P(vp), C.c_size_t, P(vp), P(vp), vp, C.c_size_t, vp]
    assert lib.rt_scene_denoise.restype is C.c_int and lib.rt_scene_denoise_device.restype is C.c_int
    assert lib.rt_denoise_request_defaults.argtypes == [P(_abi.DenoiseRequest)] and lib.rt_denoise_request_defaults.restype is None
    assert lib.rt_denoise_scratch_bytes.argtypes == [u32, u32] and lib.rt_denoise_scratch_bytes.restype is C.c_size_t


def test_libraries_export_the_entry_points_and_the_product_exactly_the_header():
    from ray_tracer_s8_amd import build
    _abi.load()
    _abi.load_debug()
    names = list(ENTRY_POINTS) + ["rt_denoise_request_defaults", "rt_denoise_scratch_bytes"]
    for path in (build.LIB_PATH, build.DEBUG_LIB_PATH):
        exported = _exported(path)
        for name in names:
            assert name in exported, (path, name)
    declared = set(re.findall(r"RT_API\s+[\w\s\*]*?\b(rt_\w+)\s*\(", HEADER))
    product = {s for s in _exported(build.LIB_PATH) if s.startswith("rt_")}
    assert product == declared, (product ^ declared)


def test_denoise_request_layout():
    assert _header_struct_fields("rt_denoise_request") == [(t, n) for t, n, _ in FIELDS]
    assert C.sizeof(_abi.DenoiseRequest) == 40
    for _, n, off in FIELDS:
        f = getattr(_abi.DenoiseRequest, n)
        assert f.offset == off and f.size == 4, n
    gcc = shutil.which("gcc")
    assert gcc
    src = "#include <stddef.h>\n#include \"rt_tile.h\"\n_Static_assert(sizeof(rt_denoise_request) == 40, \"size\");\n"
    src += "".join(f"_Static_assert(offsetof(rt_denoise_request, {n}) == {off}, \"{n}\");\n" for _, n, off in FIELDS)
    r = subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_abi_version_unchanged():
    assert re.search(r"#define\s+RT_ABI_VERSION\s+4u", HEADER)
    assert _abi.RT_ABI_VERSION == 4 and _abi.load().rt_abi_version() == 4


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
