"""ctypes binding of include/rt_tile.h — the same stub a cgo / Rust `extern "C"` user
would write.  Loading fails loudly when the HIP library is missing:
there is no CPU fallback in the product path."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import build as _build

RT_ABI_VERSION = 4          # include/rt_tile.h RT_ABI_VERSION; load() refuses a library of another version

# ---- status codes (rt_status)
RT_OK = 0
RT_ERR_BAD_ARG = -1
RT_ERR_NOT_INITIALIZED = -2
RT_ERR_NO_DEVICE = -3
RT_ERR_BAD_DEVICE = -4
RT_ERR_BUFFER_TOO_SMALL = -5
RT_ERR_FRAME_SIZE = -6
RT_ERR_HIP = -7
RT_ERR_LIMIT = -8
RT_ERR_OOM = -9

RT_FLAG_NONE = 0
RT_FLAG_EXACT_SCAN = 1
RT_FLAG_NO_BVH_CULL = 2
RT_FLAG_OC_BROAD_PHASE = 4
RT_FLAG_FULL_CHAIN = 8
RT_FLAG_BVH_TRAVERSE = 16
RT_FLAG_LINEAR_SCAN = 32
RT_FLAG_EXACT_NODES = 64
RT_FLAG_QUANT_NODES = 128
RT_FLAG_NO_LDS_TREE = 256
RT_FLAG_COUNT_STEPS = 512
RT_FLAG_CULL_WALK = 1024
RT_FLAG_NO_CULL_WALK = 2048
RT_FLAG_FRAME_QUEUE = 4096          # frame-level (rt_render_frame / rt_frame_ctx_render): dynamic strip queue
RT_FLAG_FRAME_NO_PIN = 8192         # frame-level: do not page-lock the caller's frame buffer
RT_FLAG_FRAME_STATIC = 16384        # frame-level: strip k -> devices[k % n] instead of the cost-balanced assignment
RT_FLAG_LIGHTS_BY_POWER = 32768     # rt_scene_direct* / rt_scene_trace_nee*: the emitter is picked by power (mixture with uniform)
RT_LIGHTS_AREA = 0                  # rt_scene_set_light_sampling: a sphere light is sampled over its whole area (the default) ...
RT_LIGHTS_CONE = 1                  # ... or over the cone it subtends from the hit point
RT_GLOSSY_BOUNCE = 0                # rt_scene_set_glossy_sampling: RT_NEE_MIS takes no light sample at a hit of roughness > 0 (the default) ...
RT_GLOSSY_MIS = 1                   # ... or one weighted by the density of the reference's scatter lobe, at 0 < roughness < 1
RT_MAX_BOUNCES = 62
RT_MAX_SPP = 4096                 # samples per pixel limit (rt_tile.h)
RT_MAX_PRIMITIVES = 0x3ffffff     # spheres + triangles of a scene: what the kernels' 32-bit byte offsets can address
RT_FRAME_STATS_ENTRIES = 16       # rt_frame_stats.entry_segments


def _record_dtype(struct) -> np.dtype:
    """The numpy record dtype with the layout of a ctypes Structure of scalars (arrays of it are what the calls pass and return)."""
    return np.dtype([(n, np.dtype(t).str) for n, t in struct._fields_])


# numpy dtypes with the exact layout of rt_sphere / rt_triangle (no padding)
SPHERE_DTYPE = np.dtype(
    [("cx", "<f4"), ("cy", "<f4"), ("cz", "<f4"), ("radius", "<f4"),
     ("albedo_r", "<f4"), ("albedo_g", "<f4"), ("albedo_b", "<f4"),
     ("roughness", "<f4"), ("emission", "<f4")]
)
TRIANGLE_DTYPE = np.dtype(
    [("a", "<f4", 3), ("b", "<f4", 3), ("c", "<f4", 3),
     ("albedo_r", "<f4"), ("albedo_g", "<f4"), ("albedo_b", "<f4"),
     ("roughness", "<f4"), ("emission", "<f4")]
)
assert SPHERE_DTYPE.itemsize == 36 and TRIANGLE_DTYPE.itemsize == 56


class TileRequest(C.Structure):
    """rt_tile_request = RenderMeta + division_no + the knobs the reference hard-codes."""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("divisions", C.c_uint32),
        ("division_no", C.c_uint32), ("spp", C.c_uint32), ("max_bounces", C.c_uint32),
        ("aperture", C.c_float), ("focus_distance", C.c_float), ("fov", C.c_float),
        ("focal_length", C.c_float), ("t_min", C.c_float), ("t_max", C.c_float),
        ("seed", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32),
    ]

    def copy(self) -> "TileRequest":
        r = TileRequest()
        C.memmove(C.byref(r), C.byref(self), C.sizeof(TileRequest))
        return r


class TileStats(C.Structure):
    _fields_ = [
        ("ray_segments", C.c_uint64), ("primary_rays", C.c_uint64),
        ("broad_candidates", C.c_uint64), ("exact_fallbacks", C.c_uint64),
        ("kernel_ms", C.c_float), ("h2d_ms", C.c_float), ("d2h_ms", C.c_float),
        ("n_launches", C.c_uint32), ("engine", C.c_uint32), ("broad_form", C.c_uint32),
        ("node_steps", C.c_uint64),
    ]


class FrameStats(C.Structure):
    """rt_frame_stats: where the wall time of one rt_frame_ctx_render call went (ms)."""
    _fields_ = [
        ("totals", TileStats), ("wall_ms", C.c_float), ("pin_ms", C.c_float), ("scene_ms", C.c_float),
        ("kernel_ms", C.c_float), ("d2h_exposed_ms", C.c_float), ("host_ms", C.c_float),
        ("n_devices", C.c_uint32), ("pinned", C.c_uint32),
        ("assignment", C.c_uint32), ("balance_max_over_mean", C.c_float), ("entry_segments", C.c_uint64 * RT_FRAME_STATS_ENTRIES),
    ]


class Ray(C.Structure):
    """rt_ray: origin and window start, direction (normalised by the library, Ray::new) and window end [t_min, t_max)."""
    _fields_ = [("ox", C.c_float), ("oy", C.c_float), ("oz", C.c_float), ("t_min", C.c_float),
                ("dx", C.c_float), ("dy", C.c_float), ("dz", C.c_float), ("t_max", C.c_float)]


class Hit(C.Structure):
    """rt_hit: hit point, |P - o|, the reference's normal, the primitive's position in the world (RT_HIT_NONE: a miss)."""
    _fields_ = [("px", C.c_float), ("py", C.c_float), ("pz", C.c_float), ("distance", C.c_float),
                ("nx", C.c_float), ("ny", C.c_float), ("nz", C.c_float), ("index", C.c_uint32)]


RT_HIT_NONE = 0xFFFFFFFF
RT_QUERY_CLOSEST = 0
RT_QUERY_ANY = 1
# numpy twins of rt_ray / rt_hit (arrays of them are what Scene.intersect passes and returns)
RAY_DTYPE = _record_dtype(Ray)
HIT_DTYPE = _record_dtype(Hit)

class TraceRequest(C.Structure):
    """rt_trace_request: samples per ray, bounces, seed of the seeded streams, RT_FLAG_* and the form of the first ray."""
    _fields_ = [("spp", C.c_uint32), ("max_bounces", C.c_uint32), ("seed", C.c_uint64), ("flags", C.c_uint32),
                ("ray_form", C.c_uint32)]


RT_TRACE_RAY_NEW = 0
RT_TRACE_RAY_AS_GIVEN = 1


class Bounce(C.Structure):
    """rt_bounce: the colour factor of one path step (the albedo, albedo * emission or the sky) and its RT_BOUNCE_* status."""
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float), ("status", C.c_uint32)]


class BounceRequest(C.Structure):
    """rt_bounce_request: RT_FLAG_*, the form of the incoming rays, whether the states are seeded first, and the seed."""
    _fields_ = [("flags", C.c_uint32), ("ray_form", C.c_uint32), ("seed_states", C.c_uint32), ("reserved", C.c_uint32),
                ("seed", C.c_uint64)]


RT_BOUNCE_SCATTERED = 0
RT_BOUNCE_EMITTED = 1
RT_BOUNCE_MISSED = 2
# numpy twin of rt_bounce (what Scene.bounce returns)
BOUNCE_DTYPE = _record_dtype(Bounce)


class DirectRequest(C.Structure):
    """rt_direct_request: RT_FLAG_* of the shadow rays and their window [t_min, t_max)."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32), ("t_min", C.c_float), ("t_max", C.c_float)]


class Direct(C.Structure):
    """rt_direct: one light sample of a hit — the estimate (without the surface albedo), the emitter's position in the world, the
    point sampled on it and the RT_DIRECT_* status."""
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float), ("light", C.c_uint32),
                ("lx", C.c_float), ("ly", C.c_float), ("lz", C.c_float), ("status", C.c_uint32)]


RT_DIRECT_LIT = 0
RT_DIRECT_OCCLUDED = 1
RT_DIRECT_FACING_AWAY = 2
RT_DIRECT_NO_LIGHTS = 3
RT_DIRECT_SKIPPED = 4
# numpy twin of rt_direct (what Scene.direct returns)
DIRECT_DTYPE = _record_dtype(Direct)


class NeeRequest(C.Structure):
    """rt_nee_request: rt_trace_request's fields, then the RT_NEE_* mode of the integrator."""
    _fields_ = [("spp", C.c_uint32), ("max_bounces", C.c_uint32), ("seed", C.c_uint64), ("flags", C.c_uint32),
                ("ray_form", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32)]


RT_NEE_LIGHT_ONLY = 0
RT_NEE_MIS = 1


class AovPlanes(C.Structure):
    """rt_aov_planes: the feature buffers of a strip (host or device pointers); a NULL plane is not computed."""
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("hits", C.c_void_p),
                ("index", C.c_void_p)]


AOV_PLANES = ("albedo", "normal", "depth", "hits", "index")

RT_DENOISE_MAX_ITERATIONS = 8


class DenoiseRequest(C.Structure):
    """rt_denoise_request: the a-trous denoiser's parameters (rt_tile.h "denoiser"); DenoiseRequest.defaults() for the library's."""
    _fields_ = [("color_samples", C.c_uint32), ("aov_samples", C.c_uint32), ("iterations", C.c_uint32), ("flags", C.c_uint32),
                ("k_color", C.c_float), ("color_step_scale", C.c_float), ("k_normal", C.c_float), ("k_depth", C.c_float),
                ("albedo_eps", C.c_float), ("reserved", C.c_uint32)]

    @classmethod
    def defaults(cls, **kw) -> "DenoiseRequest":
        r = cls()
        load().rt_denoise_request_defaults(C.byref(r))
        for k, v in kw.items():
            setattr(r, k, v)
        return r

class Camera(C.Structure):
    """rt_camera: a pose of the strips' camera (rt_tile.h "placed camera") — the eye, a point looked at, a roll reference."""
    _fields_ = [("origin", C.c_float * 3), ("target", C.c_float * 3), ("up", C.c_float * 3), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]

    @classmethod
    def defaults(cls) -> "Camera":
        """The reference camera as a pose (rt_camera_defaults): origin 0, target (0, 0, -1), up (0, 1, 0).  Pure Python, like
        default_request."""
        return cls.look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))

    @classmethod
    def look_at(cls, origin, target, up=(0.0, 1.0, 0.0)) -> "Camera":
        c = cls()
        c.origin[:], c.target[:], c.up[:] = [float(x) for x in origin], [float(x) for x in target], [float(x) for x in up]
        return c


assert C.sizeof(TileRequest) == 64
assert C.sizeof(Camera) == 44
assert C.sizeof(TileStats) == 64
assert C.sizeof(FrameStats) == 232
assert C.sizeof(Ray) == C.sizeof(Hit) == RAY_DTYPE.itemsize == HIT_DTYPE.itemsize == 32
assert C.sizeof(TraceRequest) == 24
assert C.sizeof(BounceRequest) == 24 and C.sizeof(Bounce) == BOUNCE_DTYPE.itemsize == 16
assert C.sizeof(DirectRequest) == 16 and C.sizeof(Direct) == DIRECT_DTYPE.itemsize == 32
assert C.sizeof(NeeRequest) == 32
assert C.sizeof(AovPlanes) == 40
assert C.sizeof(DenoiseRequest) == 40

# the structs of rt_tile.h by their C names (rt_sphere and rt_triangle have numpy records only: SPHERE_DTYPE, TRIANGLE_DTYPE)
STRUCTS = {
    "rt_tile_request": TileRequest, "rt_tile_stats": TileStats, "rt_frame_stats": FrameStats, "rt_ray": Ray, "rt_hit": Hit,
    "rt_trace_request": TraceRequest, "rt_bounce": Bounce, "rt_bounce_request": BounceRequest, "rt_direct_request": DirectRequest,
    "rt_direct": Direct, "rt_nee_request": NeeRequest, "rt_aov_planes": AovPlanes, "rt_denoise_request": DenoiseRequest,
    "rt_camera": Camera,
}


def _signatures() -> dict:
    P, vp, i32, u32, sz = C.POINTER, C.c_void_p, C.c_int, C.c_uint32, C.c_size_t
    vpp, intp, u8p, u32p, u64p, f32p = P(vp), P(i32), P(C.c_uint8), P(u32), P(C.c_uint64), P(C.c_float)
    req, stats, ray, hit, planes, dreq, cam = P(TileRequest), P(TileStats), P(Ray), P(Hit), P(AovPlanes), P(DenoiseRequest), P(Camera)
    trq, brq, drq, nrq = P(TraceRequest), P(BounceRequest), P(DirectRequest), P(NeeRequest)
    return {
        "rt_init": (i32, [intp]),
        "rt_shutdown": (None, []),
        "rt_abi_version": (u32, []),
        "rt_hip_runtime_path": (sz, [C.c_char_p, sz]),
        "rt_strerror": (C.c_char_p, [i32]),
        "rt_last_error": (C.c_char_p, []),
        "rt_tile_request_defaults": (None, [req]),
        "rt_tile_bytes": (sz, [req]),
        "rt_render_tile": (i32, [i32, req, vp, u32, vp, u32, vp, vp, sz, vp, stats]),
        "rt_scene_create": (i32, [i32, vp, u32, vp, u32, vp, vpp]),
        "rt_scene_destroy": (None, [vp]),
        "rt_scene_render_tile": (i32, [vp, req, vp, sz, vp, stats]),
        "rt_scene_render_tile_device": (i32, [vp, req, vp, sz, vp, vp]),
        "rt_scene_render_tiles_device": (i32, [vp, req, u32, vpp, sz, vpp, vp]),
        "rt_scene_render_tiles": (i32, [vp, req, u32, vpp, sz, vpp, stats]),
        "rt_scene_render_tile_pass": (i32, [vp, req, u32, u32, f32p, u8p, sz, f32p, stats]),
        "rt_scene_render_tiles_pass_device": (i32, [vp, req, u32, u32, u32, vpp, vpp, sz, vpp, vp]),
        "rt_scene_collect": (i32, [vp, stats]),
        "rt_scene_intersect": (i32, [vp, ray, u32, u32, u32, hit, stats]),
        "rt_scene_intersect_device": (i32, [vp, vp, u32, u32, u32, vp, vp]),
        "rt_scene_trace": (i32, [vp, trq, ray, u32, u64p, f32p, u32p, stats]),
        "rt_scene_trace_device": (i32, [vp, trq, vp, u32, vp, vp, vp, vp]),
        "rt_scene_bounce": (i32, [vp, brq, ray, u32, u64p, u32p, u32, P(Bounce), hit, u32p, u32p, stats]),
        "rt_scene_bounce_device": (i32, [vp, brq, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rt_scene_light_count": (i32, [vp, u32p]),
        "rt_scene_light_table": (i32, [vp, u32, u32p, f32p, u32]),
        "rt_scene_direct": (i32, [vp, drq, hit, u32, u64p, u32p, u32, P(Direct), stats]),
        "rt_scene_direct_device": (i32, [vp, drq, vp, u32, vp, vp, vp, vp, vp]),
        "rt_scene_set_light_sampling": (i32, [vp, u32]),
        "rt_scene_light_sampling": (i32, [vp, u32p]),
        "rt_scene_trace_nee": (i32, [vp, nrq, ray, u32, u64p, f32p, u32p, u32p, stats]),
        "rt_scene_trace_nee_device": (i32, [vp, nrq, vp, u32, vp, vp, vp, vp, vp]),
        "rt_scene_set_glossy_sampling": (i32, [vp, u32]),
        "rt_scene_glossy_sampling": (i32, [vp, u32p]),
        "rt_scene_render_aov": (i32, [vp, req, u32, u32, planes, stats]),
        "rt_scene_render_aovs_device": (i32, [vp, req, u32, u32, u32, planes, vp]),
        "rt_denoise_request_defaults": (None, [dreq]),
        "rt_denoise_scratch_bytes": (sz, [u32, u32]),
        "rt_scene_denoise": (i32, [vp, req, u32, dreq, vpp, planes, vpp, sz, vpp, vpp, stats]),
        "rt_scene_denoise_device": (i32, [vp, req, u32, dreq, vpp, planes, vpp, sz, vpp, vpp, vp, sz, vp]),
        "rt_camera_defaults": (None, [cam]),
        "rt_scene_set_camera": (i32, [vp, cam]),
        "rt_scene_camera_rays": (i32, [vp, req, u32, u32, ray, u64p, stats]),
        "rt_scene_camera_rays_device": (i32, [vp, req, u32, u32, vp, vp, vp]),
        "rt_frame_ctx_create": (i32, [intp, i32, vpp]),
        "rt_frame_ctx_set_world": (i32, [vp, vp, u32, vp, u32, vp]),
        "rt_frame_ctx_set_camera": (i32, [vp, cam]),
        "rt_frame_ctx_render": (i32, [vp, req, vp, sz, P(FrameStats)]),
        "rt_frame_ctx_release_buffer": (i32, [vp]),
        "rt_frame_ctx_destroy": (None, [vp]),
        "rt_render_frame": (i32, [intp, i32, req, vp, u32, vp, u32, vp, vp, sz, stats]),
    }


# every entry point of rt_tile.h, in the header's order: name -> (restype, argtypes).  _bind applies it to a loaded library; a
# new entry point is one line here (tests/test_surface.py compares the table with the header, type by type)
SIGNATURES = _signatures()
# the rt_debug_* hooks of the test library that load_debug binds on top
DEBUG_SIGNATURES = {
    "rt_debug_set": (C.c_int, [C.c_char_p, C.c_int]),
    "rt_debug_unit": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_void_p, C.c_void_p]),
}


def default_request(**kw) -> TileRequest:
    """Reference literals (slave main.rs:39-51, shapes/mod.rs:12-13, controller main.rs:33-39).
    Pure Python so that host-side code and CPU tests need no GPU library."""
    r = TileRequest(width=1920, height=1080, divisions=20, division_no=0, spp=100, max_bounces=10,
                    aperture=0.1, focus_distance=1.0, fov=float(np.float32(np.pi) / np.float32(2.0)),
                    focal_length=1.0, t_min=0.001, t_max=1000.0, seed=0, flags=0, reserved=0)
    for k, v in kw.items():
        if not hasattr(r, k):
            raise AttributeError(k)
        setattr(r, k, v)
    return r


class RtError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str):
        super().__init__(f"{what}: status {status} ({detail})")
        self.status = status


_lib = None


def lib_path() -> Path:
    return _build.LIB_PATH


def load(build_if_missing: bool = True) -> C.CDLL:
    """Load librt_s8.so (building it with hipcc if absent).  Raises if it cannot."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB_PATH
    if build_if_missing:
        path = _build.build()
    _lib = _bind(path)
    return _lib


_dbg_lib = None


def load_debug() -> C.CDLL:
    """The TEST library lib/librt_s8_dbg.so: the product sources plus the rt_debug_* hooks (build.py).  A second, independent
    instance of the library in the process (its own rt_init state)."""
    global _dbg_lib
    if _dbg_lib is None:
        _dbg_lib = _bind(_build.build_debug())
        _apply(_dbg_lib, DEBUG_SIGNATURES)
    return _dbg_lib


class debug_library:
    """`with _abi.debug_library():` — everything the package does inside the block (rt.init(), Scene, FrameContext, debug_set)
    goes to the test library instead of the product library.  Tests and tools only."""

    def __enter__(self):
        global _lib
        self._prev = _lib
        _lib = load_debug()
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self._prev
        return False


def _apply(lib: C.CDLL, table: dict) -> None:
    for name, (restype, argtypes) in table.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, list(argtypes)


def _bind(path: Path) -> C.CDLL:
    if not path.exists():
        raise FileNotFoundError(
            f"{path} not found: the HIP extension is required (run `python -m ray_tracer_s8_amd.build`); "
            "there is no CPU fallback")
    lib = C.CDLL(str(path))
    _apply(lib, {"rt_abi_version": SIGNATURES["rt_abi_version"]})
    if lib.rt_abi_version() != RT_ABI_VERSION:
        raise RuntimeError(f"{path} has ABI version {lib.rt_abi_version()}, this binding is written for "
                           f"{RT_ABI_VERSION}: rebuild it (python -m ray_tracer_s8_amd.build)")
    _apply(lib, SIGNATURES)
    return lib


def check(status: int, what: str) -> None:
    if status != RT_OK:
        lib = load()
        raise RtError(status, what, f"{lib.rt_strerror(status).decode()}: {lib.rt_last_error().decode()}")


def as_spheres(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=SPHERE_DTYPE) if a is not None else np.zeros(0, SPHERE_DTYPE)
    return a


def as_triangles(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=TRIANGLE_DTYPE) if a is not None else np.zeros(0, TRIANGLE_DTYPE)
    return a


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def as_world_index(a, n: int):
    """world_index argument: None, or one uint32 position per primitive (spheres, then triangles)."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.size != n:
        raise ValueError(f"world_index: {a.size} entries for {n} primitives")
    return a


def hip_runtime_path() -> str:
    """The libamdhip64 file the library's HIP calls are bound to (rt_hip_runtime_path).  PyTorch wheels bundle their own
    runtime; whichever of torch / this library is loaded FIRST decides which one this library uses
    (profiles/README.md, "two HIP runtimes in one process")."""
    buf = C.create_string_buffer(4096)
    return buf.value.decode() if load().rt_hip_runtime_path(buf, 4096) else ""


def hip_runtime() -> C.CDLL:
    """ctypes handle of THAT runtime (already mapped: the same instance the library uses), for callers that make their own
    streams or device buffers (tests)."""
    p = hip_runtime_path()
    if not p:
        raise RuntimeError("cannot tell which HIP runtime librt_s8.so is bound to")
    return C.CDLL(p)


def check_single_hip_runtime() -> None:
    """Refuse a process in which torch and this library would drive the GPU through DIFFERENT HIP runtimes: the second one
    to initialise finds "no ROCm-capable device" (round 2: torch.cuda.Stream() after 122 tests of this library), and a stream
    or event made by one is garbage to the other.  Safe orders: import torch first (the library then binds to torch's
    runtime), or never import torch in the process."""
    import sys
    if "torch" not in sys.modules:
        return
    import os
    torch = sys.modules["torch"]
    tdir = os.path.realpath(os.path.join(os.path.dirname(torch.__file__), "lib"))
    mine = os.path.realpath(hip_runtime_path())
    bundled = os.path.exists(os.path.join(tdir, "libamdhip64.so"))
    if bundled and mine and os.path.dirname(mine) != tdir:
        raise RuntimeError(f"librt_s8.so is bound to {mine} but torch brings its own HIP runtime in {tdir}: two HIP runtimes in one "
                           "process cannot share the device.  Import torch BEFORE loading ray_tracer_s8_amd, or keep torch out "
                           "of this process.")


def debug_set(name: str, value: int) -> int:
    """Set a launch-path knob (RT_FORCE_CAPPED, RT_STACK_LDS, RT_CULL_WALK, ...: csrc/rt_api.hip DebugKnob); returns the
    previous value.  Tests and tools only."""
    lib = load()
    if not hasattr(lib, "rt_debug_set"):
        raise RuntimeError("debug_set needs the test library: use it inside `with _abi.debug_library():` (the product library "
                           "exports no rt_debug_* hooks)")
    prev = lib.rt_debug_set(name.encode(), int(value))
    if prev == -2**31:
        raise KeyError(name)
    return prev
