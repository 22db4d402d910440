"""Host-side mirror of the reference's controller<->slave surface, on top of the C-ABI.

Reference (Rust, ray-tracer-slave/src/lib.rs:10-30):
    RenderInfo { world: Vec<Object>, render_meta: RenderMeta, division_no: u32 }
    RenderMeta { height, width, divisions, id: Uuid }
    ImageSlice { division_no, image: Vec<u8>, id: Uuid }
`Slave.render(info)` replaces the body of the slave's worker (main.rs:37-90); `Controller`
replaces dispatch + assembly (controller main.rs:47-75, 109-119) with GPUs as the slaves.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import threading
import uuid
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._abi import Camera, DenoiseRequest, FrameStats, TileRequest, TileStats, default_request
from .dispatch import assemble, strips_for_worker


@dataclass
class RenderMeta:
    height: int = 1080
    width: int = 1920
    divisions: int = 20
    id: uuid.UUID = field(default_factory=uuid.uuid4)


@dataclass
class World:
    """`world: Vec<Object>` (lib.rs:11) as the C-ABI carries it: the spheres, the triangles, and `world_index` — the
    position of every sphere, then of every triangle, in the list (None: the spheres in order, then the triangles).
    The order is observable (BVH::build numbers shapes by position, bvh_impl.rs:421-427: leaf order, tie winners)."""
    spheres: np.ndarray = field(default_factory=lambda: np.zeros(0, _abi.SPHERE_DTYPE))
    triangles: np.ndarray = field(default_factory=lambda: np.zeros(0, _abi.TRIANGLE_DTYPE))
    world_index: Optional[np.ndarray] = None

    def __post_init__(self):
        self.spheres = _abi.as_spheres(self.spheres)
        self.triangles = _abi.as_triangles(self.triangles)
        self.world_index = _abi.as_world_index(self.world_index, len(self.spheres) + len(self.triangles))

    def objects(self):
        """The list in the reference's order: ("Sphere" | "Triangle", record) per position."""
        n = len(self.spheres) + len(self.triangles)
        wi = self.world_index if self.world_index is not None else np.arange(n, dtype=np.uint32)
        out = [None] * n
        for i in range(n):
            out[int(wi[i])] = (("Sphere", self.spheres[i]) if i < len(self.spheres)
                               else ("Triangle", self.triangles[i - len(self.spheres)]))
        return out


@dataclass
class RenderSettings:
    """The knobs the reference hard-codes (defaults = its literals) + the job seed."""
    spp: int = 100
    max_bounces: int = 10
    aperture: float = 0.1
    focus_distance: float = 1.0
    fov: float = float(np.float32(np.pi) / np.float32(2.0))
    focal_length: float = 1.0
    t_min: float = 0.001
    t_max: float = 1000.0
    seed: int = 0
    flags: int = 0


@dataclass
class RenderInfo:
    world: World
    render_meta: RenderMeta
    division_no: int
    settings: RenderSettings = field(default_factory=RenderSettings)

    def request(self) -> TileRequest:
        s, m = self.settings, self.render_meta
        return default_request(width=m.width, height=m.height, divisions=m.divisions, division_no=self.division_no,
                               spp=s.spp, max_bounces=s.max_bounces, aperture=s.aperture,
                               focus_distance=s.focus_distance, fov=s.fov, focal_length=s.focal_length,
                               t_min=s.t_min, t_max=s.t_max, seed=s.seed, flags=s.flags)


@dataclass
class ImageSlice:
    division_no: int
    image: np.ndarray          # uint8, (H/div)*W*3, RGB, top row first
    id: uuid.UUID
    stats: Optional[TileStats] = None


_initialised_libs = set()                    # (the product library, and the test library where a test swapped it in)


def _is_initialised() -> bool:
    return id(_abi.load()) in _initialised_libs


def init() -> int:
    """rt_init(); returns the device count.  Raises RtError(RT_ERR_NO_DEVICE) without a GPU."""
    lib = _abi.load()
    n = C.c_int(0)
    _abi.check(lib.rt_init(C.byref(n)), "rt_init")
    _abi.check_single_hip_runtime()          # torch imported after the library was bound to ROCm's runtime: say so now
    _initialised_libs.add(id(lib))
    return n.value


# ---- marshalling, each step once: what the methods below hand to the entry points of _abi.SIGNATURES

def _addr(p: int):
    """An integer address (a device buffer, a HIP stream) as a pointer argument; 0 is NULL."""
    return C.c_void_p(p) if p else None


def _addr_array(addrs: Optional[Sequence[int]]):
    """One pointer per strip: the `void* const*` argument of a batch (None: NULL, the optional output is not wanted)."""
    return None if addrs is None else (C.c_void_p * len(addrs))(*[p or None for p in addrs])


_POINTEE = {np.dtype(np.uint8): C.c_uint8, np.dtype(np.uint32): C.c_uint32, np.dtype(np.uint64): C.c_uint64,
            np.dtype(np.float32): C.c_float, _abi.RAY_DTYPE: _abi.Ray, _abi.HIT_DTYPE: _abi.Hit, _abi.BOUNCE_DTYPE: _abi.Bounce,
            _abi.DIRECT_DTYPE: _abi.Direct}


def _arg(a: Optional[np.ndarray]):
    """A numpy array as a pointer argument: a pointer to the C type of its dtype, which the typed parameters require and the
    `void*` ones accept (it keeps the array alive); None is NULL."""
    return None if a is None else a.ctypes.data_as(C.POINTER(_POINTEE[a.dtype]))


def _requests(reqs: Sequence[TileRequest]):
    """The rt_tile_request array of a batch.  Marshalled afresh on every call (a few dozen structs): a cache keyed on id(reqs)
    served stale requests to a caller that changed seed or division_no in place."""
    return (TileRequest * len(reqs))(*reqs)


def _strip_shape(req: TileRequest):
    """(Hs, W) of the request's strip (a bad request is refused by the library)."""
    return req.height // max(req.divisions, 1), req.width


def _states(rng_state, n: int):
    """The optional (N, 4) uint64 xoshiro256++ states of n rays: None, or a C-ordered copy for the call to advance."""
    if rng_state is None:
        return None
    state = np.array(rng_state, np.uint64, order="C")
    if state.shape != (n, 4):
        raise ValueError(f"rng_state: need an (N, 4) uint64 array, got {state.shape}")
    return state


def _states_or_seeded(rng_state, n: int, seed: Optional[int]):
    """The required form: the copy of _states, or zeroed states for the library to seed when a seed stands in for them."""
    if rng_state is None and seed is None:
        raise ValueError("rng_state: need (N, 4) uint64 states, or a seed to make them from")
    return np.zeros((n, 4), np.uint64) if rng_state is None else _states(rng_state, n)


def _active(active):
    """(active, n_active) arguments of an active list: (NULL, 0) for None, all rays.  An empty list is still a list: the library gets
    a non-NULL pointer to an array of one."""
    if active is None:
        return None, 0
    act = np.ascontiguousarray(active, np.uint32).reshape(-1)
    return _arg(act if len(act) else np.zeros(1, np.uint32)), len(act)


def _aov_planes(strips: Sequence[dict]):
    """The rt_aov_planes array of a batch from one {plane name: address} dict per strip; a plane that is missing or 0 is NULL."""
    return (_abi.AovPlanes * len(strips))(*[_abi.AovPlanes(*[d.get(k) or None for k in _abi.AOV_PLANES]) for d in strips])


def _devices(devices: Optional[Sequence[int]]):
    """(devices, n_devices) arguments: the ordinals as a C int array, or (NULL, 0) for every device."""
    return (None, 0) if devices is None else ((C.c_int * len(devices))(*devices), len(devices))


def _world_args(world: "World"):
    """spheres, n_spheres, triangles, n_triangles, world_index of a World, in the order every entry point takes them."""
    return (_abi.ptr(world.spheres), len(world.spheres), _abi.ptr(world.triangles), len(world.triangles),
            _abi.ptr(world.world_index))


def _ray_form(as_given: bool) -> int:
    return _abi.RT_TRACE_RAY_AS_GIVEN if as_given else _abi.RT_TRACE_RAY_NEW


def _trace_request(spp, max_bounces, seed, flags, as_given) -> _abi.TraceRequest:
    return _abi.TraceRequest(spp, max_bounces, seed & 0xFFFFFFFFFFFFFFFF, flags, _ray_form(as_given))


def _bounce_request(flags, as_given, seed) -> _abi.BounceRequest:
    return _abi.BounceRequest(flags, _ray_form(as_given), 0 if seed is None else 1, 0, (seed or 0) & 0xFFFFFFFFFFFFFFFF)


def _direct_request(flags, t_min, t_max) -> _abi.DirectRequest:
    return _abi.DirectRequest(flags, 0, t_min, t_max)


def _nee_request(spp, max_bounces, seed, flags, as_given, mode) -> _abi.NeeRequest:
    return _abi.NeeRequest(spp, max_bounces, seed & 0xFFFFFFFFFFFFFFFF, flags, _ray_form(as_given), mode, 0)


def _pack_rays(origins, directions, t_min, t_max) -> np.ndarray:
    """The rt_ray array (RAY_DTYPE) of origins / directions (N, 3) and t_min / t_max (scalars or (N,))."""
    o = np.asarray(origins, np.float32)
    d = np.asarray(directions, np.float32)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError(f"origins and directions: need two (N, 3) arrays, got {o.shape} and {d.shape}")
    n = len(o)
    rays = np.empty(n, _abi.RAY_DTYPE)
    rays["ox"], rays["oy"], rays["oz"] = o[:, 0], o[:, 1], o[:, 2]
    rays["dx"], rays["dy"], rays["dz"] = d[:, 0], d[:, 1], d[:, 2]
    rays["t_min"] = np.broadcast_to(np.asarray(t_min, np.float32), (n,))
    rays["t_max"] = np.broadcast_to(np.asarray(t_max, np.float32), (n,))
    return rays


class Scene:
    """rt_scene handle: the world resident in one GPU's HBM."""

    def __init__(self, device: int, world: World):
        self._lib = _abi.load()
        if not _is_initialised():
            init()
        self.world = world
        self.device = device
        h = C.c_void_p()
        _abi.check(self._lib.rt_scene_create(device, *_world_args(world), C.byref(h)), "rt_scene_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_scene_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def render_tile(self, req: TileRequest, want_f32: bool = False):
        n = self._lib.rt_tile_bytes(C.byref(req))
        out = np.empty(n, np.uint8)
        outf = np.empty(n, np.float32) if want_f32 else None
        st = TileStats()
        _abi.check(self._lib.rt_scene_render_tile(self._h, C.byref(req), _arg(out), n, _arg(outf), C.byref(st)),
                   "rt_scene_render_tile")
        return out, outf, st

    def render_tile_pass(self, req: TileRequest, begin: int, end: int, accum: Optional[np.ndarray] = None,
                         want_f32: bool = False):
        """One progressive pass: samples [begin, end) of the req.spp-sample strip (rt_scene_render_tile_pass).  `accum` is the
        strip's running colour sum, a contiguous float32 (Hs, W, 3) array, updated in place; None is allowed for begin == 0 and
        allocates it.  Returns (rgb, f32 | None, accum, stats): the preview sqrt(sum / end), which at end == req.spp is
        bit-identical to render_tile(req) however the samples were split into passes."""
        n = self._lib.rt_tile_bytes(C.byref(req))
        shape = (*_strip_shape(req), 3)
        if accum is None:
            if begin != 0:
                raise ValueError("accum: a pass that starts after sample 0 continues a running sum: pass the one of the last pass")
            accum = np.empty(shape, np.float32)
        if accum.dtype != np.float32 or accum.shape != shape or not accum.flags.c_contiguous or not accum.flags.writeable:
            raise ValueError(f"accum: need a writeable contiguous float32 array of shape {shape}")
        out = np.empty(n, np.uint8)
        outf = np.empty(n, np.float32) if want_f32 else None
        st = TileStats()
        _abi.check(self._lib.rt_scene_render_tile_pass(self._h, C.byref(req), begin, end, _arg(accum), _arg(out), n, _arg(outf),
                                                       C.byref(st)), "rt_scene_render_tile_pass")
        return out, outf, accum, st

    def render_progressive(self, req: TileRequest, pass_spp: int):
        """Generator: the strip in passes of `pass_spp` samples (the last one may be shorter), yielding (end, rgb, stats) after
        each until end == req.spp; the last rgb equals render_tile(req).  Stop iterating to stop the job."""
        if pass_spp < 1:
            raise ValueError("pass_spp must be at least 1")
        accum = None
        begin = 0
        while begin < req.spp:
            end = min(begin + pass_spp, req.spp)
            rgb, _, accum, st = self.render_tile_pass(req, begin, end, accum)
            yield end, rgb, st
            begin = end

    def render_tile_device(self, req: TileRequest, d_out_ptr: int, out_len: int, d_f32_ptr: int = 0, stream: int = 0):
        _abi.check(self._lib.rt_scene_render_tile_device(self._h, C.byref(req), _addr(d_out_ptr), out_len, _addr(d_f32_ptr),
                                                         _addr(stream)), "rt_scene_render_tile_device")

    def render_tiles(self, reqs: Sequence[TileRequest], want_f32: bool = False, out=None):
        """Batched: strips of one frame, host buffers out (rt_scene_render_tiles).  `out`: a list of uint8 arrays
        from an earlier call to write into again (a caller that renders frame after frame keeps its pages warm)."""
        n = len(reqs)
        nb = self._lib.rt_tile_bytes(C.byref(reqs[0]))
        if out is not None:
            if len(out) != n or any(o.dtype != np.uint8 or o.size < nb or not o.flags.c_contiguous for o in out):
                raise ValueError("out: need one contiguous uint8 array of at least rt_tile_bytes per request")
        outs = out if out is not None else [np.empty(nb, np.uint8) for _ in range(n)]
        outf = [np.empty(nb, np.float32) for _ in range(n)] if want_f32 else None
        st = TileStats()
        _abi.check(self._lib.rt_scene_render_tiles(self._h, _requests(reqs), n, _addr_array([o.ctypes.data for o in outs]), nb,
                                                   _addr_array([o.ctypes.data for o in outf]) if want_f32 else None, C.byref(st)),
                   "rt_scene_render_tiles")
        return outs, outf, st

    def render_tiles_device(self, reqs: Sequence[TileRequest], d_out_ptrs: Sequence[int], out_len_each: int,
                            stream: int = 0):
        """Batched, asynchronous, device-resident output (rt_scene_render_tiles_device)."""
        _abi.check(self._lib.rt_scene_render_tiles_device(self._h, _requests(reqs), len(reqs), _addr_array(d_out_ptrs), out_len_each,
                                                          None, _addr(stream)), "rt_scene_render_tiles_device")

    def render_tiles_pass_device(self, reqs: Sequence[TileRequest], begin: int, end: int, d_accum_ptrs: Sequence[int],
                                 d_out_ptrs: Sequence[int], out_len_each: int, d_f32_ptrs: Optional[Sequence[int]] = None,
                                 stream: int = 0):
        """Batched progressive pass, asynchronous, device buffers (rt_scene_render_tiles_pass_device): samples [begin, end) of
        every strip, d_accum_ptrs[i] the running sum of strip i (Hs*W*3 floats on the device)."""
        _abi.check(self._lib.rt_scene_render_tiles_pass_device(self._h, _requests(reqs), len(reqs), begin, end,
                                                               _addr_array(d_accum_ptrs), _addr_array(d_out_ptrs), out_len_each,
                                                               _addr_array(d_f32_ptrs), _addr(stream)),
                   "rt_scene_render_tiles_pass_device")

    def intersect(self, origins, directions, t_min=0.001, t_max=1000.0, *, any_hit: bool = False, flags: int = 0):
        """Ray queries (rt_scene_intersect): the closest hit — or, with any_hit, whether there is one — of each ray
        Ray::new(origins[i], directions[i]) within [t_min, t_max).  origins / directions: (N, 3); t_min / t_max: scalars or (N,).
        Returns (hits, stats): a structured array of HIT_DTYPE (index = the primitive's position in the world, RT_HIT_NONE
        for a miss) and the call's TileStats."""
        rays = _pack_rays(origins, directions, t_min, t_max)
        n = len(rays)
        hits = np.empty(n, _abi.HIT_DTYPE)
        st = TileStats()
        _abi.check(self._lib.rt_scene_intersect(self._h, _arg(rays), n, _abi.RT_QUERY_ANY if any_hit else _abi.RT_QUERY_CLOSEST, flags,
                                                _arg(hits), C.byref(st)), "rt_scene_intersect")
        return hits, st

    def intersect_device(self, d_rays: int, n: int, d_hits: int, *, any_hit: bool = False, flags: int = 0, stream: int = 0):
        """Ray queries on device buffers (rt_scene_intersect_device): n rt_ray at d_rays, n rt_hit to d_hits (e.g. the
        data_ptr() of torch tensors), asynchronous on `stream`; counters until collect()."""
        _abi.check(self._lib.rt_scene_intersect_device(self._h, _addr(d_rays), n,
                                                       _abi.RT_QUERY_ANY if any_hit else _abi.RT_QUERY_CLOSEST, flags,
                                                       _addr(d_hits), _addr(stream)), "rt_scene_intersect_device")

    def trace(self, origins, directions, t_min=0.001, t_max=1000.0, *, spp: int = 1, max_bounces: int = 10, seed: int = 0,
              rng_state=None, as_given: bool = False, flags: int = 0):
        """Path tracing of caller rays (rt_scene_trace): for each ray, the f32 sum of `spp` samples of the reference's
        ray_color(ray, max_bounces + 1, rng) within [t_min, t_max).  origins / directions: (N, 3); t_min / t_max: scalars or (N,).
        as_given: take the directions bit for bit (RT_TRACE_RAY_AS_GIVEN) instead of Ray::new's normalisation.  rng_state: None
        for the seeded streams of `seed`, else (N, 4) uint64 xoshiro256++ states, one stream per ray.
        Returns (rgb_sum (N, 3) float32, segments (N,) uint32, stats), and the written-back states (N, 4) when rng_state is given."""
        rays = _pack_rays(origins, directions, t_min, t_max)
        n = len(rays)
        state = _states(rng_state, n)
        rq = _trace_request(spp, max_bounces, seed, flags, as_given)
        rgb = np.empty((n, 3), np.float32)
        segs = np.empty(n, np.uint32)
        st = TileStats()
        _abi.check(self._lib.rt_scene_trace(self._h, C.byref(rq), _arg(rays), n, _arg(state), _arg(rgb), _arg(segs), C.byref(st)),
                   "rt_scene_trace")
        if state is not None:
            return rgb, segs, st, state
        return rgb, segs, st

    def trace_device(self, d_rays: int, n: int, d_rgb: int, *, d_segments: int = 0, d_rng_state: int = 0, spp: int = 1,
                     max_bounces: int = 10, seed: int = 0, as_given: bool = False, flags: int = 0, stream: int = 0):
        """Path tracing on device buffers (rt_scene_trace_device): n rt_ray at d_rays, 3 n float32 sums to d_rgb, optionally
        n uint32 segments to d_segments and 4 n uint64 states at d_rng_state (read and written back) — e.g. the data_ptr() of
        torch tensors; asynchronous on `stream`, counters until collect()."""
        rq = _trace_request(spp, max_bounces, seed, flags, as_given)
        _abi.check(self._lib.rt_scene_trace_device(self._h, C.byref(rq), _addr(d_rays), n, _addr(d_rng_state), _addr(d_rgb),
                                                   _addr(d_segments), _addr(stream)), "rt_scene_trace_device")

    def bounce(self, rays, rng_state, active=None, as_given: bool = False, flags: int = 0, seed: Optional[int] = None,
               want_hits: bool = False, want_next: bool = False):
        """One path step of caller rays (rt_scene_bounce): one ray_color entry for each active ray — the closest hit, its shade, and
        for a ray that scatters the UnitSphere draw from its state and the scattered ray.  rays: (N,) RAY_DTYPE; rng_state: (N, 4)
        uint64; active: None (all N) or ray indices; as_given: take the directions bit for bit (the rays a step returns must be
        stepped so); seed: seed state i from seed_from_u64(seed + 4 PHI i) first (rng_state may then be None).  The inputs are not
        modified.  Returns a dict: `rays` and `states` (the scattered rays and their advanced states written over copies of the
        inputs), `bounce` (BOUNCE_DTYPE: the step's colour factor and RT_BOUNCE_* status; entries of rays that are not active
        are zero), `hits` (HIT_DTYPE of the incoming rays) when want_hits, `next` (the indices of the rays that scattered,
        ascending) when want_next, and `stats`."""
        r = np.array(rays, _abi.RAY_DTYPE, order="C")
        if r.ndim != 1:
            raise ValueError(f"rays: need a 1-d array of RAY_DTYPE records, got shape {r.shape}")
        n = len(r)
        state = _states_or_seeded(rng_state, n, seed)
        rq = _bounce_request(flags, as_given, seed)
        bnc = np.zeros(n, _abi.BOUNCE_DTYPE)
        hits = np.zeros(n, _abi.HIT_DTYPE) if want_hits else None
        nxt = np.zeros(n, np.uint32) if want_next else None
        n_next = C.c_uint32(0)
        st = TileStats()
        _abi.check(self._lib.rt_scene_bounce(self._h, C.byref(rq), _arg(r), n, _arg(state), *_active(active), _arg(bnc), _arg(hits),
                                             _arg(nxt), C.byref(n_next) if want_next else None, C.byref(st)), "rt_scene_bounce")
        out = {"rays": r, "states": state, "bounce": bnc, "stats": st}
        if want_hits:
            out["hits"] = hits
        if want_next:
            out["next"] = np.sort(nxt[:n_next.value])
        return out

    def bounce_device(self, d_rays: int, n: int, d_rng_state: int, d_bounce: int, *, d_active: int = 0, d_n_active: int = 0,
                      d_hits: int = 0, d_next_active: int = 0, d_n_next: int = 0, as_given: bool = False, flags: int = 0,
                      seed: Optional[int] = None, stream: int = 0):
        """One path step on device buffers (rt_scene_bounce_device): n rt_ray at d_rays and 4 n uint64 states at d_rng_state, both
        updated in place; n rt_bounce to d_bounce; optionally n rt_hit to d_hits, the active list d_active with its uint32 length
        at d_n_active (read on the device), and the list of the rays that scattered to d_next_active with its length to d_n_next —
        e.g. the data_ptr() of torch tensors; asynchronous on `stream`, counters until collect()."""
        rq = _bounce_request(flags, as_given, seed)
        _abi.check(self._lib.rt_scene_bounce_device(self._h, C.byref(rq), _addr(d_rays), n, _addr(d_rng_state), _addr(d_active),
                                                    _addr(d_n_active), _addr(d_bounce), _addr(d_hits), _addr(d_next_active),
                                                    _addr(d_n_next), _addr(stream)), "rt_scene_bounce_device")

    @property
    def n_lights(self) -> int:
        """The number M of emitters of the scene (rt_scene_light_count): the primitives with emission > 0."""
        m = C.c_uint32(0)
        _abi.check(self._lib.rt_scene_light_count(self._h, C.byref(m)), "rt_scene_light_count")
        return m.value

    def light_table(self, flags: int = 0):
        """The emitter list with its selection probabilities (rt_scene_light_table): (world_index (M,) uint32, p (M,) float32) — for
        emitter k its position in the world (the value rt_direct.light reports) and the probability it is picked with under `flags`:
        the mixture of the light table with RT_FLAG_LIGHTS_BY_POWER, 1 / M without.  Host only."""
        m = self.n_lights
        wi, p = np.zeros(m, np.uint32), np.zeros(m, np.float32)
        _abi.check(self._lib.rt_scene_light_table(self._h, flags, _arg(wi), _arg(p), m), "rt_scene_light_table")
        return wi, p

    def set_light_sampling(self, sampling: int):
        """How later direct() and trace_nee() calls sample the scene's sphere lights (rt_scene_set_light_sampling): _abi.RT_LIGHTS_AREA,
        over the whole sphere (the default), or _abi.RT_LIGHTS_CONE, over the cone the sphere subtends from the hit point.  Work already
        enqueued keeps the setting it was enqueued with; every other call ignores it."""
        _abi.check(self._lib.rt_scene_set_light_sampling(self._h, sampling), "rt_scene_set_light_sampling")

    @property
    def light_sampling(self) -> int:
        """The scene's light sampling (rt_scene_light_sampling): RT_LIGHTS_AREA or RT_LIGHTS_CONE."""
        v = C.c_uint32(0)
        _abi.check(self._lib.rt_scene_light_sampling(self._h, C.byref(v)), "rt_scene_light_sampling")
        return int(v.value)

    def set_glossy_sampling(self, sampling: int):
        """Whether later trace_nee() calls in mode RT_NEE_MIS take a light sample at hits of roughness 0 < rho < 1
        (rt_scene_set_glossy_sampling): _abi.RT_GLOSSY_BOUNCE, no (the default: such a hit falls back to the bounce), or
        _abi.RT_GLOSSY_MIS, one weighted by the density of the reference's scatter lobe.  Work already enqueued keeps the setting it was
        enqueued with; RT_NEE_LIGHT_ONLY, direct() and every other call ignore it."""
        _abi.check(self._lib.rt_scene_set_glossy_sampling(self._h, sampling), "rt_scene_set_glossy_sampling")

    @property
    def glossy_sampling(self) -> int:
        """The scene's glossy sampling (rt_scene_glossy_sampling): RT_GLOSSY_BOUNCE or RT_GLOSSY_MIS."""
        v = C.c_uint32(0)
        _abi.check(self._lib.rt_scene_glossy_sampling(self._h, C.byref(v)), "rt_scene_glossy_sampling")
        return int(v.value)

    def direct(self, hits, rng_state, active=None, t_min: float = 0.001, t_max: float = 1000.0, flags: int = 0):
        """Direct lighting of caller rays (rt_scene_direct): one light sample for each active hit record — an emitter picked with one
        u01 of the ray's state, a point on it, the shadow ray within [t_min, t_max) and the Lambertian estimate without the surface
        albedo.  hits: (N,) HIT_DTYPE, as a path step returns them; rng_state: (N, 4) uint64; active: None (all N) or record
        indices.  The inputs are not modified.  Returns a dict: `direct` (DIRECT_DTYPE; entries of records that are not active are
        zero), `states` (the advanced states written over a copy of the input) and `stats`."""
        h = np.array(hits, _abi.HIT_DTYPE, order="C")
        if h.ndim != 1:
            raise ValueError(f"hits: need a 1-d array of HIT_DTYPE records, got shape {h.shape}")
        n = len(h)
        if rng_state is None:
            raise ValueError("rng_state: need (N, 4) uint64 states")
        state = _states(rng_state, n)
        rq = _direct_request(flags, t_min, t_max)
        out = np.zeros(n, _abi.DIRECT_DTYPE)
        st = TileStats()
        _abi.check(self._lib.rt_scene_direct(self._h, C.byref(rq), _arg(h), n, _arg(state), *_active(active), _arg(out), C.byref(st)),
                   "rt_scene_direct")
        return {"direct": out, "states": state, "stats": st}

    def direct_device(self, d_hits: int, n: int, d_rng_state: int, d_out: int, *, d_active: int = 0, d_n_active: int = 0,
                      t_min: float = 0.001, t_max: float = 1000.0, flags: int = 0, stream: int = 0):
        """Direct lighting on device buffers (rt_scene_direct_device): n rt_hit at d_hits, 4 n uint64 states at d_rng_state (updated in
        place), n rt_direct to d_out; optionally the active list d_active with its uint32 length at d_n_active (read on the device:
        the d_next_active / d_n_next of a bounce step as they stand); asynchronous on `stream`, counters until collect()."""
        rq = _direct_request(flags, t_min, t_max)
        _abi.check(self._lib.rt_scene_direct_device(self._h, C.byref(rq), _addr(d_hits), n, _addr(d_rng_state), _addr(d_active),
                                                    _addr(d_n_active), _addr(d_out), _addr(stream)), "rt_scene_direct_device")

    def trace_nee(self, origins, directions, t_min=0.001, t_max=1000.0, *, spp: int = 1, max_bounces: int = 10, seed: int = 0,
                  rng_state=None, as_given: bool = False, mode: int = _abi.RT_NEE_MIS, flags: int = 0):
        """Next-event estimation for caller rays (rt_scene_trace_nee): for each ray, the f32 sum of `spp` samples of a path of at most
        max_bounces + 1 segments with one light sample after every hit of roughness 0 but the last, in one kernel.  mode:
        RT_NEE_LIGHT_ONLY (bit for bit the fold of Scene.bounce and Scene.direct) or RT_NEE_MIS (light sample and bounce combined by
        the balance heuristic).  The other arguments as Scene.trace.
        Returns (rgb_sum (N, 3) float32, segments (N,) uint32, shadow (N,) uint32, stats), and the written-back states (N, 4) when
        rng_state is given."""
        rays = _pack_rays(origins, directions, t_min, t_max)
        n = len(rays)
        state = _states(rng_state, n)
        rq = _nee_request(spp, max_bounces, seed, flags, as_given, mode)
        rgb = np.empty((n, 3), np.float32)
        segs, shadow = np.empty(n, np.uint32), np.empty(n, np.uint32)
        st = TileStats()
        _abi.check(self._lib.rt_scene_trace_nee(self._h, C.byref(rq), _arg(rays), n, _arg(state), _arg(rgb), _arg(segs), _arg(shadow),
                                                C.byref(st)), "rt_scene_trace_nee")
        if state is not None:
            return rgb, segs, shadow, st, state
        return rgb, segs, shadow, st

    def trace_nee_device(self, d_rays: int, n: int, d_rgb: int, *, d_segments: int = 0, d_shadow: int = 0, d_rng_state: int = 0,
                         spp: int = 1, max_bounces: int = 10, seed: int = 0, as_given: bool = False, mode: int = _abi.RT_NEE_MIS,
                         flags: int = 0, stream: int = 0):
        """Next-event estimation on device buffers (rt_scene_trace_nee_device): n rt_ray at d_rays, 3 n float32 sums to d_rgb,
        optionally n uint32 path segments to d_segments, n uint32 shadow rays to d_shadow and 4 n uint64 states at d_rng_state (read
        and written back) — e.g. the data_ptr() of torch tensors; asynchronous on `stream`, counters until collect()."""
        rq = _nee_request(spp, max_bounces, seed, flags, as_given, mode)
        _abi.check(self._lib.rt_scene_trace_nee_device(self._h, C.byref(rq), _addr(d_rays), n, _addr(d_rng_state), _addr(d_rgb),
                                                       _addr(d_segments), _addr(d_shadow), _addr(stream)),
                   "rt_scene_trace_nee_device")

    def render_aov(self, req: TileRequest, begin: int = 0, end: Optional[int] = None, *,
                   planes: Sequence[str] = _abi.AOV_PLANES, out: Optional[dict] = None):
        """Feature buffers of a strip (rt_scene_render_aov): over samples [begin, end) of the req.spp-sample job (end None:
        req.spp), the per-pixel sums of what the tile's own camera rays first hit — albedo (Hs, W, 3) float32 (the sky colour
        on a miss), normal (Hs, W, 3) float32, depth (Hs, W) float32, hits (Hs, W) uint32 — and index (Hs, W) uint32, the world
        position hit by sample 0 (RT_HIT_NONE: a miss; written only when begin == 0).  `out`: the dict of planes of an earlier
        call, updated in place, which carries the sums across calls (required when begin > 0, like render_tile_pass's accum).
        Returns (planes dict, stats); aov_means() turns the sums into means."""
        end = req.spp if end is None else end
        names = tuple(planes)
        bad = [n for n in names if n not in _abi.AOV_PLANES]
        if bad or not names:
            raise ValueError(f"planes: a non-empty subset of {_abi.AOV_PLANES}, got {names}")
        hs, w = _strip_shape(req)
        shapes = {"albedo": ((hs, w, 3), np.float32), "normal": ((hs, w, 3), np.float32),
                  "depth": ((hs, w), np.float32), "hits": ((hs, w), np.uint32), "index": ((hs, w), np.uint32)}
        if out is None:
            if begin != 0:
                raise ValueError("out: a call that starts after sample 0 continues the sums: pass the planes of the last call")
            out = {n: np.empty(*shapes[n]) for n in names}
        for n in names:
            a = out.get(n)
            shape, dt = shapes[n]
            if a is None or a.dtype != dt or a.shape != shape or not a.flags.c_contiguous or not a.flags.writeable:
                raise ValueError(f"out[{n!r}]: need a writeable contiguous {np.dtype(dt).name} array of shape {shape}")
        pl = _aov_planes([{n: out[n].ctypes.data for n in names}])
        st = TileStats()
        _abi.check(self._lib.rt_scene_render_aov(self._h, C.byref(req), begin, end, pl, C.byref(st)), "rt_scene_render_aov")
        return {n: out[n] for n in names}, st

    def render_aovs_device(self, reqs: Sequence[TileRequest], begin: int, end: int, d_planes: Sequence[dict], stream: int = 0):
        """Feature buffers of n strips of one frame on device buffers (rt_scene_render_aovs_device), asynchronous on `stream`,
        counters until collect().  d_planes[i]: {plane name: device pointer} of strip i (e.g. torch tensors' data_ptr()); every
        entry names the same planes."""
        n = len(reqs)
        if len(d_planes) != n:
            raise ValueError("d_planes: one entry per request")
        _abi.check(self._lib.rt_scene_render_aovs_device(self._h, _requests(reqs), n, begin, end, _aov_planes(d_planes), _addr(stream)),
                   "rt_scene_render_aovs_device")

    def denoise(self, reqs, accum, planes, color_samples: int, aov_samples: int = 1, dreq: Optional[DenoiseRequest] = None,
                outputs: Sequence[str] = ("rgb", "f32")):
        """The a-trous denoiser on host buffers (rt_scene_denoise).  reqs: one request or n strips of one frame with consecutive
        division_no; accum: the strips' progressive sums after [0, color_samples) ((Hs, W, 3) float32 each); planes: the strips'
        feature-buffer dicts of render_aov (summed over [0, aov_samples); 'index' ignored, any other plane optional, the same set
        for every strip); dreq: DenoiseRequest (None: the defaults), whose sample counts are set from the arguments; outputs: a
        non-empty subset of ("rgb", "linear", "f32").  Returns ({output: array}, stats) for one request, ([{...} per strip],
        stats) for a sequence."""
        single = isinstance(reqs, TileRequest)
        reqs = [reqs] if single else list(reqs)
        accum = [accum] if single else list(accum)
        planes = [planes] if single else list(planes)
        n = len(reqs)
        if len(accum) != n or len(planes) != n:
            raise ValueError("accum and planes: one entry per request")
        outs = tuple(outputs)
        if not outs or any(o not in DENOISE_OUTPUTS for o in outs):
            raise ValueError(f"outputs: a non-empty subset of {DENOISE_OUTPUTS}, got {outs}")
        dq = DenoiseRequest.defaults() if dreq is None else DenoiseRequest.from_buffer_copy(dreq)
        dq.color_samples, dq.aov_samples = color_samples, aov_samples
        shape = (*_strip_shape(reqs[0]), 3)
        acc = [np.ascontiguousarray(a, np.float32) for a in accum]
        if any(a.shape != shape for a in acc):
            raise ValueError(f"accum: need arrays of shape {shape}")
        want = {"albedo": np.float32, "normal": np.float32, "depth": np.float32, "hits": np.uint32}
        # (contiguous copies where needed, kept alive until the call returns)
        keep = [{k: np.ascontiguousarray(a, want[k]) for k, a in (d or {}).items() if k in want and a is not None} for d in planes]
        res = [{} for _ in range(n)]
        arrays = {}
        for o in DENOISE_OUTPUTS:
            if o in outs:
                for r in res:
                    r[o] = np.empty(shape, np.uint8 if o == "rgb" else np.float32)
                arrays[o] = _addr_array([r[o].ctypes.data for r in res])
            else:
                arrays[o] = None
        st = TileStats()
        _abi.check(self._lib.rt_scene_denoise(self._h, _requests(reqs), n, C.byref(dq), _addr_array([a.ctypes.data for a in acc]),
                                              _aov_planes([{k: a.ctypes.data for k, a in d.items()} for d in keep]), arrays["rgb"],
                                              shape[0] * shape[1] * 3, arrays["f32"], arrays["linear"], C.byref(st)),
                   "rt_scene_denoise")
        return (res[0] if single else res), st

    def denoise_device(self, reqs: Sequence[TileRequest], dreq: DenoiseRequest, d_accum: Sequence[int], d_planes: Sequence[dict],
                       d_scratch: int, scratch_bytes: int, *, d_rgb: Optional[Sequence[int]] = None,
                       d_f32: Optional[Sequence[int]] = None, d_linear: Optional[Sequence[int]] = None, out_len_each: int = 0,
                       stream: int = 0):
        """The denoiser on device buffers (rt_scene_denoise_device), asynchronous on `stream`, counters until collect().  d_accum:
        one device pointer per strip; d_planes[i]: {plane name: device pointer} of strip i (e.g. torch tensors' data_ptr()), the
        same names for every strip; d_scratch: >= denoise_scratch_bytes(W, n * Hs) bytes; d_rgb / d_f32 / d_linear: None or one
        device pointer per strip (out_len_each: 0 means Hs * W * 3)."""
        reqs = list(reqs)
        n = len(reqs)
        if len(d_accum) != n or len(d_planes) != n:
            raise ValueError("d_accum and d_planes: one entry per request")
        if any(a is not None and len(a) != n for a in (d_rgb, d_f32, d_linear)):
            raise ValueError("output arrays: one device pointer per request")
        if not out_len_each:
            hs, w = _strip_shape(reqs[0])
            out_len_each = hs * w * 3
        _abi.check(self._lib.rt_scene_denoise_device(self._h, _requests(reqs), n, C.byref(dreq), _addr_array(d_accum),
                                                     _aov_planes(d_planes), _addr_array(d_rgb), out_len_each, _addr_array(d_f32),
                                                     _addr_array(d_linear), _addr(d_scratch), scratch_bytes, _addr(stream)),
                   "rt_scene_denoise_device")

    def set_camera(self, cam: Optional[Camera]):
        """Place the camera of every later call that generates camera rays (rt_scene_set_camera): tiles, passes, feature buffers,
        camera_rays.  None: back to the reference camera.  Work already enqueued keeps the camera it was enqueued with."""
        _abi.check(self._lib.rt_scene_set_camera(self._h, C.byref(cam) if cam is not None else None), "rt_scene_set_camera")

    def camera_rays(self, req: TileRequest, begin: int = 0, end: Optional[int] = None, want_states: bool = True):
        """The camera rays of a strip (rt_scene_camera_rays): for samples [begin, end) of the req.spp-sample job (end None: req.spp),
        the ray the tile kernel traces first for each sample of each pixel, record (row W + x) (end - begin) + (s - begin).
        Returns (rays, states, stats): a RAY_DTYPE array whose directions are to be traced as given, and the (n, 4) uint64
        xoshiro256++ states after the camera's draws (None unless want_states) — the arguments of trace(..., as_given=True)."""
        end = req.spp if end is None else end
        hs, w = _strip_shape(req)
        n = hs * w * max(end - begin, 0)
        rays = np.empty(n, _abi.RAY_DTYPE)
        states = np.empty((n, 4), np.uint64) if want_states else None
        st = TileStats()
        _abi.check(self._lib.rt_scene_camera_rays(self._h, C.byref(req), begin, end, _arg(rays), _arg(states), C.byref(st)),
                   "rt_scene_camera_rays")
        return rays, states, st

    def camera_rays_device(self, req: TileRequest, begin: int, end: int, d_rays: int, d_rng_state: int = 0, stream: int = 0):
        """The camera rays of a strip on device buffers (rt_scene_camera_rays_device): Hs W (end - begin) rt_ray to d_rays and,
        optionally, 4 uint64 per record to d_rng_state — e.g. the data_ptr() of torch tensors that trace_device / intersect_device
        then read; asynchronous on `stream`, counters until collect()."""
        _abi.check(self._lib.rt_scene_camera_rays_device(self._h, C.byref(req), begin, end, _addr(d_rays), _addr(d_rng_state),
                                                         _addr(stream)), "rt_scene_camera_rays_device")

    def collect(self) -> TileStats:
        st = TileStats()
        _abi.check(self._lib.rt_scene_collect(self._h, C.byref(st)), "rt_scene_collect")
        return st


class Slave:
    """One GPU playing the reference's `ray-tracer-slave` worker."""

    def __init__(self, device: int = 0):
        self.device = device
        self._scene: Optional[Scene] = None
        self._scene_key = None
        # The reference slave drains its requests through ONE worker thread (slave main.rs:32-36, 159-160), so two
        # jobs never overlap on a slave.  Callers here may be threads of different jobs (controller_shim starts a set
        # per upload): the whole of render() — key check, scene swap, render — runs under this lock, or one job would
        # destroy the scene the other is rendering from.
        self._lock = threading.Lock()

    def render(self, info: RenderInfo) -> ImageSlice:
        with self._lock:
            return self._render_locked(info)

    def _render_locked(self, info: RenderInfo) -> ImageSlice:
        # the reference rebuilds the BVH per strip; the scene stays resident while the world's CONTENT is the same
        # (a slave behind HTTP gets a freshly decoded world object with every strip of a job)
        w = info.world
        key = (len(w.spheres), len(w.triangles), hashlib.blake2b(w.spheres.tobytes(), digest_size=16).digest(),
               hashlib.blake2b(w.triangles.tobytes(), digest_size=16).digest(),
               None if w.world_index is None else hashlib.blake2b(w.world_index.tobytes(), digest_size=16).digest())
        if self._scene is None or self._scene_key != key:
            if self._scene:
                self._scene.close()
            self._scene = Scene(self.device, info.world)
            self._scene_key = key
        img, _, st = self._scene.render_tile(info.request())
        return ImageSlice(division_no=info.division_no, image=img, id=info.render_meta.id, stats=st)

    def close(self):
        with self._lock:
            if self._scene:
                self._scene.close()
                self._scene = None


class Controller:
    """Dispatch strips to GPUs instead of docker slaves and assemble the frame."""

    def __init__(self, devices: Optional[Sequence[int]] = None):
        n = init()
        self.devices = list(devices) if devices is not None else list(range(n))
        self.slaves = [Slave(d) for d in self.devices]

    def render_frame(self, world: World, meta: RenderMeta, settings: RenderSettings) -> np.ndarray:
        """Strip k goes to slave k mod n; the slaves work concurrently, one dispatcher thread each (the controller fires
        its requests with join_all, controller main.rs:47-75; ctypes releases the GIL inside the render call)."""
        results: list = [None] * len(self.slaves)

        def run(w: int, slave: Slave):
            try:
                results[w] = [slave.render(RenderInfo(world, meta, k, settings))
                              for k in strips_for_worker(meta.divisions, w, len(self.slaves))]
            except BaseException as e:          # handed to the caller below
                results[w] = e

        threads = [threading.Thread(target=run, args=(w, s)) for w, s in enumerate(self.slaves)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        slices = []
        for r in results:
            if isinstance(r, BaseException):
                raise r
            slices += [(s.division_no, s.image) for s in r]
        return assemble(slices, meta.width, meta.height, meta.divisions)

    def close(self):
        for s in self.slaves:
            s.close()


def aov_means(planes: dict, n_samples: int) -> dict:
    """Means of the feature-buffer sums of Scene.render_aov after samples [0, n_samples): albedo / n_samples, the normal
    normalised (zero where no sample hit), depth / hits (zero where no sample hit).  hits and index are passed through."""
    out = {}
    hits = planes.get("hits")
    if "albedo" in planes:
        out["albedo"] = (planes["albedo"] / np.float32(n_samples)).astype(np.float32)
    if "normal" in planes:
        nrm = planes["normal"]
        ln = np.sqrt((nrm.astype(np.float32) ** 2).sum(-1, keepdims=True))
        with np.errstate(divide="ignore", invalid="ignore"):
            out["normal"] = np.where(ln > 0, nrm / ln, np.float32(0)).astype(np.float32)
        if hits is not None:
            out["normal"][hits == 0] = 0
    if "depth" in planes:
        if hits is None:
            raise ValueError("depth means need the hits plane")
        with np.errstate(divide="ignore", invalid="ignore"):
            out["depth"] = np.where(hits > 0, planes["depth"] / np.maximum(hits, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    for k in ("hits", "index"):
        if k in planes:
            out[k] = planes[k]
    return out


DENOISE_OUTPUTS = ("rgb", "linear", "f32")


def denoise_scratch_bytes(width: int, rows: int) -> int:
    """Device scratch rt_scene_denoise_device needs for an image of width x rows pixels (rt_denoise_scratch_bytes)."""
    return int(_abi.load().rt_denoise_scratch_bytes(width, rows))


class FrameContext:
    """rt_frame_ctx: the controller's state for a job — dispatcher threads, the world resident on every device, streams,
    strip buffers and the page-locked registration of the frame buffer, all made once and reused frame after frame
    (replaces controller main.rs:47-75, 109-115)."""

    def __init__(self, devices: Optional[Sequence[int]] = None, world: Optional[World] = None):
        self._lib = _abi.load()
        if not _is_initialised():
            init()
        h = C.c_void_p()
        _abi.check(self._lib.rt_frame_ctx_create(*_devices(devices), C.byref(h)), "rt_frame_ctx_create")
        self._h = h
        self._buf = None
        self._pinned = None                  # the array whose page-locked registration the context holds (kept alive here)
        if world is not None:
            self.set_world(world)

    def set_world(self, world: World):
        _abi.check(self._lib.rt_frame_ctx_set_world(self._h, *_world_args(world)), "rt_frame_ctx_set_world")

    def set_camera(self, cam: Optional[Camera]):
        """The job's camera (rt_frame_ctx_set_camera): every later frame is rendered from it; None: the reference camera."""
        _abi.check(self._lib.rt_frame_ctx_set_camera(self._h, C.byref(cam) if cam is not None else None), "rt_frame_ctx_set_camera")

    def render(self, req: TileRequest, out: Optional[np.ndarray] = None):
        """One frame.  `out`: a uint8 array of H*W*3 bytes to write into (the SAME array frame after frame keeps its
        page-locked registration: only the first frame pays pin_ms); default: the context's own buffer.
        Returns (H x W x 3 view of the buffer, FrameStats)."""
        n = req.width * req.height * 3
        if out is None:
            if self._buf is None or self._buf.size != n:
                self._buf = np.empty(n, np.uint8)
            out = self._buf
        if out.dtype != np.uint8 or out.size < n or not out.flags.c_contiguous:
            raise ValueError("out: need a contiguous uint8 array of at least H*W*3 bytes")
        # rt_tile.h: "the caller must not free a buffer the context still holds".  The context recognises a registered buffer by
        # its ADDRESS, and a freed array's address may come back with the next allocation — over pages that are no longer the
        # registered ones.  So the wrapper keeps the registered array alive (self._pinned) and drops the registration BEFORE
        # another array takes its place.
        if self._pinned is not None and self._pinned is not out:
            self.release_buffer()
        fs = FrameStats()
        try:
            _abi.check(self._lib.rt_frame_ctx_render(self._h, C.byref(req), _arg(out), out.size, C.byref(fs)), "rt_frame_ctx_render")
        finally:
            self._pinned = out               # (registered or not: harmless to hold, and an error return may have left it registered)
        return out.reshape(-1)[:n].reshape(req.height, req.width, 3), fs

    def release_buffer(self):
        _abi.check(self._lib.rt_frame_ctx_release_buffer(self._h), "rt_frame_ctx_release_buffer")
        self._pinned = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_frame_ctx_destroy(self._h)      # (drops the registration before the buffer can go away)
            self._h = None
            self._buf = None
            self._pinned = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def render_frame_native(world: World, req: TileRequest, devices: Optional[Sequence[int]] = None):
    """rt_render_frame: the one-shot form of FrameContext (create, set world, one frame, destroy)."""
    lib = _abi.load()
    if not _is_initialised():
        init()
    n = req.width * req.height * 3
    out = np.empty(n, np.uint8)
    st = TileStats()
    _abi.check(lib.rt_render_frame(*_devices(devices), C.byref(req), *_world_args(world), _arg(out), n, C.byref(st)),
               "rt_render_frame")
    return out.reshape(req.height, req.width, 3), st
