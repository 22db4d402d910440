"""A device-resident film: frames from the tile's own camera rays through the caller-ray integrators to the denoiser, with no host
round trip.

The film composes entry points that exist: rt_scene_camera_rays_device writes the camera rays of a strip and the RNG states after
them, rt_scene_trace_device or rt_scene_trace_nee_device traces them as given, one sample per record, and the film folds the records
into a per-pixel f32 sum that rt_scene_render_aovs_device's feature buffers and rt_scene_denoise_device consume.  The fold is the only
arithmetic here: a few elementwise f32 adds done with torch on the device.

Normative: after passes covering [0, e), accum[p] is the f32 sum in the order s = 0 ... e - 1, starting from +0, of the colour the
chosen integrator returns for the camera ray of (p, s) traced from the camera's state of (p, s) — bit for bit however the samples were
cut into passes or sub-ranges.  With integrator="path" that sum is the tile path's progressive accum.

With moments=True the film also keeps, per pixel, the sums S1 and S2 of the samples' y = (c0 + c1) + c2 and of y y, folded by a HIP
kernel of the film library (lib/librt_film.so, film_csrc/) that replaces the torch fold, and resolve_guided() runs that
library's variance-guided a-trous over accum and the moments.  resolve_regression() runs that library's other kind of resolve, a local
regression of the colour on the feature planes, with or without moments.

This module imports without torch; torch is imported when a Film is constructed, and must have been imported before the library
bound a HIP runtime (_abi.check_single_hip_runtime)."""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional, Sequence

from . import _abi, _film_lib
from ._abi import DenoiseRequest, TileRequest, TileStats
from .interface import DENOISE_OUTPUTS, denoise_scratch_bytes

INTEGRATORS = ("path", "nee")
NEE_MODES = (_abi.RT_NEE_LIGHT_ONLY, _abi.RT_NEE_MIS)
FEATURE_PLANES = ("albedo", "normal", "depth", "hits")
# The library holds at most 16 384 uncollected launches per scene (rt_scene_collect): the film collects into its running sum before
# its own could pass half of that, which leaves the other half to whatever else the caller enqueues on the scene.
COLLECT_AT = 8192
# resolve_guided: what it writes, the planes it reads, and its defaults.  sigma_l: the least mean squared error of the
# grid 1 ... 128 at 8 samples on c2 and c3 (SVGF's 4 leaves most of the noise in: a variance estimated from 8 samples and not
# accumulated over frames is itself noisy); var_eps, a standard deviation of y, is small against that of a visibly noisy pixel, keeps
# a step of 1/255 in converged regions and barely moves the error anywhere on the grid (4.23 "Measured").
GUIDED_OUTPUTS = ("rgb", "linear", "f32", "variance")
GUIDED_PLANES = ("normal", "depth", "hits")
GUIDED_MAX_ITERATIONS = _film_lib.MAX_ITERATIONS
SIGMA_L = 16.0
VAR_EPS = 2.0 ** -8
# resolve_regression: what it writes, the floats of a node's record, and the ridge of the fit, lambda n added to the
# diagonal of every feature but the constant.  RIDGE: measured on the grid 1e-5 ... 1e-1 on c2 and c3 (4.31 "Measured").  The grid has
# no single best: at 8 and at 32 samples the error is flat from 1e-5 to 1e-3, and which end is ahead, by under 2 %, changes with the
# scene and the planes; 1e-4 is the middle of that stretch and within 2 % of the least error of each of those rows.  At 2 samples on c2
# the other end, 1e-1, is better by a quarter.  In f32 a ridge of 1e-7 and below loses the pivots of collinear features (a flat wall's
# normal) to rounding, so the default keeps three decades above that.
REGRESSION_OUTPUTS = ("rgb", "linear", "f32")
REGRESSION_RECORD = _film_lib.REGRESS_RECORD
REGRESSION_PITCH = 16
RIDGE = 1e-4

# every field of a request but division_no: what the strips of one frame agree on
_FRAME_FIELDS = tuple(n for n, _ in TileRequest._fields_ if n != "division_no")
# the fields of rt_tile_stats that add up over launches (engine and broad_form are those of the last launch)
_SUMMED_STATS = ("ray_segments", "primary_rays", "broad_candidates", "exact_fallbacks", "kernel_ms", "h2d_ms", "d2h_ms", "n_launches",
                 "node_steps")


def sample_chunks(pixels: int, begin: int, end: int, max_records: int) -> list:
    """The schedule of a pass over a strip of `pixels` pixels: samples [begin, end) cut, in order, into sub-ranges (b, e) of at most
    max_records // pixels samples, so that no sub-range makes more than max_records records.  Pure: no torch, no GPU."""
    if pixels < 1 or max_records < 1:
        raise ValueError("pixels and max_records must be at least 1")
    if begin < 0 or end < begin:
        raise ValueError(f"samples [{begin}, {end}): need 0 <= begin <= end")
    k = max_records // pixels
    if k < 1:
        raise ValueError(f"a strip of {pixels} pixels makes more than max_records = {max_records} records per sample: use more "
                         "divisions or a larger max_records")
    return [(b, min(b + k, end)) for b in range(begin, end, k)]


class FilmPlan(NamedTuple):
    """What check_job makes of a film's arguments: the strips (copies, top to bottom), the strip's rows, the width, the image's rows
    R = n Hs, the job's sample count and k, the most samples of a strip the scratch holds."""
    reqs: tuple
    hs: int
    width: int
    rows: int
    spp: int
    k: int


def check_job(reqs, integrator: str = "nee", mode: int = _abi.RT_NEE_MIS, max_records: int = 1 << 22) -> FilmPlan:
    """The checks of Film's arguments, all of them ValueError and none of them a GPU call: one TileRequest or the strips of one frame
    (consecutive ascending division_no, every other field the same), a known integrator and mode, and a strip that fits max_records."""
    if integrator not in INTEGRATORS:
        raise ValueError(f"integrator: one of {INTEGRATORS}, got {integrator!r}")
    if mode not in NEE_MODES:
        raise ValueError(f"mode: RT_NEE_LIGHT_ONLY or RT_NEE_MIS, got {mode!r}")
    strips = [reqs] if isinstance(reqs, TileRequest) else list(reqs)
    if not strips or any(not isinstance(r, TileRequest) for r in strips):
        raise ValueError("reqs: one TileRequest or a non-empty sequence of them")
    r0 = strips[0]
    if r0.width == 0 or r0.height == 0 or r0.divisions == 0 or r0.spp == 0 or r0.height // r0.divisions == 0:
        raise ValueError("reqs: width, height, divisions, spp and the rows of a strip must be non-zero")
    for i, r in enumerate(strips):
        differ = [f for f in _FRAME_FIELDS if getattr(r, f) != getattr(r0, f)]
        if differ:
            raise ValueError(f"reqs[{i}] differs from reqs[0] in {differ}: the strips of one frame agree on every field but division_no")
        if r.division_no != r0.division_no + i:
            raise ValueError(f"reqs[{i}].division_no is {r.division_no}: strips have consecutive ascending division_no from "
                             f"{r0.division_no}")
    if strips[-1].division_no >= r0.divisions:
        raise ValueError(f"division_no {strips[-1].division_no} of {r0.divisions} divisions")
    hs = r0.height // r0.divisions
    k = min(r0.spp, max_records // (hs * r0.width)) if max_records >= 1 else 0
    if k < 1:
        raise ValueError(f"a strip of {hs} x {r0.width} pixels makes more than max_records = {max_records} records per sample: use "
                         "more divisions or a larger max_records")
    return FilmPlan(tuple(r.copy() for r in strips), hs, r0.width, hs * len(strips), r0.spp, k)


def fold(accum, records) -> None:
    """accum (P, 3) += records (P, n, 3), sample by sample: accum.add_(records[:, j]) for j = 0 ... n - 1 in that order, one plain f32
    add per element each.  Never a sum over the axis: its order is unspecified."""
    for j in range(records.shape[1]):
        accum.add_(records[:, j])


def check_guided(moments: bool, samples: int, planes: Sequence[str] = (), outputs: Sequence[str] = ("rgb",), iterations: int = 5,
                 sigma_l: float = SIGMA_L, var_eps: float = VAR_EPS, k_normal: float = 1.0, k_depth: float = 4.0) -> tuple:
    """The checks of resolve_guided's arguments, all of them ValueError and none of them a GPU call.  moments: whether the film was
    made with moments=True; planes: the names of the planes given (index is ignored).  Returns (planes, outputs) as tuples, the
    planes in GUIDED_PLANES' order.  Pure: no torch, no GPU."""
    if not moments:
        raise ValueError("resolve_guided and variance need a film made with moments=True")
    if samples < 2:
        raise ValueError(f"the film holds {samples} samples: a variance needs at least 2")
    outs = tuple(outputs)
    if not outs or any(o not in GUIDED_OUTPUTS for o in outs) or len(set(outs)) != len(outs):
        raise ValueError(f"outputs: a non-empty subset of {GUIDED_OUTPUTS}, got {outs}")
    names = tuple(n for n in planes if n != "index")
    if "albedo" in names:
        raise ValueError("planes: the guided filter does not demodulate by the albedo, leave it out")
    if any(n not in GUIDED_PLANES for n in names):
        raise ValueError(f"planes: a subset of {GUIDED_PLANES}, got {names}")
    if "depth" in names and "hits" not in names:
        raise ValueError("planes: the depth plane needs the hits plane")
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= GUIDED_MAX_ITERATIONS:
        raise ValueError(f"iterations: an int in 0 ... {GUIDED_MAX_ITERATIONS}, got {iterations!r}")
    for name, v in (("sigma_l", sigma_l), ("var_eps", var_eps), ("k_normal", k_normal), ("k_depth", k_depth)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name}: a finite number >= 0, got {v!r}")
    if not var_eps > 0:
        raise ValueError("var_eps must be > 0")
    return tuple(n for n in GUIDED_PLANES if n in names), outs


def check_regression(samples: int, planes: Sequence[str] = (), outputs: Sequence[str] = ("rgb",), ridge: float = RIDGE,
                     albedo_eps: Optional[float] = None) -> tuple:
    """The checks of resolve_regression's arguments, all of them ValueError and none of them a GPU call.  planes: the names of the
    planes given (index is ignored).  Returns (planes, outputs) as tuples, the planes in FEATURE_PLANES' order.  Pure: no torch, no
    GPU."""
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
        raise ValueError(f"the film holds {samples!r} samples: a fit needs at least 1")
    outs = tuple(outputs)
    if not outs or any(o not in REGRESSION_OUTPUTS for o in outs) or len(set(outs)) != len(outs):
        raise ValueError(f"outputs: a non-empty subset of {REGRESSION_OUTPUTS}, got {outs}")
    names = tuple(n for n in planes if n != "index")
    if any(n not in FEATURE_PLANES for n in names):
        raise ValueError(f"planes: a subset of {FEATURE_PLANES}, got {names}")
    if "depth" in names and "hits" not in names:
        raise ValueError("planes: the depth plane needs the hits plane")
    for name, v in (("ridge", ridge),) + ((("albedo_eps", albedo_eps),) if albedo_eps is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name}: a finite number > 0, got {v!r}")
        as_f32 = ctypes.c_float(v).value
        if not (as_f32 > 0 and math.isfinite(as_f32)):
            raise ValueError(f"{name}: finite and > 0 as a float32, got {v!r}")
    return tuple(n for n in FEATURE_PLANES if n in names), outs


def regression_nodes(width: int, rows: int) -> tuple:
    """(NY, NX) of the regression resolve's nodes on a width x rows image: one every 16 pixels, and one past each edge.  Pure."""
    if width < 1 or rows < 1:
        raise ValueError("width and rows must be at least 1")
    return (rows - 1) // REGRESSION_PITCH + 2, (width - 1) // REGRESSION_PITCH + 2


def _add_stats(total: TileStats, st: TileStats) -> None:
    for f in _SUMMED_STATS:
        setattr(total, f, getattr(total, f) + getattr(st, f))
    if st.n_launches:
        total.engine, total.broad_form = st.engine, st.broad_form


class Film:
    """The running colour sum of one frame on the device, and the calls that fill, inspect and denoise it.

        with rt.Film(scene, strips, integrator="nee") as film:
            for samples in film.render_progressive(4):
                rgb = film.preview()["rgb"]                      # (R, W, 3) uint8 on the device, after `samples` samples
            planes = film.features(1)
            out = film.resolve(planes=planes, outputs=("rgb",))
            film.sync()
            image = out["rgb"].cpu().numpy()

    accum: one (R, W, 3) float32 tensor, strip i in rows [i Hs, (i + 1) Hs); samples: the samples folded so far.  The camera, the
    light sampling and the glossy sampling are the scene's settings at the moment a pass is enqueued.

    Streams.  Everything the film enqueues, its torch ops and the library's kernels alike, goes to ONE stream, Film.stream: its own
    torch.cuda.Stream on the scene's device, or the caller's.  A stream whose handle is 0 is refused: to the library 0 means the scene's
    own non-blocking stream, to torch the default stream, and the two are not ordered with each other.  Calls return once the work is
    enqueued.  A consumer on another stream must wait first, torch.cuda.current_stream().wait_stream(film.stream); sync() makes the
    host wait.  The tensors the film returns (accum, the planes, the outputs of resolve) are its own and are written again by the next
    call of the same kind.

    Counters.  collect() returns the summed rt_tile_stats of the film's launches since the last collect().  The film collects from
    the scene by itself into that sum before its uncollected launches could reach the library's limit; a Scene.collect() of the
    caller's own between two calls takes the counters of the film's launches with it.  A Film is not thread-safe, and after an
    RtError its accum is undefined until reset()."""

    _taps: Sequence = ()                          # (the constructor's list; a film put together without it has no tap)

    def __init__(self, scene, reqs, *, integrator: str = "nee", mode: int = _abi.RT_NEE_MIS, flags: int = 0,
                 max_records: int = 1 << 22, stream=None, moments: bool = False, _collect_at: int = COLLECT_AT):
        plan = check_job(reqs, integrator, mode, max_records)
        import torch
        _abi.check_single_hip_runtime()           # torch imported after the library bound its runtime: say so, before any HIP call
        self._film_lib = _film_lib.load() if moments else None        # (after the check: it binds to the same HIP runtime)
        self._torch = torch
        self.scene = scene
        self.integrator, self.mode, self.flags, self.max_records = integrator, mode, flags, max_records
        self.reqs, self.hs, self.width, self.rows, self.spp, self.k = plan
        self.device = torch.device("cuda", scene.device)
        if stream is None:
            stream = torch.cuda.Stream(device=self.device)
        if stream.cuda_stream == 0:
            raise ValueError("stream: handle 0 is the scene's own stream to the library and the default stream to torch, which are "
                             "not ordered with each other: pass a torch.cuda.Stream of its own")
        if stream.device != self.device:
            raise ValueError(f"stream: on {stream.device}, the scene is on {self.device}")
        self.stream = stream
        self._collect_at = _collect_at
        self._uncollected = 0
        self._stats = TileStats()
        self.samples = 0
        self.aov_samples = 0
        self.planes: dict = {}
        self._out: dict = {}
        self._scratch = None
        n = self.hs * self.width * self.k
        with torch.cuda.stream(stream):
            self.accum = torch.zeros((self.rows, self.width, 3), dtype=torch.float32, device=self.device)
            self._rays = torch.empty((n, 8), dtype=torch.float32, device=self.device)
            self._states = torch.empty((n, 4), dtype=torch.int64, device=self.device)
            self._rgb = torch.empty((n, 3), dtype=torch.float32, device=self.device)
            self.moments = torch.zeros((self.rows, self.width, 2), dtype=torch.float32, device=self.device) if moments else None
        self._guided_scratch = None
        self._guided_out: dict = {}
        self.regression_model = None
        self._regression_out: dict = {}
        self._taps: list = []                     # what is shown every strip's records after their fold (film_robust.py)

    # ---- the film's own state

    def _check_open(self):
        if self.accum is None:
            raise ValueError("the film is closed")

    def _reserve(self, launches: int):
        """Room for `launches` more uncollected launches on the scene (an upper bound will do)."""
        if self._uncollected + launches > self._collect_at:
            self._absorb()
        self._uncollected += launches

    def _absorb(self):
        _add_stats(self._stats, self.scene.collect())
        self._uncollected = 0

    def _strip(self, frame, i: int):
        """Strip i of a frame-shaped tensor (a view)."""
        return frame[i * self.hs:(i + 1) * self.hs]

    def collect(self) -> TileStats:
        """Wait for the film's launches and return their summed rt_tile_stats since the last collect() (engine and broad_form: the
        last launch's)."""
        self._check_open()
        self._absorb()
        st, self._stats = self._stats, TileStats()
        return st

    def sync(self):
        """Wait until everything the film enqueued has run."""
        self.stream.synchronize()

    def reset(self, seed: Optional[int] = None):
        """Back to no samples: accum (and moments) are zeroed on the film's stream.  The feature buffers do not depend on it and
        stay.  seed: also the job's seed from here on, set on the film's own copies of the requests (never the caller's), for the
        passes and the features that follow.  A sample's stream depends on (seed, pixel, sample) only: without a new seed a frame
        rendered again under the same camera has the same bytes, and a history of identical frames (rt.FilmHistory) gains nothing."""
        self._check_open()
        if seed is not None:
            if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
                raise ValueError(f"seed: an int in 0 ... 2^64 - 1, got {seed!r}")
            for rq in self.reqs:
                rq.seed = seed
        with self._torch.cuda.stream(self.stream):
            self.accum.zero_()
            if self.moments is not None:
                self.moments.zero_()
            for t in self._taps:
                t._on_reset()
        self.samples = 0

    def close(self):
        """Wait for the film's work and drop its tensors.  The scene stays the caller's."""
        if getattr(self, "accum", None) is None:
            return
        self.sync()
        self.accum = self._rays = self._states = self._rgb = self._scratch = None
        self.moments = self._guided_scratch = self.regression_model = None
        self.planes, self._out, self._guided_out, self._regression_out = {}, {}, {}, {}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- samples

    def _trace(self, n: int, max_bounces: int, handle: int, rays=None, states=None):
        """The film's integrator over the first n records of its ray and state buffers into _rgb.  rays, states: tensors to trace in
        the place of the film's own (film_sampler.py)."""
        rays, states = self._rays if rays is None else rays, self._states if states is None else states
        kw = dict(d_rng_state=states.data_ptr(), spp=1, max_bounces=max_bounces, as_given=True, flags=self.flags, stream=handle)
        if self.integrator == "path":
            self.scene.trace_device(rays.data_ptr(), n, self._rgb.data_ptr(), **kw)
        else:
            self.scene.trace_nee_device(rays.data_ptr(), n, self._rgb.data_ptr(), mode=self.mode, **kw)

    _fold = staticmethod(fold)                    # (tools/film_bench.py times a pass without it by shadowing this on the instance)

    def _fold_moments(self, acc, mom, records):
        """accum and moments of a strip += its records (P, n, 3), in record order: one launch of the film library's fold kernel on the
        film's stream."""
        P, n = records.shape[0], records.shape[1]
        _film_lib.check("rtf_fold_moments", self._film_lib.rtf_fold_moments(records.data_ptr(), P, n, acc.data_ptr(), mom.data_ptr(),
                                                                            self.stream.cuda_stream))

    def render_pass(self, begin: int, end: int):
        """Add samples [begin, end) of the spp-sample job to accum; begin must be `samples`, and begin < end <= spp.  Per strip and
        per sub-range of sample_chunks: the camera's rays and states, the trace from those states with spp = 1, and the fold.  A tap
        in _taps (rt.FilmRobust) is then shown the records the fold just read, on the film's stream: _on_records(strip, b, e, records)
        with records the (pixels, e - b, 3) view.  With no tap nothing more is enqueued."""
        self._check_open()
        if begin != self.samples:
            raise ValueError(f"render_pass({begin}, {end}): the film holds samples [0, {self.samples}), the next pass begins there")
        if not begin < end <= self.spp:
            raise ValueError(f"render_pass({begin}, {end}): need begin < end <= spp = {self.spp}")
        pixels = self.hs * self.width
        chunks = sample_chunks(pixels, begin, end, self.max_records)
        handle = self.stream.cuda_stream
        with self._torch.cuda.stream(self.stream):
            for i, rq in enumerate(self.reqs):
                acc = self._strip(self.accum, i).view(pixels, 3)
                mom = self._strip(self.moments, i).view(pixels, 2) if self.moments is not None else None
                for b, e in chunks:
                    n = pixels * (e - b)
                    self._reserve(2)
                    self.scene.camera_rays_device(rq, b, e, self._rays.data_ptr(), self._states.data_ptr(), stream=handle)
                    self._trace(n, rq.max_bounces, handle)
                    records = self._rgb[:n].view(pixels, e - b, 3)
                    if mom is None:
                        self._fold(acc, records)
                    else:
                        self._fold_moments(acc, mom, records)
                    for t in self._taps:
                        t._on_records(i, b, e, records)
        self.samples = end

    def render_progressive(self, pass_spp: int):
        """Generator: the rest of the job in passes of pass_spp samples (the last may be shorter), yielding `samples` after each."""
        if pass_spp < 1:
            raise ValueError("pass_spp must be at least 1")
        while self.samples < self.spp:
            self.render_pass(self.samples, min(self.samples + pass_spp, self.spp))
            yield self.samples

    # ---- feature buffers and the denoiser

    def _strip_ptrs(self, frame):
        return [self._strip(frame, i).data_ptr() for i in range(len(self.reqs))]

    def _plane_spec(self, name: str) -> tuple:
        """(shape, dtype) of a feature plane: albedo and normal (R, W, 3), the rest (R, W); hits and index int32, the rest float32."""
        shape = (self.rows, self.width, 3) if name in ("albedo", "normal") else (self.rows, self.width)
        return shape, self._torch.int32 if name in ("hits", "index") else self._torch.float32

    def _check_plane(self, name: str, t) -> None:
        """A caller's tensor against _plane_spec: contiguous, on the film's device, of that shape and dtype."""
        shape, dtype = self._plane_spec(name)
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"planes[{name!r}]: need a contiguous {dtype} tensor of shape {shape} on {self.device}, as features() "
                             "returns it")

    def features(self, aov_samples: int = 1, planes: Sequence[str] = FEATURE_PLANES) -> dict:
        """The feature buffers of the frame over samples [0, aov_samples) (rt_scene_render_aovs_device), as frame-shaped tensors laid
        out like accum: albedo and normal (R, W, 3) float32, depth (R, W) float32, hits and index (R, W) int32 holding the uint32
        counts and world positions.  Returns {plane: tensor}; the film keeps it as `planes`, with `aov_samples`."""
        self._check_open()
        torch = self._torch
        names = tuple(planes)
        if not names or any(n not in _abi.AOV_PLANES for n in names):
            raise ValueError(f"planes: a non-empty subset of {_abi.AOV_PLANES}, got {names}")
        if not 1 <= aov_samples <= self.spp:
            raise ValueError(f"aov_samples: need 1 <= aov_samples <= spp = {self.spp}")
        with torch.cuda.stream(self.stream):
            out = {}
            for n in names:
                shape, dtype = self._plane_spec(n)
                t = self.planes.get(n)
                out[n] = t.zero_() if t is not None else torch.zeros(shape, dtype=dtype, device=self.device)
            ptrs = {n: self._strip_ptrs(t) for n, t in out.items()}
            self._reserve(len(self.reqs))
            self.scene.render_aovs_device(self.reqs, 0, aov_samples, [{n: p[i] for n, p in ptrs.items()} for i in range(len(self.reqs))],
                                          stream=self.stream.cuda_stream)
        self.planes, self.aov_samples = out, aov_samples
        return dict(out)

    def _check_planes(self, planes: Optional[dict]) -> dict:
        guide = {}
        for n, t in (planes or {}).items():
            if n == "index" or t is None:
                continue
            if n not in FEATURE_PLANES:
                raise ValueError(f"planes: unknown plane {n!r}")
            self._check_plane(n, t)
            guide[n] = t
        if guide and not self.aov_samples:
            raise ValueError("planes: call features() first, it sets their sample count")
        return guide

    def resolve(self, dreq: Optional[DenoiseRequest] = None, planes: Optional[dict] = None, outputs: Sequence[str] = ("rgb",),
                _state: Optional[tuple] = None) -> dict:
        """The denoiser over all strips as one image (rt_scene_denoise_device) with color_samples = samples.  dreq: None for the
        library's defaults; its sample counts are set here.  planes: the dict features() returned (its sample count is the film's
        aov_samples), a part of it, or None for the plain colour a-trous.  outputs: a non-empty subset of ("rgb", "linear", "f32").
        Returns {output: (R, W, 3) tensor}, uint8 for rgb and float32 otherwise.  _state: (accum, moments) tensors of the film's
        shape to resolve in the place of the film's own (film_history.py)."""
        self._check_open()
        accum = self.accum if _state is None else _state[0]
        torch = self._torch
        outs = tuple(outputs)
        if not outs or any(o not in DENOISE_OUTPUTS for o in outs):
            raise ValueError(f"outputs: a non-empty subset of {DENOISE_OUTPUTS}, got {outs}")
        if self.samples < 1:
            raise ValueError("resolve: the film holds no samples yet")
        guide = self._check_planes(planes)
        dq = DenoiseRequest.defaults() if dreq is None else DenoiseRequest.from_buffer_copy(dreq)
        dq.color_samples, dq.aov_samples = self.samples, max(self.aov_samples, 1)
        n = len(self.reqs)
        with torch.cuda.stream(self.stream):
            if self._scratch is None:
                self._scratch = torch.empty(denoise_scratch_bytes(self.width, self.rows), dtype=torch.uint8, device=self.device)
            for o in outs:
                if o not in self._out:
                    self._out[o] = torch.empty((self.rows, self.width, 3), dtype=torch.uint8 if o == "rgb" else torch.float32,
                                               device=self.device)
            ptrs = {k: self._strip_ptrs(t) for k, t in guide.items()}
            arrays = {o: self._strip_ptrs(self._out[o]) if o in outs else None for o in DENOISE_OUTPUTS}
            self._reserve(2 * n + _abi.RT_DENOISE_MAX_ITERATIONS)
            self.scene.denoise_device(self.reqs, dq, self._strip_ptrs(accum), [{k: p[i] for k, p in ptrs.items()} for i in range(n)],
                                      self._scratch.data_ptr(), self._scratch.numel(), d_rgb=arrays["rgb"], d_f32=arrays["f32"],
                                      d_linear=arrays["linear"], stream=self.stream.cuda_stream)
        return {o: self._out[o] for o in outs}

    def preview(self, outputs: Sequence[str] = ("rgb",)) -> dict:
        """resolve with no iterations and no planes: sqrt(accum / samples), what the tile path's pass shows."""
        return self.resolve(DenoiseRequest.defaults(iterations=0), None, outputs)

    # ---- the variance-guided resolve

    def _guided(self, guide: dict, outs: tuple, iterations: int, sigma_l: float, var_eps: float, k_normal: float, k_depth: float,
                lds_max_step: int, _state: Optional[tuple] = None) -> dict:
        """One rtf_resolve call on the film's stream into the film's own output tensors.  These launches are the film library's, not
        the scene's: they count neither against _reserve nor in collect().  _state: (accum, moments) tensors of the film's shape to
        resolve in the place of the film's own (film_history.py)."""
        torch = self._torch
        accum, moments = (self.accum, self.moments) if _state is None else _state
        with torch.cuda.stream(self.stream):
            if self._guided_scratch is None:
                self._guided_scratch = torch.empty(_film_lib.resolve_scratch_bytes(self.width, self.rows), dtype=torch.uint8,
                                                   device=self.device)
            for o in outs:
                if o not in self._guided_out:
                    shape = (self.rows, self.width) if o == "variance" else (self.rows, self.width, 3)
                    self._guided_out[o] = torch.empty(shape, dtype=torch.uint8 if o == "rgb" else torch.float32, device=self.device)
            ptr = lambda d, k: d[k].data_ptr() if k in d else None
            out = {o: self._guided_out[o] for o in outs}
            a = _film_lib.ResolveArgs(W=self.width, R=self.rows, samples=self.samples, iterations=iterations, lds_max_step=lds_max_step,
                                      sigma_l=sigma_l, var_eps=var_eps, k_normal=k_normal, k_depth=k_depth,
                                      accum=accum.data_ptr(), moments=moments.data_ptr(), normal=ptr(guide, "normal"),
                                      depth=ptr(guide, "depth"), hits=ptr(guide, "hits"), scratch=self._guided_scratch.data_ptr(),
                                      scratch_bytes=self._guided_scratch.numel(), out_rgb=ptr(out, "rgb"), out_f32=ptr(out, "f32"),
                                      out_linear=ptr(out, "linear"), out_variance=ptr(out, "variance"))
            _film_lib.check("rtf_resolve", self._film_lib.rtf_resolve(a, self.stream.cuda_stream))
        return out

    def variance(self):
        """v0 of every pixel, the variance of the mean of y over the samples folded so far, as an (R, W) float32 tensor (the film's
        own: the next variance() or resolve_guided(outputs=("variance", ...)) writes it again).  Needs moments=True and samples >= 2."""
        self._check_open()
        check_guided(self.moments is not None, self.samples, (), ("variance",), 0)
        return self._guided({}, ("variance",), 0, SIGMA_L, VAR_EPS, 0.0, 0.0, _film_lib.LDS_PLAN)["variance"]

    def resolve_guided(self, planes: Optional[dict] = None, outputs: Sequence[str] = ("rgb",), iterations: int = 5,
                       sigma_l: float = SIGMA_L, var_eps: float = VAR_EPS, k_normal: Optional[float] = None,
                       k_depth: Optional[float] = None, _lds_max_step: int = _film_lib.LDS_PLAN,
                       _state: Optional[tuple] = None) -> dict:
        """The variance-guided a-trous over all strips as one image (rtf_resolve): the colour edge-stop of each pixel
        is scaled by its prefiltered variance of the mean, which the iterations carry along.  planes: a part of what features()
        returned out of normal, depth (needs hits) and hits, or None; index is ignored and albedo refused (no demodulation here).
        outputs: a non-empty subset of ("rgb", "linear", "f32", "variance").  k_normal, k_depth: None for DenoiseRequest.defaults()'s.
        Returns {output: tensor} in resolve()'s layout, variance as (R, W) float32.  Needs moments=True and samples >= 2.  _state: as
        resolve()'s."""
        self._check_open()
        given = {n: t for n, t in (planes or {}).items() if t is not None}
        if k_normal is None or k_depth is None:
            dq = DenoiseRequest.defaults()
            k_normal = dq.k_normal if k_normal is None else k_normal
            k_depth = dq.k_depth if k_depth is None else k_depth
        names, outs = check_guided(self.moments is not None, self.samples, tuple(given), outputs, iterations, sigma_l, var_eps,
                                   k_normal, k_depth)
        guide = self._check_planes({n: given[n] for n in names})
        return self._guided(guide, outs, iterations, float(sigma_l), float(var_eps), float(k_normal), float(k_depth), _lds_max_step,
                            _state)

    # ---- the regression resolve

    def resolve_regression(self, planes: Optional[dict] = None, outputs: Sequence[str] = ("rgb",), ridge: float = RIDGE,
                           albedo_eps: Optional[float] = None, _state: Optional[tuple] = None) -> dict:
        """The local feature regression over all strips as one image (rtf_resolve, kind 1): around a node every 16
        pixels the colour is fitted, over a 32 x 32 window, as a linear function of eight features of the planes (1, the unit normal,
        the window's normalised depth and its square, the position in the window), by ridge-regularised least squares, and a pixel
        takes the bilinear blend of its four nodes' fits.  planes: what features() returned or a part of it out of albedo (the colour
        is then fitted demodulated), normal, depth (needs hits) and hits, or None; index is ignored.  outputs: a non-empty subset of
        ("rgb", "linear", "f32").  albedo_eps: None for DenoiseRequest.defaults()'s.  Returns {output: tensor} in resolve()'s layout:
        the film's own tensors, written again by the next call, as regression_model is, the (NY, NX, 32) float32 records of the fit.
        Needs samples >= 1; works without moments (the film library is loaded here if the film did not load it).  _state: as
        resolve()'s (its moments are not read)."""
        self._check_open()
        torch = self._torch
        given = {n: t for n, t in (planes or {}).items() if t is not None}
        names, outs = check_regression(self.samples, tuple(given), outputs, ridge, albedo_eps)
        guide = self._check_planes({n: given[n] for n in names})
        if albedo_eps is None:
            albedo_eps = DenoiseRequest.defaults().albedo_eps
        accum = self.accum if _state is None else _state[0]
        if self._film_lib is None:
            self._film_lib = _film_lib.load()
        NY, NX = regression_nodes(self.width, self.rows)
        with torch.cuda.stream(self.stream):
            if self.regression_model is None:
                self.regression_model = torch.zeros((NY, NX, REGRESSION_RECORD), dtype=torch.float32, device=self.device)
            for o in outs:
                if o not in self._regression_out:
                    self._regression_out[o] = torch.empty((self.rows, self.width, 3), dtype=torch.uint8 if o == "rgb" else torch.float32,
                                                          device=self.device)
            ptr = lambda d, k: d[k].data_ptr() if k in d else None
            out = {o: self._regression_out[o] for o in outs}
            model = self.regression_model
            a = _film_lib.ResolveArgs(W=self.width, R=self.rows, samples=self.samples, kind=_film_lib.RESOLVE_REGRESS,
                                      accum=accum.data_ptr(), normal=ptr(guide, "normal"), depth=ptr(guide, "depth"),
                                      hits=ptr(guide, "hits"), out_rgb=ptr(out, "rgb"), out_f32=ptr(out, "f32"),
                                      out_linear=ptr(out, "linear"), albedo=ptr(guide, "albedo"),
                                      aov_samples=self.aov_samples if guide else 0, albedo_eps=float(albedo_eps), ridge=float(ridge),
                                      model=model.data_ptr(), model_bytes=model.numel() * 4)
            _film_lib.check("rtf_resolve", self._film_lib.rtf_resolve(a, self.stream.cuda_stream))
        return out
