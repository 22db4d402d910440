"""Full-resolution frames from a low-resolution film: joint-bilateral upsampling of a linear image of rt.Film, with the edges taken
from feature buffers rendered at both resolutions.

    with rt.Film(scene, strips_lo, integrator="nee") as film, rt.FilmUpsampler(film, strips_hi) as up:
        film.render_pass(0, film.spp)                      # the lit film: a quarter (s = 2) or a ninth (s = 3) of the records
        film.features(1, rt.film_upsampler.PLANES)         # the low-resolution feature buffers, index among them
        up.features(1)                                     # the full-resolution ones: one sample of the tile engines
        rgb = up.resolve("resolve", planes=film.planes)["rgb"]     # (s R, s W, 3) uint8

The feature buffers cost a fraction of a film pass (they come from the tile engines), so the lit film is rendered at a half to a
quarter of the resolution and the frame reconstructed at the full one: every output pixel takes the 2 x 2 bilinear footprint of its
position in the low film and admits only the taps that show the same primitive (index), hit or miss alike (hits), at about the same
distance (depth) under about the same normal; a pixel with no admitted tap falls back to plain bilinear and says so in the class
plane.  With the albedo planes the low-resolution colour is divided by its albedo before the taps are weighted and multiplied by the
full-resolution albedo after, so texture and primitive boundaries come back at the full resolution.

The arithmetic is normative in upsample_csrc/rt_upsample.h and runs in one HIP kernel of a private library (lib/librt_upsample.so,
_upsample_lib.py).  This module imports without torch; the library is loaded when a FilmUpsampler is constructed."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence

from . import _upsample_lib
from ._abi import DenoiseRequest, TileRequest
from .film import check_job

PLANES = _upsample_lib.PLANES                     # ("albedo", "normal", "depth", "hits", "index")
OUTPUTS = ("rgb", "linear", "f32", "class")
SOURCES = ("resolve", "guided", "preview")
MIN_SCALE, MAX_SCALE = _upsample_lib.MIN_SCALE, _upsample_lib.MAX_SCALE
# what the two frames of one camera agree on
CAMERA_FIELDS = ("fov", "focal_length", "aperture", "focus_distance")
# The defaults.  k_depth: a tap whose distance is within a tenth of the pixel's, the history's K_DEPTH.  k_normal: the least cosine
# between the two normals, about 25 degrees.  (The denoiser's k_normal and k_depth are slopes of its Tukey weight, not a cosine and a
# relative distance: as thresholds here, 1 would reject every tap of a curved surface and 4 admit every distance.)  eps: None takes
# DenoiseRequest.defaults().albedo_eps, the albedo's eps of the denoiser.
K_DEPTH = 0.1
K_NORMAL = 0.9


class UpsamplePlan(NamedTuple):
    """What check_upsample makes of its arguments: the scale, the strips of the full-resolution frame (copies), its width, the rows
    of the output and of the full frame, the first global row on each side, the planes of a call in PLANES' order, and the constants."""
    scale: int
    reqs_hi: tuple
    width: int
    rows: int
    height: int
    y0_lo: int
    y0_hi: int
    planes: tuple
    k_depth: float
    k_normal: float
    eps: float


def _strips(reqs) -> list:
    strips = [reqs] if isinstance(reqs, TileRequest) else list(reqs or ())
    if not strips or any(not isinstance(r, TileRequest) for r in strips):
        raise ValueError("reqs: one TileRequest or a non-empty sequence of them")
    return strips


def check_planes(planes_lo: Sequence[str] = (), planes_hi: Sequence[str] = (), use_index: bool = True, albedo: bool = True) -> tuple:
    """The plane set of a call from the names given on each side: ValueError for an unknown plane, a plane on one side only, or depth
    without hits.  albedo=False and use_index=False leave those planes out.  Returns the names in PLANES' order.  Pure."""
    lo, hi = tuple(planes_lo), tuple(planes_hi)
    for side, names in (("planes_lo", lo), ("planes_hi", hi)):
        if any(n not in PLANES for n in names) or len(set(names)) != len(names):
            raise ValueError(f"{side}: a subset of {PLANES}, got {names}")
    skip = (() if albedo else ("albedo",)) + (() if use_index else ("index",))
    lo, hi = {n for n in lo if n not in skip}, {n for n in hi if n not in skip}
    if lo != hi:
        raise ValueError(f"planes: {sorted(lo ^ hi)} given on one side only; a plane steers the taps only with both resolutions of it")
    if "depth" in lo and "hits" not in lo:
        raise ValueError("planes: the depth plane needs the hits plane")
    return tuple(n for n in PLANES if n in lo)


def check_upsample(reqs_lo, reqs_hi, planes_lo: Sequence[str] = (), planes_hi: Sequence[str] = (), outputs: Sequence[str] = ("rgb",),
                   use_index: bool = True, k_depth: float = K_DEPTH, k_normal: float = K_NORMAL, eps: float = 2.0 ** -8,
                   albedo: bool = True) -> UpsamplePlan:
    """The checks of FilmUpsampler's and upsample()'s arguments, all of them ValueError and none of them a GPU call.  reqs_lo: the
    strips of the low-resolution film; reqs_hi: the strips of the full-resolution frame, each a frame as film.check_job takes it.  The
    full frame is s times the low one in both directions, s an integer in 2 ... 4, under the same camera fields, and its strips cover
    exactly the rows the film's cover.  planes_lo, planes_hi: the names of the planes given on each side.  Pure: no torch, no GPU."""
    lo = check_job(_strips(reqs_lo), max_records=1 << 62)
    hi = check_job(_strips(reqs_hi), max_records=1 << 62)
    l0, h0 = lo.reqs[0], hi.reqs[0]
    s = h0.width // l0.width
    if h0.width != s * l0.width or h0.height != s * l0.height or not MIN_SCALE <= s <= MAX_SCALE:
        raise ValueError(f"reqs_hi: {h0.width} x {h0.height} is not s times the film's {l0.width} x {l0.height} with an integer s in "
                         f"{MIN_SCALE} ... {MAX_SCALE}")
    differ = [f for f in CAMERA_FIELDS if getattr(l0, f) != getattr(h0, f)]
    if differ:
        raise ValueError(f"reqs_hi differs from the film's strips in {differ}: both frames are one camera's")
    y0_lo, y0_hi = l0.division_no * lo.hs, h0.division_no * hi.hs
    if y0_hi != s * y0_lo or hi.rows != s * lo.rows:
        raise ValueError(f"reqs_hi covers rows [{y0_hi}, {y0_hi + hi.rows}) of its frame, the film rows [{y0_lo}, {y0_lo + lo.rows}): "
                         f"need the film's rows times {s}")
    if hi.rows * hi.width > (1 << 31) - 1:
        raise ValueError("reqs_hi: more than 2^31 - 1 output pixels")
    outs = tuple(outputs)
    if not outs or any(o not in OUTPUTS for o in outs) or len(set(outs)) != len(outs):
        raise ValueError(f"outputs: a non-empty subset of {OUTPUTS}, got {outs}")
    for name, v in (("k_depth", k_depth), ("k_normal", k_normal), ("eps", eps)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name}: a finite number >= 0, got {v!r}")
    if not eps > 0:
        raise ValueError(f"eps: need eps > 0, got {eps!r}")
    if not isinstance(use_index, bool) or not isinstance(albedo, bool):
        raise ValueError("use_index and albedo: bools")
    names = check_planes(planes_lo, planes_hi, use_index, albedo)
    return UpsamplePlan(s, hi.reqs, hi.width, hi.rows, h0.height, y0_lo, y0_hi, names, float(k_depth), float(k_normal), float(eps))


class FilmUpsampler:
    """The full-resolution side of one low-resolution film: the feature buffers of the full frame, the output tensors, and the call
    that upsamples a linear image of the film into them.

    film: the low-resolution rt.Film.  reqs_hi: the strips of the full-resolution frame, s times the film's frame in both directions
    (s = 2, 3 or 4), covering the film's rows, with the film's camera fields.  use_index=False leaves the index planes out of every
    call.  k_depth: the relative distance within which a tap is admitted; k_normal: the least cosine between its normal and the
    pixel's; eps: the albedo's eps (None: the module's K_DEPTH and K_NORMAL and the denoiser's albedo_eps).

    What the caller owes.  Both feature sets (film.features and features() here) and the film's passes are rendered under the same
    scene camera: the upsampler cannot know under which camera a plane was enqueued.  Everything is enqueued on film.stream, the
    scene's launches counting against the film's own reserve of uncollected launches; a consumer on another stream must wait first,
    torch.cuda.current_stream().wait_stream(film.stream).  The tensors returned are the upsampler's own and are written again by the
    next call of the same kind.  Not thread-safe."""

    def __init__(self, film, reqs_hi, *, use_index: bool = True, k_depth: Optional[float] = None, k_normal: Optional[float] = None,
                 eps: Optional[float] = None):
        if film is None or not hasattr(film, "reqs"):
            raise ValueError("film: an rt.Film")
        if eps is None:
            eps = DenoiseRequest.defaults().albedo_eps
        self.plan = check_upsample(film.reqs, reqs_hi, use_index=use_index, k_depth=K_DEPTH if k_depth is None else k_depth,
                                   k_normal=K_NORMAL if k_normal is None else k_normal, eps=eps)
        film._check_open()
        if film.stream.cuda_stream == 0:
            raise ValueError("film.stream: handle 0 is the scene's own stream to the library and the default stream to torch")
        self._lib = _upsample_lib.load()
        self.film = film
        self.use_index = use_index
        self.scale, self.reqs_hi, self.width, self.rows = self.plan.scale, self.plan.reqs_hi, self.plan.width, self.plan.rows
        self.hs = self.rows // len(self.reqs_hi)
        self.k_depth, self.k_normal, self.eps = self.plan.k_depth, self.plan.k_normal, self.plan.eps
        self.planes_hi: dict = {}
        self.aov_samples_hi = 0
        self._out: Optional[dict] = {}

    # ---- state

    def _check_open(self):
        if self._out is None:
            raise ValueError("the upsampler is closed")
        self.film._check_open()
        if self.film.stream.cuda_stream == 0:
            raise ValueError("film.stream: handle 0 is the scene's own stream to the library and the default stream to torch")

    def close(self):
        """Wait for the film's stream and drop the upsampler's tensors.  The film stays the caller's."""
        if getattr(self, "_out", None) is None:
            return
        if self.film.accum is not None:
            self.film.sync()
        self._out = None
        self.planes_hi = {}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _plane_spec(self, name: str) -> tuple:
        torch = self.film._torch
        shape = (self.rows, self.width, 3) if name in ("albedo", "normal") else (self.rows, self.width)
        return shape, torch.int32 if name in ("hits", "index") else torch.float32

    def _check_plane(self, name: str, t) -> None:
        shape, dtype = self._plane_spec(name)
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != self.film.device or not t.is_contiguous():
            raise ValueError(f"planes_hi[{name!r}]: need a contiguous {dtype} tensor of shape {shape} on {self.film.device}, as "
                             "features() returns it")

    # ---- the full-resolution feature buffers

    def features(self, aov_samples: int = 1, planes: Sequence[str] = PLANES) -> dict:
        """The feature buffers of the full-resolution frame over samples [0, aov_samples) (rt_scene_render_aovs_device over reqs_hi),
        as frame-shaped tensors laid out like the film's: albedo and normal (s R, s W, 3) float32, depth (s R, s W) float32, hits and
        index (s R, s W) int32.  Returns {plane: tensor}; the upsampler keeps it as `planes_hi`, with `aov_samples_hi`.  The
        low-resolution planes are the film's own film.features(...)."""
        self._check_open()
        film, torch = self.film, self.film._torch
        names = tuple(planes)
        if not names or any(n not in PLANES for n in names) or len(set(names)) != len(names):
            raise ValueError(f"planes: a non-empty subset of {PLANES}, got {names}")
        spp = self.reqs_hi[0].spp
        if isinstance(aov_samples, bool) or not isinstance(aov_samples, int) or not 1 <= aov_samples <= spp:
            raise ValueError(f"aov_samples: need 1 <= aov_samples <= spp = {spp} of reqs_hi")
        n = len(self.reqs_hi)
        with torch.cuda.stream(film.stream):
            out = {}
            for name in names:
                shape, dtype = self._plane_spec(name)
                t = self.planes_hi.get(name)
                out[name] = t.zero_() if t is not None else torch.zeros(shape, dtype=dtype, device=film.device)
            ptrs = [{name: t[i * self.hs:(i + 1) * self.hs].data_ptr() for name, t in out.items()} for i in range(n)]
            film._reserve(n)
            film.scene.render_aovs_device(self.reqs_hi, 0, aov_samples, ptrs, stream=film.stream.cuda_stream)
        self.planes_hi, self.aov_samples_hi = out, aov_samples
        return dict(out)

    # ---- the kernel

    def upsample(self, linear, planes_lo: Optional[dict] = None, planes_hi: Optional[dict] = None, outputs: Sequence[str] = ("rgb",),
                 albedo: bool = True) -> dict:
        """One rtu_upsample call on the film's stream.  linear: an (R, W, 3) float32 tensor on the film's device, a linear image of
        the film (the "linear" output of a resolve of the film or of a history of it).  planes_lo: the low-resolution planes, None for
        the film's own (film.planes), {} for none; planes_hi: the full-resolution ones, None for planes_hi of features().  The planes
        of the call are those given on both sides (a plane on one side only is refused), without the albedo when albedo=False and
        without the index when the upsampler was made with use_index=False; no planes at all is plain bilinear.  Their sample counts are
        film.aov_samples and aov_samples_hi.  outputs: a non-empty subset of ("rgb", "linear", "f32", "class").  Returns {output:
        tensor}: (s R, s W, 3) uint8 for rgb, float32 for linear and f32, (s R, s W) uint8 for class, 1 where no tap was admitted and
        the pixel is the bilinear one.  A refused call (ValueError, or _upsample_lib.RtuError) writes nothing."""
        self._check_open()
        film, torch = self.film, self.film._torch
        lo = {n: t for n, t in (film.planes if planes_lo is None else planes_lo).items() if t is not None}
        hi = {n: t for n, t in (self.planes_hi if planes_hi is None else planes_hi).items() if t is not None}
        plan = check_upsample(film.reqs, self.reqs_hi, tuple(lo), tuple(hi), outputs, self.use_index, self.k_depth, self.k_normal,
                              self.eps, albedo)
        outs = tuple(outputs)
        shape = (film.rows, film.width, 3)
        if (not isinstance(linear, torch.Tensor) or tuple(linear.shape) != shape or linear.dtype != torch.float32 or
                linear.device != film.device or not linear.is_contiguous()):
            raise ValueError(f"linear: need a contiguous float32 tensor of shape {shape} on {film.device}")
        for n in plan.planes:
            film._check_plane(n, lo[n])
            self._check_plane(n, hi[n])
        if plan.planes and not (film.aov_samples and self.aov_samples_hi):
            raise ValueError("planes: call film.features() and features() first, they set the planes' sample counts")
        ptr = lambda d, n: d[n].data_ptr() if n in plan.planes else None
        side = lambda d, k: _upsample_lib.Planes(**{n: ptr(d, n) for n in PLANES}, samples=max(k, 1))
        with torch.cuda.stream(film.stream):
            for o in outs:
                if o not in self._out:
                    oshape = (self.rows, self.width) if o == "class" else (self.rows, self.width, 3)
                    self._out[o] = torch.empty(oshape, dtype=torch.float32 if o in ("linear", "f32") else torch.uint8, device=film.device)
            out = {o: self._out[o] for o in outs}
            optr = lambda o: out[o].data_ptr() if o in out else None
            a = _upsample_lib.UpsampleArgs(Wl=film.width, Rl=film.rows, Hl=film.reqs[0].height, y0l=plan.y0_lo, Wh=self.width,
                                           Rh=self.rows, Hh=plan.height, y0h=plan.y0_hi, scale=plan.scale, k_depth=plan.k_depth,
                                           k_normal=plan.k_normal, eps=plan.eps, linear=linear.data_ptr(),
                                           lo=side(lo, film.aov_samples), hi=side(hi, self.aov_samples_hi), out_linear=optr("linear"),
                                           out_f32=optr("f32"), out_rgb=optr("rgb"), out_class=optr("class"))
            _upsample_lib.check("rtu_upsample", self._lib.rtu_upsample(a, film.stream.cuda_stream))
        return out

    def resolve(self, source: str = "resolve", outputs: Sequence[str] = ("rgb",), albedo: bool = True, **kw) -> dict:
        """The film's "linear" image by one of its resolves, upsampled: film.resolve(**kw), film.resolve_guided(**kw) or
        film.preview() for source "resolve", "guided" or "preview", then upsample() with the film's planes and planes_hi.  A
        convenience over upsample(); a history's "linear" goes through upsample() directly."""
        self._check_open()
        if source not in SOURCES:
            raise ValueError(f"source: one of {SOURCES}, got {source!r}")
        if "outputs" in kw:
            raise ValueError("outputs are the upsampler's; the film is asked for its linear image")
        check_upsample(self.film.reqs, self.reqs_hi, outputs=outputs)
        if source == "resolve":
            linear = self.film.resolve(outputs=("linear",), **kw)["linear"]
        elif source == "guided":
            linear = self.film.resolve_guided(outputs=("linear",), **kw)["linear"]
        else:
            if kw:
                raise ValueError("preview takes no arguments")
            linear = self.film.preview(("linear",))["linear"]
        return self.upsample(linear, outputs=outputs, albedo=albedo)
