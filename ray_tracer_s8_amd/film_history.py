"""Temporal accumulation for rt.Film: the last frame's colour sums, moments and history length, reprojected into the current frame by
its depth and the two camera poses, and blended with the current frame's.

    with rt.Film(scene, strips, integrator="nee", moments=True) as film, rt.FilmHistory(film) as history:
        for i, camera in enumerate(path):
            scene.set_camera(camera)
            film.reset(seed=seed0 + i)                      # a seed per frame: see Film.reset
            film.render_pass(0, film.spp)
            planes = film.features(1, ("normal", "depth", "hits", "index"))
            history.accumulate(camera, planes)
            rgb = history.resolve_guided(planes)["rgb"]

The arithmetic is normative in history_csrc/rt_history.h and runs in one HIP kernel of a private library (lib/librt_history.so,
_history_lib.py).  What the history holds are sums at the film's sample count, like the film's own accum and moments, so the film's
resolves run on them unchanged; every frame of a history therefore has the same film.samples.  The world is static: only the
camera moves.  FilmHistory(film, clip=g) also clips the reprojected colours to the current frame's colour box before the blend
(DESIGN.md 4.26); it is off by default.

This module imports without torch; the library is loaded when a FilmHistory is constructed."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

from . import _film_lib, _history_lib
from ._abi import Camera, DenoiseRequest
from .film import SIGMA_L, VAR_EPS, check_guided

# The defaults (DESIGN.md 4.24 "Defaults"), from the grid of tools/film_history_bench.py on the c2 and c3 orbits.  alpha: the least error
# of {0.05, 0.1, 0.2, 0.5} on three of the four orbits, as a mean and through resolve_guided; the reprojected history carries bias
# (mirrors, resampling blur) that a longer memory keeps.  Under a still or slow camera a smaller alpha averages more frames.  n_max:
# with alpha >= 1/2 it only caps the length reported.  k_depth: a tap whose stored distance is within a tenth of the reprojected one.
ALPHA = 0.5
N_MAX = 32
K_DEPTH = 0.1
REQUIRED_PLANES = ("depth", "hits", "index")
OUTPUTS = ("accum", "moments", "length")


def check_history(moments: bool, alpha: float = ALPHA, n_max: float = N_MAX, k_depth: float = K_DEPTH,
                  k_normal: Optional[float] = None) -> tuple:
    """The checks of FilmHistory's arguments, all of them ValueError and none of them a GPU call.  moments: whether the film was made
    with moments=True.  Returns (alpha, n_max, k_depth, k_normal) as floats, k_normal None for a history without normals.  Pure: no
    torch, no GPU."""
    if not moments:
        raise ValueError("a history needs a film made with moments=True")
    for name, v in (("alpha", alpha), ("n_max", n_max), ("k_depth", k_depth)) + ((("k_normal", k_normal),) if k_normal is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name}: a finite number >= 0, got {v!r}")
    if not 0 < alpha <= 1:
        raise ValueError(f"alpha: need 0 < alpha <= 1, got {alpha!r}")
    if not n_max >= 1:
        raise ValueError(f"n_max: need n_max >= 1, got {n_max!r}")
    return float(alpha), float(n_max), float(k_depth), None if k_normal is None else float(k_normal)


def check_clip(clip: Optional[float] = None, clip_radius: int = 1) -> tuple:
    """The checks of FilmHistory's clip arguments: ValueError, and no GPU call.  Returns (gamma, radius): (0.0, 0) for clip=None, the
    history without the clip; otherwise clip is a finite number > 0, the half-width of the colour box in standard deviations of the
    window, and clip_radius 1 or 2, the window's radius in pixels.  Pure: no torch, no GPU."""
    if clip is None:
        return 0.0, 0
    if isinstance(clip, bool) or not isinstance(clip, (int, float)) or not math.isfinite(clip) or not clip > 0:
        raise ValueError(f"clip: None or a finite number > 0, got {clip!r}")
    if isinstance(clip_radius, bool) or not isinstance(clip_radius, int) or clip_radius not in (1, 2):
        raise ValueError(f"clip_radius: 1 or 2, got {clip_radius!r}")
    return float(clip), int(clip_radius)


class FilmHistory:
    """The history of one film: two sets of state planes on the film's device, alternated frame by frame, and the calls that fill and
    resolve them.

    accumulate(camera, planes) takes the film's accum and moments as they stand and the feature buffers of the same frame.  A pixel
    takes history from the 2 x 2 bilinear footprint of where its surface point lay in the previous frame; a tap is admitted only if it
    shows the same primitive at about the same distance (and, with k_normal, under about the same normal).  A pixel with no admitted
    tap starts again from the current frame alone, with length 1.  k_normal: the least cosine between the two frames' normals, or
    None to leave the normals out.

    clip: None, or g > 0 to clip the reprojected colour of every pixel, before the blend, to mean +- g standard deviations of the
    current frame's colours in the (2 clip_radius + 1)^2 window around it (rt_history.h step 5a): history the frame
    does not support (a highlight that moved, a surface uncovered) is pulled to what it does support, at the price of a bias
    towards the frame's own noise where the box is narrow.  The history then keeps one more (R, W) plane, clip_amount: by how much
    each pixel's history was moved, summed over the channels, in the frame accumulated last.

    Everything is enqueued on film.stream; the tensors returned are the history's own and are written again two frames later.  The
    resolves write the film's output tensors.  Not thread-safe."""

    def __init__(self, film, alpha: float = ALPHA, n_max: float = N_MAX, k_depth: float = K_DEPTH, k_normal: Optional[float] = None,
                 clip: Optional[float] = None, clip_radius: int = 1):
        self.alpha, self.n_max, self.k_depth, self.k_normal = check_history(getattr(film, "moments", None) is not None, alpha, n_max,
                                                                            k_depth, k_normal)
        self.clip, self.clip_radius = check_clip(clip, clip_radius)
        self._clip_form = 0                       # the library's choice; tests and tools set a _history_lib.CLIP_FORM_*
        film._check_open()
        self._lib = _history_lib.load()
        self.film = film
        torch = film._torch
        R, W = film.rows, film.width
        shapes = {"accum": ((R, W, 3), torch.float32), "moments": ((R, W, 2), torch.float32), "length": ((R, W), torch.float32),
                  "depth": ((R, W), torch.float32), "index": ((R, W), torch.int32)}
        if self.k_normal is not None:
            shapes["normal"] = ((R, W, 3), torch.float32)
        with torch.cuda.stream(film.stream):
            self._sets = [{n: torch.zeros(s, dtype=d, device=film.device) for n, (s, d) in shapes.items()} for _ in range(2)]
            self._clip_amount = torch.zeros((R, W), dtype=torch.float32, device=film.device) if self.clip else None
        self._cur: Optional[int] = None           # the set the last frame wrote
        self._request = self._camera = None       # the last frame's first strip and camera
        self._samples = 0
        self.frames = 0

    # ---- state

    def _check_open(self):
        if self._sets is None:
            raise ValueError("the history is closed")
        self.film._check_open()

    def _state(self) -> tuple:
        self._check_open()
        if self._cur is None:
            raise ValueError("the history holds no frame yet: call accumulate() first")
        s = self._sets[self._cur]
        return s["accum"], s["moments"]

    @property
    def accum(self):
        return self._state()[0]

    @property
    def moments(self):
        return self._state()[1]

    @property
    def length(self):
        """N of every pixel, the frames its history spans (clamped at n_max), as an (R, W) float32 tensor."""
        self._state()
        return self._sets[self._cur]["length"]

    @property
    def clip_amount(self):
        """Of a history with clip: by how much the last frame's clip moved each pixel's history (the sum over the channels of the
        absolute change of the colour sums; 0 where nothing was clipped or there was no history), as an (R, W) float32 tensor."""
        self._state()
        if self._clip_amount is None:
            raise ValueError("the history was made without clip")
        return self._clip_amount

    def reset(self):
        """Forget the history: the next frame is a first frame.  Nothing is enqueued."""
        self._check_open()
        self._cur = self._request = self._camera = None
        self._samples = 0
        self.frames = 0

    def close(self):
        """Wait for the film's stream and drop the state.  The film stays the caller's."""
        if getattr(self, "_sets", None) is None:
            return
        if self.film.accum is not None:
            self.film.sync()
        self._sets = self._clip_amount = None
        self._cur = self._request = self._camera = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- a frame

    def _check_planes(self, planes) -> dict:
        names = REQUIRED_PLANES + (("normal",) if self.k_normal is not None else ())
        given = planes or {}
        missing = [n for n in names if given.get(n) is None]
        if missing:
            raise ValueError(f"planes: need {names} as film.features() returns them, {missing} missing")
        for n in names:
            self.film._check_plane(n, given[n])
        return {n: given[n] for n in names}

    def accumulate(self, camera: Optional[Camera], planes: dict) -> dict:
        """One frame into the history (rth_accumulate): the film's accum and moments as they stand, under `camera`, the rt.Camera the
        frame's passes and features were enqueued under (None: the reference camera; the film cannot know it, so the caller states
        it), with the feature buffers `planes` of the same frame: depth, hits and index, and normal when the history has a k_normal.
        Returns {"accum", "moments", "length"}: (R, W, 3), (R, W, 2) and (R, W) float32 tensors of the history's, and with clip also
        "clip": the (R, W) clip_amount.  A refused call
        (ValueError, or _history_lib.RthError for a pose the library refuses) leaves the history as it was."""
        self._check_open()
        film = self.film
        if camera is not None and not isinstance(camera, Camera):
            raise ValueError("camera: an rt.Camera or None")
        if film.samples < 1:
            raise ValueError("accumulate: the film holds no samples yet")
        if self._cur is not None and film.samples != self._samples:
            raise ValueError(f"accumulate: the film holds {film.samples} samples, the history's frames {self._samples}: every frame of "
                             "a history has the same sample count (reset() starts another)")
        given = self._check_planes(planes)
        request = film.reqs[0].copy()
        cam = None if camera is None else Camera.from_buffer_copy(camera)
        nxt = 0 if self._cur is None else self._cur ^ 1
        ptr = lambda d, n: d[n].data_ptr() if n in d else None
        state = lambda d: _history_lib.State(**{n: ptr(d, n) for n in ("accum", "moments", "length", "depth", "index", "normal")})
        a = _history_lib.AccumulateArgs(W=film.width, R=film.rows, have_prev=0 if self._cur is None else 1, alpha=self.alpha,
                                        n_max=self.n_max, k_depth=self.k_depth, k_normal=self.k_normal or 0.0,
                                        accum=film.accum.data_ptr(), moments=film.moments.data_ptr(), depth=given["depth"].data_ptr(),
                                        hits=given["hits"].data_ptr(), index=given["index"].data_ptr(), normal=ptr(given, "normal"),
                                        next=state(self._sets[nxt]))
        a.samples = film.samples
        if self.clip:
            a.clip_gamma, a.clip_radius, a.clip_form = self.clip, self.clip_radius, self._clip_form
            a.clip_amount = self._clip_amount.data_ptr()
        a.request = C.pointer(request)
        if cam is not None:
            a.camera = C.pointer(cam)
        if self._cur is not None:
            a.prev = state(self._sets[self._cur])
            a.prev_request = C.pointer(self._request)
            if self._camera is not None:
                a.prev_camera = C.pointer(self._camera)
        with film._torch.cuda.stream(film.stream):
            _history_lib.check("rth_accumulate", self._lib.rth_accumulate(a, film.stream.cuda_stream))
        self._cur, self._request, self._camera, self._samples = nxt, request, cam, film.samples
        self.frames += 1
        out = {n: self._sets[nxt][n] for n in OUTPUTS}
        if self.clip:
            out["clip"] = self._clip_amount
        return out

    # ---- the film's resolves, on the history's sums

    def resolve(self, dreq: Optional[DenoiseRequest] = None, planes: Optional[dict] = None, outputs: Sequence[str] = ("rgb",)) -> dict:
        """Film.resolve on the history's accum."""
        return self.film.resolve(dreq, planes, outputs, _state=self._state())

    def preview(self, outputs: Sequence[str] = ("rgb",)) -> dict:
        """Film.preview on the history's accum."""
        return self.film.resolve(DenoiseRequest.defaults(iterations=0), None, outputs, _state=self._state())

    def resolve_guided(self, planes: Optional[dict] = None, outputs: Sequence[str] = ("rgb",), iterations: int = 5,
                       sigma_l: float = SIGMA_L, var_eps: float = VAR_EPS, k_normal: Optional[float] = None,
                       k_depth: Optional[float] = None) -> dict:
        """Film.resolve_guided on the history's accum and moments.  The variance that steers it is that of one frame's e samples,
        estimated from the blended moments: steadier than a single frame's, not smaller (rt_history.h).  k_normal, k_depth: the
        resolve's, not the history's."""
        return self.film.resolve_guided(planes, outputs, iterations, sigma_l, var_eps, k_normal, k_depth, _state=self._state())

    def variance(self):
        """Film.variance on the history's moments."""
        state = self._state()
        check_guided(True, self.film.samples, (), ("variance",), 0)
        return self.film._guided({}, ("variance",), 0, SIGMA_L, VAR_EPS, 0.0, 0.0, _film_lib.LDS_PLAN, state)["variance"]
