"""Adaptive sampling for rt.Film: after a floor of uniform passes, further samples go only to the pixels whose sample moments say they
are still noisy.

    with rt.Film(scene, strips, integrator="nee", moments=True) as film, rt.FilmSampler(film, threshold=0.05) as sampler:
        film.render_pass(0, 4)                              # the floor: every pixel, uniformly
        sampler.begin()
        sampler.render(4)                                   # rounds of up to 4 sample indices, until no pixel is active
        rgb = sampler.resolve_guided(planes)["rgb"]
        counts = sampler.counts                             # (R, W) int32: the samples each pixel got

A round decides from the sums as they stand: a pixel is noisy if the standard error of its mean luminance, relative to |mean| + eps,
exceeds `threshold`, and active if a pixel within `dilate` of it is noisy.  The active pixels of a strip are listed in ascending
order, their camera rays and RNG states are gathered out of the strip's ray buffer, the film's integrator traces the compact batch,
and the colours are folded back by pixel.  Sample (pixel, s) has a stream of its own, so a pixel that sat out a round simply never
draws that round's indices.  The arithmetic is normative in sampler_csrc/rt_sampler.h and runs in HIP kernels of a private library
(lib/librt_sampler.so, _sampler_lib.py).

The sampler keeps sums of its own: it never writes the film's accum, moments or samples, so the uniform passes stay the floor and the
film stays what it was.  Its resolves are the film's, run on the sums restated "at the film's count" (rts_normalise).

Composing with rt.FilmHistory is out of scope: a history blends sums that every pixel holds at one count, which the sampler's are not.
The sampler's rounds do not feed the film's taps (rt.FilmRobust): a tap sees the film's own passes only, and composing the two is out
of scope.

This module imports without torch; the library is loaded when a FilmSampler is constructed."""
from __future__ import annotations

import math
from typing import Optional, Sequence

from . import _film_lib, _sampler_lib
from ._abi import DenoiseRequest
from .film import SIGMA_L, VAR_EPS, check_guided, sample_chunks

# The defaults (DESIGN.md 4.25 "Measured"): the best of the grid of tools/film_sampler_bench.py, threshold in {0.05, 0.1, 0.2, 0.4, 0.8},
# by the mean squared error at equal time against the uniform film on c2 and c3 at 1920 x 1080, through preview and resolve_guided.
# At 0.05 the sampler equals the uniform film at equal time (ratios 1.00 to 1.01); at every more selective threshold of the grid it
# loses at equal time on both scenes, though on c3 it wins at equal traced samples (0.77 to 0.83 x at 0.1 and 0.2).  eps, in units of
# y, keeps a black pixel from being selected on rounding noise; 2^-6 and 2^-10 measured the same.
THRESHOLD = 0.05
EPS = 2.0 ** -6
DILATE = 1


def check_sampler(moments: bool, threshold: float = THRESHOLD, dilate: int = DILATE, eps: float = EPS) -> tuple:
    """The checks of FilmSampler's arguments, all of them ValueError and none of them a GPU call.  moments: whether the film was made
    with moments=True.  threshold: a number >= 0 that is not a NaN; finite, or +inf for a sampler that never finds a noisy pixel.
    dilate: 0 or 1.  eps: finite and > 0.  Returns (threshold, dilate, eps).  Pure: no torch, no GPU."""
    if not moments:
        raise ValueError("a sampler needs a film made with moments=True")
    for name, v in (("threshold", threshold), ("eps", eps)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
            raise ValueError(f"{name}: a number, got {v!r}")
    if not threshold >= 0:
        raise ValueError(f"threshold: need threshold >= 0, got {threshold!r}")
    if not math.isfinite(eps) or not eps > 0:
        raise ValueError(f"eps: need a finite eps > 0, got {eps!r}")
    if isinstance(dilate, bool) or not isinstance(dilate, int) or dilate not in (0, 1):
        raise ValueError(f"dilate: 0 or 1, got {dilate!r}")
    return float(threshold), dilate, float(eps)


class FilmSampler:
    """The adaptive sampler of one film made with moments=True.

    begin() takes the film as it stands (at least 2 samples) as the floor: the film's accum and moments are copied into the
    sampler's own tensors and every pixel's count is film.samples.  render_pass(n) is one round over the sample indices
    [samples, min(samples + n, film.spp)); render(n) repeats it until a round finds no active pixel or the indices run out.

    Normative: after any rounds, accum[p] is the f32 sum, in order, of the integrator's colours of (p, s) over the film's [0, e0) and
    then over the indices of every round in which p was active, moments[p] the sums of their y and y y in the same order, and
    counts[p] the number of those samples.

    Everything is enqueued on film.stream.  A round waits for the stream once, to read the strips' active counts.  The tensors
    returned are the sampler's own (the resolves' outputs the film's) and are written again by the next call of the same kind.  The
    film must hold the floor's sample count for as long as the sampler is used; begin() again takes a new floor.  Not thread-safe."""

    def __init__(self, film, threshold: float = THRESHOLD, dilate: int = DILATE, eps: float = EPS):
        self.threshold, self.dilate, self.eps = check_sampler(getattr(film, "moments", None) is not None, threshold, dilate, eps)
        film._check_open()
        self._lib = _sampler_lib.load()
        self.film = film
        torch = film._torch
        R, W, hs = film.rows, film.width, film.hs
        self._strips = R // hs
        n = hs * W * film.k
        with torch.cuda.stream(film.stream):
            dev = film.device
            self.accum = torch.zeros((R, W, 3), dtype=torch.float32, device=dev)
            self.moments = torch.zeros((R, W, 2), dtype=torch.float32, device=dev)
            self.counts = torch.zeros((R, W), dtype=torch.int32, device=dev)
            self.error = torch.zeros((R, W), dtype=torch.float32, device=dev)
            self.active = torch.zeros((R * W,), dtype=torch.int32, device=dev)              # uint32 strip indices, strip i from i hs W
            self.strip_counts = torch.zeros((self._strips,), dtype=torch.int32, device=dev)
            self._scratch = torch.empty(_sampler_lib.scratch_bytes(W, R, hs), dtype=torch.uint8, device=dev)
            self._rays = torch.empty((n, 8), dtype=torch.float32, device=dev)               # the compact batch, sized like the film's
            self._states = torch.empty((n, 4), dtype=torch.int64, device=dev)
            self._norm = (torch.zeros((R, W, 3), dtype=torch.float32, device=dev), torch.zeros((R, W, 2), dtype=torch.float32, device=dev))
        self._host_counts = torch.zeros((self._strips,), dtype=torch.int32).pin_memory()
        self._e0 = 0
        self.samples = 0
        self.rounds = 0
        self.last_active = None                   # the strips' active counts of the last select, a list

    # ---- state

    def _check_open(self):
        if getattr(self, "accum", None) is None:
            raise ValueError("the sampler is closed")
        self.film._check_open()

    def _check_begun(self):
        self._check_open()
        if not self._e0:
            raise ValueError("the sampler holds no floor yet: call begin() first")
        if self.film.samples != self._e0:
            raise ValueError(f"the film holds {self.film.samples} samples, the sampler's floor {self._e0}: call begin() again")

    def begin(self):
        """Take the film as it stands as the floor.  Needs film.samples >= 2 (a variance needs two samples)."""
        self._check_open()
        film = self.film
        if film.samples < 2:
            raise ValueError(f"begin: the film holds {film.samples} samples, the floor is at least 2")
        with film._torch.cuda.stream(film.stream):
            self.accum.copy_(film.accum)
            self.moments.copy_(film.moments)
            self.counts.fill_(film.samples)
            self.error.zero_()
        self._e0 = self.samples = film.samples
        self.rounds = 0
        self.last_active = None

    def reset(self):
        """Forget the floor and the rounds: the next call is begin().  Nothing is enqueued."""
        self._check_open()
        self._e0 = self.samples = self.rounds = 0
        self.last_active = None

    def close(self):
        """Wait for the film's stream and drop the tensors.  The film stays the caller's."""
        if getattr(self, "accum", None) is None:
            return
        if self.film.accum is not None:
            self.film.sync()
        self.accum = self.moments = self.counts = self.error = self.active = self.strip_counts = None
        self._scratch = self._rays = self._states = self._norm = self._host_counts = None
        self._e0 = self.samples = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def active_fraction(self) -> float:
        """The share of the image's pixels the last select found active (0.0 before any)."""
        if not self.last_active:
            return 0.0
        return sum(self.last_active) / float(self.film.rows * self.film.width)

    # ---- a round

    def _select(self) -> list:
        """rts_select on the sums as they stand, then the round's only host wait: the strips' counts."""
        film = self.film
        a = _sampler_lib.SelectArgs(W=film.width, R=film.rows, Hs=film.hs, dilate=self.dilate, threshold=self.threshold, eps=self.eps,
                                    moments=self.moments.data_ptr(), counts=self.counts.data_ptr(), err=self.error.data_ptr(),
                                    active=self.active.data_ptr(), strip_counts=self.strip_counts.data_ptr(),
                                    scratch=self._scratch.data_ptr(), scratch_bytes=self._scratch.numel())
        _sampler_lib.check("rts_select", self._lib.rts_select(a, film.stream.cuda_stream))
        self._host_counts.copy_(self.strip_counts, non_blocking=True)
        film.stream.synchronize()
        self.last_active = [int(c) for c in self._host_counts.tolist()]
        return self.last_active

    def render_pass(self, n: int) -> int:
        """One round over the sample indices [samples, min(samples + n, film.spp)).  Returns the number of active pixels; 0 means
        nothing was traced and the indices are not consumed (no pixel is active, or the indices have run out)."""
        self._check_begun()
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"render_pass: n is an int >= 1, got {n!r}")
        film = self.film
        begin, end = self.samples, min(self.samples + n, film.spp)
        if begin >= end:
            return 0
        pixels = film.hs * film.width
        handle = film.stream.cuda_stream
        with film._torch.cuda.stream(film.stream):
            counts = self._select()
            total = sum(counts)
            if total == 0:
                return 0
            chunks = sample_chunks(pixels, begin, end, film.max_records)
            for i, rq in enumerate(film.reqs):
                na = counts[i]
                if na == 0:
                    continue
                active = self.active[i * pixels:].data_ptr()
                acc, mom, cnt = (film._strip(t, i).data_ptr() for t in (self.accum, self.moments, self.counts))
                for b, e in chunks:
                    k = e - b
                    film._reserve(2)
                    film.scene.camera_rays_device(rq, b, e, film._rays.data_ptr(), film._states.data_ptr(), stream=handle)
                    g = _sampler_lib.GatherArgs(n_active=na, k=k, pixels=pixels, active=active, rays=film._rays.data_ptr(),
                                                states=film._states.data_ptr(), out_rays=self._rays.data_ptr(),
                                                out_states=self._states.data_ptr())
                    _sampler_lib.check("rts_gather", self._lib.rts_gather(g, handle))
                    film._trace(na * k, rq.max_bounces, handle, self._rays, self._states)
                    f = _sampler_lib.FoldArgs(n_active=na, k=k, pixels=pixels, active=active, rgb=film._rgb.data_ptr(), accum=acc,
                                              moments=mom, counts=cnt)
                    _sampler_lib.check("rts_fold", self._lib.rts_fold(f, handle))
        self.samples = end
        self.rounds += 1
        return total

    def render(self, n: int) -> int:
        """Rounds of up to n sample indices until one finds no active pixel or the indices reach film.spp.  Returns the rounds run."""
        rounds = 0
        while self.render_pass(n):
            rounds += 1
        return rounds

    # ---- the film's resolves, on the normalised sums

    def normalised(self) -> tuple:
        """(accum, moments) restated at the film's count (rts_normalise): what the film's resolves read.  The sampler's own tensors,
        written again by the next resolve."""
        self._check_begun()
        film = self.film
        a = _sampler_lib.NormaliseArgs(W=film.width, R=film.rows, e0=self._e0, accum=self.accum.data_ptr(),
                                       moments=self.moments.data_ptr(), counts=self.counts.data_ptr(),
                                       out_accum=self._norm[0].data_ptr(), out_moments=self._norm[1].data_ptr())
        with film._torch.cuda.stream(film.stream):
            _sampler_lib.check("rts_normalise", self._lib.rts_normalise(a, film.stream.cuda_stream))
        return self._norm

    def resolve(self, dreq: Optional[DenoiseRequest] = None, planes: Optional[dict] = None, outputs: Sequence[str] = ("rgb",)) -> dict:
        """Film.resolve on the normalised accum."""
        return self.film.resolve(dreq, planes, outputs, _state=self.normalised())

    def preview(self, outputs: Sequence[str] = ("rgb",)) -> dict:
        """Film.preview on the normalised accum."""
        return self.film.resolve(DenoiseRequest.defaults(iterations=0), None, outputs, _state=self.normalised())

    def resolve_guided(self, planes: Optional[dict] = None, outputs: Sequence[str] = ("rgb",), iterations: int = 5,
                       sigma_l: float = SIGMA_L, var_eps: float = VAR_EPS, k_normal: Optional[float] = None,
                       k_depth: Optional[float] = None) -> dict:
        """Film.resolve_guided on the normalised sums: the variance that steers it is each pixel's variance of the mean at the
        pixel's own count (rt_sampler.h)."""
        return self.film.resolve_guided(planes, outputs, iterations, sigma_l, var_eps, k_normal, k_depth, _state=self.normalised())

    def variance(self):
        """Film.variance on the normalised moments: every pixel's variance of the mean at its own count."""
        state = self.normalised()
        check_guided(True, self.film.samples, (), ("variance",), 0)
        return self.film._guided({}, ("variance",), 0, SIGMA_L, VAR_EPS, 0.0, 0.0, _film_lib.LDS_PLAN, state)["variance"]
