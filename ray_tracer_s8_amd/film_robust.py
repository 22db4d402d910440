"""A firefly-robust estimate of an rt.Film by median of means.

    with rt.Film(scene, strips, integrator="path", moments=True) as film, rt.FilmRobust(film) as robust:
        film.render_pass(0, 32)                             # the film's own passes: the robust film sees every strip's records
        rgb = robust.preview()["rgb"]                       # the film's preview of the robust estimate
        out = robust.estimate(("linear", "gini", "kept"))   # the estimate itself, and what it kept of every pixel
        rgb = robust.resolve_guided(planes)["rgb"]          # the film's resolves, steered by the robust variance

One sample that finds a small lamp by chance, or lands next to a light under area sampling, is a white dot in the plain mean, an
inflated variance for the guided resolve and a pixel that stays "noisy" for good.  Here sample s of a pixel is added to bucket
s mod K of K colour sums, and the pixel is estimated from the central bucket means in the order of their luminance: the median bucket
alone where the bucket means are spread widely, every bucket (the plain mean of means) where they agree, the width chosen per pixel
from their Gini coefficient (GMoN, Buisine et al. 2021) or fixed by the caller.  The arithmetic is normative in
robust_csrc/rt_robust.h and runs in HIP kernels of a private library (lib/librt_robust.so, _robust_lib.py).

The robust film is a tap of the film (Film._taps): it is shown the records of every strip's sub-range right after the film folded
them, on the film's stream, and folds them into its buckets in order.  It never writes the film's accum, moments or samples, and the
bytes of its buckets do not depend on how the job was cut into passes.  The median of means is biased low on skewed pixels: it trades
energy for the absence of fireflies (DESIGN.md 4.29 "Measured").

Composing with rt.FilmHistory and rt.FilmUpsampler works through the `linear` output only; rt.FilmSampler's rounds do not feed taps.

This module imports without torch; the library is loaded when a FilmRobust is constructed."""
from __future__ import annotations

from typing import Optional, Sequence

from . import _film_lib, _robust_lib
from ._abi import DenoiseRequest
from .film import SIGMA_L, VAR_EPS, check_guided

# The defaults (DESIGN.md 4.29 "Measured", tools/film_robust_bench.py: c2 and c3 at 1920 x 1080, 16 to 64 samples, K in {5, 9, 15}).
# "gini" has the smaller error than the median bucket alone at every point measured.  K = 5, not the 9 this began with: at these counts
# fewer, fuller buckets lose less energy and have the smaller error on c2 under every integrator (at 32 samples of light-only NEE the
# image keeps 87 % of its energy with K = 5, 82 % with 9, 75 % with 15) and on c3 K = 9 is ahead by no more than 6 % in the preview.
BUCKETS = 5
MODES = ("gini", "trim")
OUTPUTS = ("linear", "gini", "kept", "variance")
MIN_BUCKETS, MAX_BUCKETS = _robust_lib.MIN_BUCKETS, _robust_lib.MAX_BUCKETS


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def check_robust(samples: int, buckets: int = BUCKETS, mode: str = "gini", c: Optional[int] = None) -> tuple:
    """The checks of FilmRobust's arguments, all of them ValueError and none of them a GPU call.  samples: what the film holds at
    construction, which must be 0 (the buckets start with the job).  buckets: odd, 3 ... 15.  mode: "gini" or "trim".  c: under "trim"
    the half-width of the kept centre, 0 (the median bucket) ... (buckets - 1) / 2 (every bucket); under "gini" it is refused.
    Returns (buckets, mode, c), c as 0 under "gini".  Pure: no torch, no GPU."""
    if not _is_int(buckets) or not MIN_BUCKETS <= buckets <= MAX_BUCKETS or buckets % 2 == 0:
        raise ValueError(f"buckets: an odd int in {MIN_BUCKETS} ... {MAX_BUCKETS}, got {buckets!r}")
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"mode: one of {MODES}, got {mode!r}")
    h = (buckets - 1) // 2
    if mode == "trim":
        if not _is_int(c) or not 0 <= c <= h:
            raise ValueError(f'c: under mode="trim" an int in 0 ... {h}, got {c!r}')
    elif c is not None:
        raise ValueError('c: under mode="gini" the width is the pixel\'s own, leave c out')
    if not _is_int(samples) or samples != 0:
        raise ValueError(f"the film holds {samples!r} samples: a robust film starts with the job, at 0 samples (film.reset() first)")
    return buckets, mode, (c if mode == "trim" else 0)


def check_estimate(film_samples: int, samples: int, buckets: int, outputs: Sequence[str] = ("linear",)) -> tuple:
    """The checks of every estimate, ValueError: the buckets hold what the film holds, every bucket holds a sample, and the outputs
    are a non-empty subset of OUTPUTS.  Returns the outputs as a tuple.  Pure: no torch, no GPU."""
    outs = tuple(outputs)
    if not outs or any(o not in OUTPUTS for o in outs) or len(set(outs)) != len(outs):
        raise ValueError(f"outputs: a non-empty subset of {OUTPUTS}, got {outs}")
    if film_samples != samples:
        raise ValueError(f"the film holds {film_samples} samples, the buckets {samples}: the film was advanced while the robust film "
                         "was not its tap; film.reset() and render again")
    if samples < buckets:
        raise ValueError(f"the buckets hold {samples} samples: an estimate needs one in each of the {buckets} buckets")
    return outs


class FilmRobust:
    """The robust estimate of one film, made while the film holds no samples.

    Memory: the buckets are one (K, R, W, 3) float32 tensor, K R W 12 bytes: 224 MB at 1920 x 1080 with K = 9, 124 MB with the default
    K = 5.  buckets[k] is a film-shaped colour sum.

    Normative: after film passes covering [0, e), buckets[k][p] is the f32 sum from +0, in ascending s, of the integrator's colours of
    the samples (p, s) with s mod K == k, bit for bit however the samples were cut into passes or sub-ranges.

    Everything is enqueued on film.stream.  The tensors returned are the robust film's own (the resolves' outputs the film's) and are
    written again by the next call of the same kind.  Every estimate refuses, with a ValueError, a film whose sample count is not the
    buckets' (it was advanced while close() or a removal had taken the tap away) and a count below K.  film.reset() zeroes the
    buckets with the film.  Not thread-safe."""

    def __init__(self, film, buckets: int = BUCKETS, mode: str = "gini", c: Optional[int] = None):
        self.K, self.mode, self.c = check_robust(getattr(film, "samples", None), buckets, mode, c)
        film._check_open()
        self._lib = _robust_lib.load()
        self.film = film
        torch = film._torch
        R, W = film.rows, film.width
        with torch.cuda.stream(film.stream):
            dev = film.device
            self.buckets = torch.zeros((self.K, R, W, 3), dtype=torch.float32, device=dev)
            self._state = (torch.zeros((R, W, 3), dtype=torch.float32, device=dev), torch.zeros((R, W, 2), dtype=torch.float32, device=dev))
        self._out: dict = {}
        self.samples = 0
        film._taps.append(self)

    # ---- state

    def _check_open(self):
        if getattr(self, "buckets", None) is None:
            raise ValueError("the robust film is closed")
        self.film._check_open()

    def close(self):
        """Leave the film's taps, wait for the film's stream and drop the tensors.  The film stays the caller's."""
        if getattr(self, "buckets", None) is None:
            return
        if self in self.film._taps:
            self.film._taps.remove(self)
        if self.film.accum is not None:
            self.film.sync()
        self.buckets = self._state = None
        self._out = {}
        self.samples = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- the tap (Film.render_pass, Film.reset)

    def _on_records(self, i: int, b: int, e: int, records) -> None:
        """Samples [b, e) of strip i, records (pixels, e - b, 3): one rtr_fold on the film's stream."""
        film = self.film
        pixels = film.hs * film.width
        a = _robust_lib.FoldArgs(pixels=pixels, n=e - b, first=b, K=self.K, bucket_stride=film.rows * film.width * 3,
                                 records=records.data_ptr(), buckets=film._strip(self.buckets[0], i).data_ptr())
        _robust_lib.check("rtr_fold", self._lib.rtr_fold(a, film.stream.cuda_stream))
        if i == len(film.reqs) - 1:
            self.samples = e

    def _on_reset(self) -> None:
        with self.film._torch.cuda.stream(self.film.stream):
            self.buckets.zero_()
        self.samples = 0

    # ---- the estimate

    def _resolve(self, outs: tuple, state: bool) -> dict:
        """One rtr_resolve on the film's stream into the robust film's own tensors."""
        film = self.film
        torch = film._torch
        R, W = film.rows, film.width
        with torch.cuda.stream(film.stream):
            for o in outs:
                if o not in self._out:
                    shape = (R, W, 3) if o == "linear" else (R, W)
                    self._out[o] = torch.empty(shape, dtype=torch.int32 if o == "kept" else torch.float32, device=film.device)
            ptr = lambda o: self._out[o].data_ptr() if o in outs else None
            a = _robust_lib.ResolveArgs(W=W, R=R, K=self.K, samples=self.samples, mode=_robust_lib.MODES[self.mode], c=self.c,
                                        buckets=self.buckets.data_ptr(), out_linear=ptr("linear"), out_gini=ptr("gini"),
                                        out_kept=ptr("kept"), out_variance=ptr("variance"),
                                        out_accum=self._state[0].data_ptr() if state else None,
                                        out_moments=self._state[1].data_ptr() if state else None)
            _robust_lib.check("rtr_resolve", self._lib.rtr_resolve(a, film.stream.cuda_stream))
        return {o: self._out[o] for o in outs}

    def estimate(self, outputs: Sequence[str] = ("linear",)) -> dict:
        """The estimate at the film's count: {output: tensor} out of linear (R, W, 3) float32, the robust mean colour; gini (R, W)
        float32, the Gini coefficient of the pixel's bucket means; kept (R, W) int32, the buckets the estimate kept, 1 ... K; variance
        (R, W) float32, the winsorised variance of the estimate's luminance."""
        self._check_open()
        outs = check_estimate(self.film.samples, self.samples, self.K, outputs)
        return self._resolve(outs, False)

    def state(self) -> tuple:
        """(accum, moments) of the robust estimate restated at the film's count (rt_robust.h "Restated sums"): what the film's
        resolves read through _state.  The robust film's own tensors, written again by the next state()."""
        self._check_open()
        check_estimate(self.film.samples, self.samples, self.K)
        self._resolve((), True)
        return self._state

    # ---- the film's resolves, on the restated sums

    def resolve(self, dreq: Optional[DenoiseRequest] = None, planes: Optional[dict] = None, outputs: Sequence[str] = ("rgb",)) -> dict:
        """Film.resolve on the robust accum."""
        return self.film.resolve(dreq, planes, outputs, _state=self.state())

    def preview(self, outputs: Sequence[str] = ("rgb",)) -> dict:
        """Film.preview on the robust accum."""
        return self.film.resolve(DenoiseRequest.defaults(iterations=0), None, outputs, _state=self.state())

    def resolve_guided(self, planes: Optional[dict] = None, outputs: Sequence[str] = ("rgb",), iterations: int = 5,
                       sigma_l: float = SIGMA_L, var_eps: float = VAR_EPS, k_normal: Optional[float] = None,
                       k_depth: Optional[float] = None) -> dict:
        """Film.resolve_guided on the restated sums: the variance that steers it is the robust estimate's.  Needs a film made with
        moments=True."""
        check_guided(self.film.moments is not None, self.film.samples)
        return self.film.resolve_guided(planes, outputs, iterations, sigma_l, var_eps, k_normal, k_depth, _state=self.state())

    def variance(self):
        """Film.variance on the restated moments.  Needs a film made with moments=True."""
        check_guided(self.film.moments is not None, self.film.samples, (), ("variance",), 0)
        state = self.state()
        return self.film._guided({}, ("variance",), 0, SIGMA_L, VAR_EPS, 0.0, 0.0, _film_lib.LDS_PLAN, state)["variance"]
