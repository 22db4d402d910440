"""A pyramid bloom of a film's linear image: the glare that shows how bright a light is.

    with rt.Film(scene, strips, moments=True) as film:
        bloom, disp = rt.FilmBloom(film), rt.FilmDisplay(film)
        film.render_pass(0, 32)
        linear = film.resolve_guided(planes, ("linear",))["linear"]
        rgb = disp.display(bloom.apply(linear)["linear"])["rgb"]

A tone curve compresses the pixels of a lamp but cannot give them extent; a bloom can.  The image is sanitised (NaN and negatives to
0, every value under `cap`), optionally thresholded with a soft knee, filtered down through `levels` levels of half the size each
with a 4 x 4 binomial kernel, summed back up with bilinear taps, each coarser level weighted by `spread` more, normalised and mixed
into the image: "mix" is (1 - strength) image + strength bloom and keeps a constant image as it is, "add" is image + strength bloom.
This is the dual-filter pyramid of Jimenez's and Kawase's talks without their firefly weighting: the bloom spreads whatever
fireflies it is given, and rt.FilmRobust upstream is the project's answer to those.

The arithmetic is normative in bloom_csrc/rt_bloom.h and runs in HIP kernels of a private library (lib/librt_bloom.so, _bloom_lib.py)
on the film's stream; nothing returns to the host.  `linear` is any contiguous (R, W, 3) float32 tensor on the film's device: the
"linear" output of Film.preview, resolve, resolve_guided and resolve_regression, of a FilmHistory, of FilmRobust.estimate and, for a
bloom made with shape=, of FilmUpsampler.  The bloom reads it and never writes it, the film or any tensor of theirs, and its output is
the input of FilmDisplay.display.

This module imports without torch; the library is loaded when a FilmBloom is constructed."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence

from . import _bloom_lib

MODES = ("mix", "add")
OUTPUTS = ("linear", "bloom")
MAX_LEVELS = _bloom_lib.MAX_LEVELS
MAX_CAP = 2.0 ** 62
# The form rtb_apply runs in (bloom_csrc/rt_bloom.h): the same bytes under either.  "levels" is a launch a level each way; "tail" gives
# the small levels to one workgroup that keeps them in LDS.  "levels" is the faster at 1920 x 1080 with the default eight levels
# (DESIGN.md 4.33 "Measured", tools/film_bloom_bench.py: 85.7 against 90.5 us, a run-to-run spread of 1.9 %) and at 3840 x 2160;
# "tail" won only at 256 x 144 with eight levels (46.7 against 54.0 us).
FORM = "levels"


class Settings(NamedTuple):
    shape: tuple                  # (R, W)
    levels: int
    spread: float
    strength: float
    mode: str
    threshold: float
    knee: float
    cap: float


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _f32(v) -> Optional[float]:
    """v as the f32 the library will see, or None if it is no real number or does not fit a finite one."""
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return None
    try:
        f = _bloom_lib.f32(v)
    except (OverflowError, ValueError):
        return None
    return f if math.isfinite(f) else None


def _check_shape(shape) -> tuple:
    if not isinstance(shape, (tuple, list)) or len(shape) != 2 or not all(_is_int(v) and v >= 1 for v in shape):
        raise ValueError(f"shape: (rows, columns), positive ints, got {shape!r}")
    if shape[0] * shape[1] > 0x7FFFFFFF:
        raise ValueError(f"shape: {shape[0]} x {shape[1]} is more than 2^31 - 1 pixels")
    return (shape[0], shape[1])


def default_levels(shape) -> int:
    """max(1, min(8, floor(log2(min(R, W))))): the pyramid stops where the shorter side reaches 1 or 2.  Pure."""
    R, W = _check_shape(shape)
    return max(1, min(MAX_LEVELS, min(R, W).bit_length() - 1))


def level_shapes(shape, levels: int) -> tuple:
    """((R_0, W_0), ..., (R_levels, W_levels)): each side is (side + 1) >> 1 of the level above, and a side of 1 stays 1.  Pure."""
    R, W = _check_shape(shape)
    if not _is_int(levels) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels: an int in 1 ... {MAX_LEVELS}, got {levels!r}")
    out = [(R, W)]
    for _ in range(levels):
        R, W = (R + 1) >> 1, (W + 1) >> 1
        out.append((R, W))
    return tuple(out)


def scratch_layout(shape, levels: int) -> tuple:
    """(the byte offsets of levels 1 ... levels in the scratch, its size): each level is its pixels times 12 bytes, rounded up to 16."""
    at, offsets = 0, []
    for R, W in level_shapes(shape, levels)[1:]:
        offsets.append(at)
        at += (R * W * 12 + 15) & ~15
    return tuple(offsets), at


def check_bloom(shape, levels=None, spread: float = 0.7, strength: float = 0.05, mode: str = "mix", threshold: float = 0.0,
                knee: float = 0.5, cap: float = 65536.0) -> Settings:
    """The checks of FilmBloom's arguments, all of them ValueError and none of them a GPU call.  shape: (R, W), positive ints with
    R W <= 2^31 - 1.  levels: None (default_levels) or an int in 1 ... 8.  spread: in (0, 1] as f32.  mode: one of MODES.  strength:
    in (0, 1) as f32 under "mix", finite and positive under "add".  threshold: finite, >= 0 and <= cap; 0 is no threshold.  knee: in
    [0, 1].  cap: in (0, 2^62].  Returns the Settings the calls are made with.  Pure: no torch, no GPU."""
    shape = _check_shape(shape)
    if levels is None:
        levels = default_levels(shape)
    level_shapes(shape, levels)
    s = _f32(spread)
    if s is None or not 0.0 < s <= 1.0:
        raise ValueError(f"spread: in (0, 1], got {spread!r}")
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"mode: one of {MODES}, got {mode!r}")
    g = _f32(strength)
    if g is None or not g > 0.0 or (mode == "mix" and not g < 1.0):
        raise ValueError(f"strength: in (0, 1) under 'mix', finite and positive under 'add', got {strength!r}")
    c = _f32(cap)
    if c is None or not 0.0 < c <= MAX_CAP:
        raise ValueError(f"cap: in (0, 2^62], got {cap!r}")
    t = _f32(threshold)
    if t is None or not 0.0 <= t <= c:
        raise ValueError(f"threshold: finite, at least 0 and at most the cap, got {threshold!r}")
    k = _f32(knee)
    if k is None or not 0.0 <= k <= 1.0:
        raise ValueError(f"knee: in [0, 1], got {knee!r}")
    return Settings(shape, levels, float(spread), float(strength), mode, float(threshold), float(knee), float(cap))


def check_outputs(outputs: Sequence[str] = ("linear",)) -> tuple:
    """The outputs of apply: a subset of OUTPUTS that holds "linear", ValueError otherwise.  Pure."""
    outs = tuple(outputs)
    if "linear" not in outs or any(o not in OUTPUTS for o in outs) or len(set(outs)) != len(outs):
        raise ValueError(f"outputs: 'linear', and 'bloom' where wanted, got {outs}")
    return outs


class FilmBloom:
    """The bloom of one film's frames (or, with shape=, of frames of another size on the film's device and stream).

    The defaults are aesthetic settings, not tuned results: a spread of 0.7 puts a third of the bloom into the finest level and keeps
    the widest visible, a strength of 0.05 under "mix" leaves ordinary surfaces as they were to within a code or two and lets a lamp a
    hundred times brighter than white glow, no threshold keeps the stage energy-conserving, and the cap of 65 536 only keeps one
    infinite pixel from flooding the frame.  levels=None takes max(1, min(8, floor(log2(min(R, W))))).

    State on the device: the scratch that holds the pyramid, and nothing else.  apply() enqueues on film.stream, waits for nothing
    and returns new tensors at every call.  Not thread-safe."""

    def __init__(self, film, levels=None, spread: float = 0.7, strength: float = 0.05, mode: str = "mix", threshold: float = 0.0,
                 knee: float = 0.5, cap: float = 65536.0, shape=None):
        if shape is None:
            shape = (getattr(film, "rows", None), getattr(film, "width", None))
        self.settings = check_bloom(shape, levels, spread, strength, mode, threshold, knee, cap)
        film._check_open()
        self._lib = _bloom_lib.load()
        self.film = film
        self.form = FORM
        s = self.settings
        self.norm = _bloom_lib.norm_of(s.spread, s.levels)
        self.K = _bloom_lib.knee_of(s.threshold, s.knee)
        torch = film._torch
        self.scratch_bytes = scratch_layout(s.shape, s.levels)[1]
        with torch.cuda.stream(film.stream):
            self._scratch = torch.empty((self.scratch_bytes,), dtype=torch.uint8, device=film.device)

    def _check_open(self):
        if getattr(self, "_scratch", None) is None:
            raise ValueError("the bloom is closed")
        self.film._check_open()

    def close(self):
        """Wait for the film's stream and drop the scratch.  The film stays the caller's."""
        if getattr(self, "_scratch", None) is None:
            return
        if self.film.accum is not None:
            self.film.sync()
        self._scratch = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check_linear(self, linear):
        torch = self.film._torch
        R, W = self.settings.shape
        if not isinstance(linear, torch.Tensor):
            raise ValueError(f"linear: a tensor, got {type(linear).__name__}")
        if tuple(linear.shape) != (R, W, 3) or linear.dtype != torch.float32:
            raise ValueError(f"linear: a ({R}, {W}, 3) float32 tensor, got {tuple(linear.shape)} {linear.dtype}")
        if linear.device != self.film.device:
            raise ValueError(f"linear: on {linear.device}, the film is on {self.film.device}")
        if not linear.is_contiguous() or linear.data_ptr() % 16:
            raise ValueError("linear: a contiguous tensor at a 16-byte boundary")

    def apply(self, linear, outputs: Sequence[str] = ("linear",)) -> dict:
        """The frame with its bloom: {output: a new (R, W, 3) float32 tensor} out of "linear", the mixed image, and "bloom", the
        normalised bloom alone.  One rtb_apply on the film's stream; the input is not written."""
        outs = check_outputs(outputs)
        self._check_open()
        self._check_linear(linear)
        torch = self.film._torch
        s = self.settings
        R, W = s.shape
        with torch.cuda.stream(self.film.stream):
            out = {o: torch.empty((R, W, 3), dtype=torch.float32, device=self.film.device) for o in outs}
        a = _bloom_lib.ApplyArgs(W=W, R=R, levels=s.levels, mode=_bloom_lib.MODES[s.mode], form=_bloom_lib.FORMS[self.form],
                                 spread=s.spread, strength=s.strength, norm=self.norm, cap=s.cap, T=s.threshold, K=self.K,
                                 inp=linear.data_ptr(), out=out["linear"].data_ptr(),
                                 out_bloom=out["bloom"].data_ptr() if "bloom" in out else None,
                                 scratch=self._scratch.data_ptr(), scratch_bytes=self.scratch_bytes)
        _bloom_lib.check("rtb_apply", self._lib.rtb_apply(a, self.film.stream.cuda_stream))
        return out
