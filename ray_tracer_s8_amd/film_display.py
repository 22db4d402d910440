"""The display transform of a film's linear image: metered exposure, a tone curve, quantisation.

    with rt.Film(scene, strips, moments=True) as film:
        disp = rt.FilmDisplay(film, rate=0.25)
        film.render_pass(0, 32)
        rgb = disp.display(film.resolve_guided(planes, ("linear",))["linear"])["rgb"]

The film's own "rgb" is sqrt(linear) * 255.999, saturated: the reference's convention.  A linear HDR image wants more of its last
stage: the frame is metered into a luminance histogram (eight bins an octave, binned from the float's bit pattern), a percentile of
the histogram is scaled to a key value, the exposure follows the frames at a rate, the highlights are compressed by a tone curve
(Reinhard's with a white point, or Narkowicz's fit of the ACES filmic curve) and the result is quantised, with an ordered dither where
asked.  The arithmetic is normative in display_csrc/rt_display.h and runs in HIP kernels of a private library
(lib/librt_display.so, _display_lib.py); the exposure record lives in device memory and nothing returns to the host, so a frame's
display is three launches and a 1 KB clear on the film's stream.

`linear` is any contiguous (R, W, 3) float32 tensor on the film's device: the "linear" output of Film.preview, resolve and
resolve_guided, of a FilmHistory, of FilmUpsampler (a display made with shape=) and of FilmRobust.estimate.  The display reads it and
never writes it, the film or any tensor of theirs.

This module imports without torch; the library is loaded when a FilmDisplay is constructed."""
from __future__ import annotations

import math
import struct
from typing import NamedTuple, Optional, Sequence

from . import _display_lib

CURVES = ("none", "reinhard", "filmic")
OUTPUTS = ("rgb", "f32")
# The defaults (DESIGN.md 4.30 "Measured", tools/film_display_bench.py).  key 0.54 is the middle of the bin of 0.5 ... 0.545, so a
# frame whose median luminance sits there gets scale 1; luminance is the channels' sum, so 0.54 is a mid grey of 0.18 a channel.
KEY, KEY_PERCENTILE, WHITE_PERCENTILE = 0.54, 0.5, 0.99
SCALE_RANGE = (2.0 ** -8, 2.0 ** 8)
# The histogram form rtd_meter counts with (display_csrc/rt_display.hip.h): the counts are the same bytes under either.  "wave" is
# the faster on a rendered frame and on noise and never far off (DESIGN.md 4.30 "Measured": 11, 15 and 12 us a 1920 x 1080 frame on a
# preview, a constant image and noise, against 16 ... 31, 10 and 46 us for "match").
HISTOGRAM_FORM = "wave"


class Settings(NamedTuple):
    shape: tuple                  # (R, W)
    curve: str
    key: float
    key_q16: int
    white_q16: int
    rate: float
    scale_min: float
    scale_max: float
    dither: bool


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _f32(v) -> Optional[float]:
    """v as the f32 the library will see, or None if it is no real number or does not fit one."""
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return None
    try:
        f = struct.unpack("f", struct.pack("f", v))[0]
    except (OverflowError, struct.error):
        return None
    return None if math.isinf(f) and not math.isinf(v) else f


def _finite_positive(v) -> bool:
    f = _f32(v)
    return f is not None and 0.0 < f < math.inf


def percentile_q16(p) -> int:
    """A percentile in [0, 1] as the library's q16: min(65535, floor(p * 65536)).  ValueError for anything else.  Pure."""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
        raise ValueError(f"a percentile is a number in [0, 1], got {p!r}")
    return min(65535, int(math.floor(p * 65536.0)))


def check_display(shape, curve: str = "filmic", key: float = KEY, key_percentile: float = KEY_PERCENTILE,
                  white_percentile: float = WHITE_PERCENTILE, rate: float = 1.0, scale_range=SCALE_RANGE, dither: bool = False) -> Settings:
    """The checks of FilmDisplay's arguments, all of them ValueError and none of them a GPU call.  shape: (R, W), positive ints with
    R W <= 2^31 - 1.  curve: one of CURVES.  key, rate and both ends of scale_range: finite and positive as f32, rate <= 1,
    scale_range ascending.  The percentiles: in [0, 1], the white one not below the key one.  dither: a bool.  Returns the Settings
    the calls are made with.  Pure: no torch, no GPU."""
    if not isinstance(shape, (tuple, list)) or len(shape) != 2 or not all(_is_int(v) and v >= 1 for v in shape):
        raise ValueError(f"shape: (rows, columns), positive ints, got {shape!r}")
    if shape[0] * shape[1] > 0x7FFFFFFF:
        raise ValueError(f"shape: {shape[0]} x {shape[1]} is more than 2^31 - 1 pixels")
    if not isinstance(curve, str) or curve not in CURVES:
        raise ValueError(f"curve: one of {CURVES}, got {curve!r}")
    if not _finite_positive(key):
        raise ValueError(f"key: finite and positive, got {key!r}")
    if not _finite_positive(rate) or _f32(rate) > 1.0:
        raise ValueError(f"rate: in (0, 1], got {rate!r}")
    if not isinstance(scale_range, (tuple, list)) or len(scale_range) != 2 or not all(_finite_positive(v) for v in scale_range):
        raise ValueError(f"scale_range: (least, greatest), finite and positive, got {scale_range!r}")
    if _f32(scale_range[0]) > _f32(scale_range[1]):
        raise ValueError(f"scale_range: the least scale is above the greatest in {scale_range!r}")
    key_q16, white_q16 = percentile_q16(key_percentile), percentile_q16(white_percentile)
    if white_q16 < key_q16:
        raise ValueError(f"white_percentile {white_percentile!r} is below key_percentile {key_percentile!r}")
    if not isinstance(dither, bool):
        raise ValueError(f"dither: a bool, got {dither!r}")
    return Settings((shape[0], shape[1]), curve, float(key), key_q16, white_q16, float(rate), float(scale_range[0]),
                    float(scale_range[1]), dither)


def check_exposure(scale, white=math.inf) -> tuple:
    """The checks of set_exposure, ValueError: scale > 0 and white >= 1 as f32, each finite or +inf.  Returns (scale, white).  Pure."""
    s, w = (math.inf if v == math.inf else _f32(v) for v in (scale, white))
    if s is None or not s > 0.0:
        raise ValueError(f"scale: positive, finite or +inf, got {scale!r}")
    if w is None or not w >= 1.0:
        raise ValueError(f"white: at least 1, finite or +inf, got {white!r}")
    return float(scale), float(white)


def check_outputs(outputs: Sequence[str] = ("rgb",)) -> tuple:
    """The outputs of apply and display: a non-empty subset of OUTPUTS, ValueError otherwise.  Pure."""
    outs = tuple(outputs)
    if not outs or any(o not in OUTPUTS for o in outs) or len(set(outs)) != len(outs):
        raise ValueError(f"outputs: a non-empty subset of {OUTPUTS}, got {outs}")
    return outs


class FilmDisplay:
    """The display of one film's frames (or, with shape=, of frames of another size on the film's device and stream).

    State on the device: `histogram`, the (257,) int32 counts of the last metered frame (256 bins and the excluded pixels), and the
    exposure record, eight words that rtd_expose reads and writes.  Under "auto" (the default) meter() counts the frame and moves
    the exposure: the first frame after construction or reset() takes its target scale as it is, a later one moves the scale by
    `rate` of the way to its target.  set_exposure() fixes scale and white until auto().  apply() displays a frame under the record
    as it stands; display() is meter() then apply().

    Everything is enqueued on film.stream and nothing waits for the device but exposure().  The tensors returned are the display's
    own and are written again by the next call.  Not thread-safe."""

    def __init__(self, film, shape=None, curve: str = "filmic", key: float = KEY, key_percentile: float = KEY_PERCENTILE,
                 white_percentile: float = WHITE_PERCENTILE, rate: float = 1.0, scale_range=SCALE_RANGE, dither: bool = False):
        if shape is None:
            shape = (getattr(film, "rows", None), getattr(film, "width", None))
        self.settings = check_display(shape, curve, key, key_percentile, white_percentile, rate, scale_range, dither)
        film._check_open()
        self._lib = _display_lib.load()
        self.film = film
        self.form = HISTOGRAM_FORM
        self._manual: Optional[tuple] = None
        torch = film._torch
        with torch.cuda.stream(film.stream):
            self._hist = torch.zeros((_display_lib.HIST_WORDS,), dtype=torch.int32, device=film.device)
            # scale 1, white +inf, target 1, frames 0: what apply() shows before any frame was metered
            self._record = torch.tensor([0x3F800000, 0x7F800000, 0x3F800000, 0, 0, 0, 0, 0], dtype=torch.int32).to(film.device)
        self._out: dict = {}

    # ---- state

    def _check_open(self):
        if getattr(self, "_record", None) is None:
            raise ValueError("the display is closed")
        self.film._check_open()

    def close(self):
        """Wait for the film's stream and drop the tensors.  The film stays the caller's."""
        if getattr(self, "_record", None) is None:
            return
        if self.film.accum is not None:
            self.film.sync()
        self._hist = self._record = None
        self._out = {}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def histogram(self):
        """The counts of the last metered frame: a (257,) int32 tensor on the film's device, bins 0 ... 255 and the excluded."""
        self._check_open()
        return self._hist

    def exposure(self) -> dict:
        """The exposure record as a dict of its eight fields (scale, white, target: floats; bin_key, bin_white, counted, excluded,
        frames: ints).  Waits for the film's stream: for inspection, not for the frame loop."""
        self._check_open()
        self.film.sync()
        words = self._record.cpu()
        f = words[:3].view(self.film._torch.float32).tolist()
        return dict(zip(_display_lib.RECORD_FIELDS, f + [int(v) & 0xFFFFFFFF for v in words[3:].tolist()]))

    def reset(self):
        """frames = 0: the next metered frame takes its target as it is."""
        self._check_open()
        with self.film._torch.cuda.stream(self.film.stream):
            self._record[7:].zero_()

    def set_exposure(self, scale: float, white: float = math.inf):
        """A fixed exposure (RTD_MANUAL), written to the record now and kept by meter() until auto()."""
        manual = check_exposure(scale, white)
        self._check_open()
        self._manual = manual
        self._expose()

    def auto(self):
        """Back to the metered exposure.  The adaptation starts again (reset()): a manual scale is no frame's exposure to move on
        from."""
        self._check_open()
        if self._manual is not None:
            self._manual = None
            self.reset()

    # ---- the calls

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

    def _expose(self):
        s = self.settings
        if self._manual is not None:
            a = _display_lib.ExposeArgs(mode=_display_lib.MODES["manual"], scale=self._manual[0], white=self._manual[1],
                                        record=self._record.data_ptr())
        else:
            a = _display_lib.ExposeArgs(mode=_display_lib.MODES["auto"], key=s.key, key_q16=s.key_q16, white_q16=s.white_q16, rate=s.rate,
                                        scale_min=s.scale_min, scale_max=s.scale_max, hist=self._hist.data_ptr(),
                                        record=self._record.data_ptr())
        _display_lib.check("rtd_expose", self._lib.rtd_expose(a, self.film.stream.cuda_stream))

    def meter(self, linear) -> None:
        """Count the frame into `histogram` and move the exposure record: rtd_meter and rtd_expose on the film's stream.  Under
        set_exposure() the frame is counted and the record keeps the manual values."""
        self._check_open()
        self._check_linear(linear)
        R, W = self.settings.shape
        a = _display_lib.MeterArgs(W=W, R=R, form=_display_lib.FORMS[self.form], linear=linear.data_ptr(), hist=self._hist.data_ptr())
        _display_lib.check("rtd_meter", self._lib.rtd_meter(a, self.film.stream.cuda_stream))
        self._expose()

    def apply(self, linear, outputs: Sequence[str] = ("rgb",)) -> dict:
        """The frame under the record as it stands: {output: tensor} out of rgb (R, W, 3) uint8 and f32 (R, W, 3) float32, the
        value before quantisation.  One rtd_apply on the film's stream."""
        outs = check_outputs(outputs)
        self._check_open()
        self._check_linear(linear)
        torch = self.film._torch
        s = self.settings
        R, W = s.shape
        with torch.cuda.stream(self.film.stream):
            for o in outs:
                if o not in self._out:
                    self._out[o] = torch.empty((R, W, 3), dtype=torch.uint8 if o == "rgb" else torch.float32, device=self.film.device)
        ptr = lambda o: self._out[o].data_ptr() if o in outs else None
        a = _display_lib.ApplyArgs(W=W, R=R, curve=_display_lib.CURVES[s.curve], dither=int(s.dither), linear=linear.data_ptr(),
                                   record=self._record.data_ptr(), out_f32=ptr("f32"), out_rgb=ptr("rgb"))
        _display_lib.check("rtd_apply", self._lib.rtd_apply(a, self.film.stream.cuda_stream))
        return {o: self._out[o] for o in outs}

    def display(self, linear, outputs: Sequence[str] = ("rgb",)) -> dict:
        """meter(linear), then apply(linear, outputs)."""
        outs = check_outputs(outputs)
        self.meter(linear)
        return self.apply(linear, outs)
