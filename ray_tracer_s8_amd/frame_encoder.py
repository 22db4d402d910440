"""Baseline JPEG encoding of a frame in device memory.

    with rt.Film(scene, strips, moments=True) as film:
        display, encoder = rt.FilmDisplay(film), rt.FrameEncoder(film, quality=90)
        film.render_pass(0, 32)
        rgb = display.display(film.resolve_guided(planes, ("linear",))["linear"])["rgb"]
        open("frame.jpg", "wb").write(encoder.encode(rgb))

The reference's controller ends a frame as a JPEG (controller_shim.encode_jpeg restates it with Pillow on the host).  FrameEncoder
writes that file on the device: a baseline sequential JFIF file, 4:4:4, with the Huffman tables of T.81 Annex K.3 and restart
intervals, which are what lets the entropy coding run in parallel.  The format is normative in jpeg_csrc/rt_jpeg.h and runs in HIP
kernels of a private library (lib/librt_jpeg.so, _jpeg_lib.py).  Only the compressed bytes cross to the host.

`rgb` is any contiguous (R, W, 3) uint8 tensor on the film's device: the "rgb" of a film, of its resolves, of FilmDisplay.apply and of
an upsampled frame (an encoder made with shape=).  The encoder reads it and never writes it.

This module imports without torch; the library is loaded when a FrameEncoder is constructed."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

from . import _jpeg_lib

# The default interval, 16 MCUs: the fastest of a row of MCUs, 64 and 16 as measured (DESIGN.md 4.32 "Measured", tools/jpeg_bench.py):
# 219 us of kernels a 1920 x 1080 frame against 238 and 314, for files 0.3 % larger.  A wave takes an interval in the stuffing passes,
# so short intervals fill the device.
QUALITY, INTERVAL = 90, 16


class Settings(NamedTuple):
    shape: tuple                  # (R, W)
    quality: int
    interval: int
    capacity: int


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def check_encoder(shape, quality: int = QUALITY, interval: Optional[int] = None, capacity: Optional[int] = None) -> Settings:
    """The checks of FrameEncoder's arguments, all of them ValueError and none of them a GPU call.  shape: (R, W), ints in
    1 ... 65535.  quality: an int in 1 ... 100.  interval: MCUs a restart interval, an int in 1 ... 65535, or None for INTERVAL.
    capacity: the bytes of the output buffer, an int above the header's 629 and below 2^32, or None for the header plus R W 3.
    Returns the Settings the calls are made with.  Pure: no torch, no GPU."""
    if not isinstance(shape, (tuple, list)) or len(shape) != 2 or not all(_is_int(v) and 1 <= v <= _jpeg_lib.MAX_SIDE for v in shape):
        raise ValueError(f"shape: (rows, columns), ints in 1 ... {_jpeg_lib.MAX_SIDE}, got {shape!r}")
    if not _is_int(quality) or not 1 <= quality <= 100:
        raise ValueError(f"quality: an int in 1 ... 100, got {quality!r}")
    if interval is None:
        interval = INTERVAL
    if not _is_int(interval) or not 1 <= interval <= _jpeg_lib.MAX_INTERVAL:
        raise ValueError(f"interval: an int in 1 ... {_jpeg_lib.MAX_INTERVAL}, got {interval!r}")
    if capacity is None:
        capacity = _jpeg_lib.HEADER_LEN + shape[0] * shape[1] * 3
    if not _is_int(capacity) or not _jpeg_lib.HEADER_LEN < capacity < 1 << 32:
        raise ValueError(f"capacity: an int above {_jpeg_lib.HEADER_LEN} and below 2^32, got {capacity!r}")
    return Settings((shape[0], shape[1]), quality, interval, capacity)


class FrameEncoder:
    """The JPEG encoder of one film's frames (or, with shape=, of frames of another size on the film's device and stream).

    encode_device(rgb) enqueues the encode on film.stream and returns (out, record): the encoder's own output tensor, whose first
    record[0] bytes are the file once the stream has run, and the eight-word device record (total, raw, stuffed, intervals, overflow).
    Nothing waits.  encode(rgb) is encode_device plus one read of the record and one copy of `total` bytes: it returns the file as
    bytes.  If the file does not fit `capacity` (the default holds any frame that compresses at all), encode retries once with a
    buffer of `bound` bytes, which the encoder then keeps; the device record says so in `overflow` for a caller of encode_device.

    The tensors returned are the encoder's own and are written again by the next call.  Not thread-safe."""

    def __init__(self, film, shape=None, quality: int = QUALITY, interval: Optional[int] = None, capacity: Optional[int] = None):
        if shape is None:
            shape = (getattr(film, "rows", None), getattr(film, "width", None))
        self.settings = check_encoder(shape, quality, interval, capacity)
        film._check_open()
        self._lib = _jpeg_lib.load()
        self.film = film
        s = self.settings
        R, W = s.shape
        n = C.c_uint64(0)
        _jpeg_lib.check("rtj_bound", self._lib.rtj_bound(W, R, s.interval, C.byref(n)))
        self._bound = n.value
        _jpeg_lib.check("rtj_scratch_bytes", self._lib.rtj_scratch_bytes(W, R, s.interval, C.byref(n)))
        head = (C.c_uint8 * _jpeg_lib.HEADER_LEN)()
        a = _jpeg_lib.EncodeArgs(W=W, R=R, quality=s.quality, interval=s.interval)
        got = C.c_uint64(0)
        _jpeg_lib.check("rtj_header", self._lib.rtj_header(a, head, _jpeg_lib.HEADER_LEN, C.byref(got)))
        self._header = bytes(head[:got.value])
        torch = film._torch
        with torch.cuda.stream(film.stream):
            self._scratch = torch.empty((n.value,), dtype=torch.uint8, device=film.device)
            self._record = torch.zeros((_jpeg_lib.RECORD_WORDS,), dtype=torch.int32, device=film.device)
        self._out = None
        self._allocate(s.capacity)

    def _allocate(self, capacity: int):
        """The output buffer with the header in its first bytes."""
        torch = self.film._torch
        head = torch.frombuffer(bytearray(self._header), dtype=torch.uint8)
        with torch.cuda.stream(self.film.stream):
            self._out = torch.empty((capacity,), dtype=torch.uint8, device=self.film.device)
            self._out[:len(self._header)].copy_(head)
        self.film.stream.synchronize()                 # (the host bytes are gone after this line)

    # ---- state

    def _check_open(self):
        if getattr(self, "_record", None) is None:
            raise ValueError("the encoder is closed")
        self.film._check_open()

    def close(self):
        """Wait for the film's stream and drop the tensors.  The film stays the caller's."""
        if getattr(self, "_record", None) is None:
            return
        if self.film.accum is not None:
            self.film.sync()
        self._scratch = self._record = self._out = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def header(self) -> bytes:
        """The bytes SOI ... SOS of every file this encoder writes."""
        return self._header

    @property
    def tables(self) -> tuple:
        """The two quantisation tables, 64 ints each in natural (row) order, as the header carries them."""
        zigzag = _ZIGZAG
        out = []
        for at in (25, 94):                            # the entries of DQT 0 and DQT 1 in the header
            t = [0] * 64
            for k, n in enumerate(zigzag):
                t[n] = self._header[at + k]
            out.append(tuple(t))
        return tuple(out)

    @property
    def bound(self) -> int:
        """The most bytes a file of this shape and interval can have (rtj_bound)."""
        return self._bound

    @property
    def capacity(self) -> int:
        self._check_open()
        return int(self._out.numel())

    # ---- the calls

    def _check_rgb(self, rgb):
        torch = self.film._torch
        R, W = self.settings.shape
        if not isinstance(rgb, torch.Tensor):
            raise ValueError(f"rgb: a tensor, got {type(rgb).__name__}")
        if tuple(rgb.shape) != (R, W, 3) or rgb.dtype != torch.uint8:
            raise ValueError(f"rgb: a ({R}, {W}, 3) uint8 tensor, got {tuple(rgb.shape)} {rgb.dtype}")
        if rgb.device != self.film.device:
            raise ValueError(f"rgb: on {rgb.device}, the film is on {self.film.device}")
        if not rgb.is_contiguous() or rgb.data_ptr() % 4:
            raise ValueError("rgb: a contiguous tensor at a 4-byte boundary")

    def encode_device(self, rgb) -> tuple:
        """Enqueue the encode on the film's stream: (out, record), the encoder's output tensor and its (8,) int32 device record."""
        self._check_open()
        self._check_rgb(rgb)
        s = self.settings
        R, W = s.shape
        a = _jpeg_lib.EncodeArgs(W=W, R=R, quality=s.quality, interval=s.interval, rgb=rgb.data_ptr(), scratch=self._scratch.data_ptr(),
                                 scratch_bytes=self._scratch.numel(), out=self._out.data_ptr(), capacity=self._out.numel(),
                                 header_len=len(self._header), record=self._record.data_ptr())
        _jpeg_lib.check("rtj_encode", self._lib.rtj_encode(a, self.film.stream.cuda_stream))
        return self._out, self._record

    def record(self) -> dict:
        """The record of the last encode as a dict (total, raw, stuffed, intervals, overflow).  Waits for the film's stream."""
        self._check_open()
        self.film.stream.synchronize()
        words = [int(v) & 0xFFFFFFFF for v in self._record.cpu().tolist()]
        return dict(zip(_jpeg_lib.RECORD_FIELDS, words))

    def encode(self, rgb) -> bytes:
        """The frame as a complete JPEG file: encode_device, one read of the record, one copy of `total` bytes."""
        out, _ = self.encode_device(rgb)
        rec = self.record()
        if rec["overflow"]:
            self._allocate(max(self._bound, rec["total"]))
            out, _ = self.encode_device(rgb)
            rec = self.record()
            if rec["overflow"]:
                raise RuntimeError(f"a file of {rec['total']} bytes is beyond the encoder's bound of {self._bound}")
        return out[:rec["total"]].cpu().numpy().tobytes()


_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
           56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
